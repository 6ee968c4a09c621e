"""The call plan (csrc/call_plan.cpp: which kernels a search call launches, on which visited set) without a device, through
tests/cpp/call_plan_units.cpp -- a driver compiled from the sources of call_plan.cpp, sizing.cpp and walk_plan.cpp (host code only).

tests/golden/call_plan_cases.txt holds one line per search call traced on an MI355X before the plan was cut out of search_core.cpp: the
call's inputs (the device's CU count among them), its sizing history, and what ran -- the first-pass kernel, its grid and LDS bytes, the
retry kernel or "copy" / "none", and whether a stand-alone re-rank kernel followed.  The cases sit on either side of each automatic rule
(two-wavefront walk, bitmap pass, late rows, speculative tail, calm history, retry action, fused re-rank)."""
import os
import subprocess

import pytest

import walk_instances as wi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gbnns_dim_red_amd", "csrc")
LIBDIR = os.path.join(ROOT, "gbnns_dim_red_amd", "lib")


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    import gbnns_dim_red_amd as g
    g.build_library()
    exe = str(tmp_path_factory.mktemp("units") / "call_plan_units")
    # GBNNS_UNITS_SAN=1: the same driver with AddressSanitizer + UBSan on its host code (a plain executable: nothing is preloaded)
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-fsanitize=address,undefined", "-g"] \
        if os.environ.get("GBNNS_UNITS_SAN") == "1" else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "call_plan_units.cpp")] + [os.path.join(CSRC, u) for u in ("call_plan.cpp", "sizing.cpp", "walk_plan.cpp")] +
                          ["-o", exe, "-L" + LIBDIR, "-lgbnns_hip", "-Wl,-rpath," + LIBDIR])

    def run(*args):
        env = {k: v for k, v in os.environ.items() if k not in ("GBNNS_BITMAP_MIN_EF", "GBNNS_DEBUG_SIZING", "GBNNS_WIDE2", "GBNNS_STAMPS_GENERIC")}
        p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
        return p.stdout
    return run


def test_traced_calls_get_the_same_plan(unit):
    out = unit("golden", os.path.join(ROOT, "tests", "golden", "call_plan_cases.txt"))
    assert "golden: 32 lines, 0 failed" in out, out


def test_plan_conditions_over_the_census_grid(unit):
    """First-pass LDS within 160 KB unless all_general; fuse only off the LDS-list pass and within the re-rank room; a bitmap pass without
    coop, tags, a byte walk or a half walk; a half-base handle's LOWQ call never fused; skip_retry only with an automatic capacity and not all_general; the history untouched; the same plan twice."""
    out = unit("grid", ",".join(str(d) for d in wi.DIMS), ",".join(str(e) for e in wi.BEAMS))
    plans = 5 * 2 * len(wi.DIMS) * len(wi.BEAMS) * 3 * 2
    assert "grid: %d plans, 0 failed" % plans in out, out


def test_plan_walk_is_the_recorded_function(unit):
    """plan_walk over the cross product of everything it reads -- both environments x metric x dim x n either side of the two-wavefront walk's
    and the 24-bit ids' limits x adjacency width x auxiliary graph x beam x entry points x force_wide, for each of three passes and eighteen
    feature variants: per (variant, pass) one digest of every plan's kernel name, family and layout facts.  tests/golden/walk_plan_grid.txt was
    recorded by this driver built against the commits its header names: the first fifteen variants before WalkInstance's switches became one
    set of named flags, the three half-walk variants before the handle's row kind became one field."""
    with open(os.path.join(ROOT, "tests", "golden", "walk_plan_grid.txt")) as f:
        want = [line.rstrip("\n") for line in f if not line.startswith("#")]
    assert want[0] == "walkgrid: %d plans" % (18 * 3 * 2 * 2 * len(wi.DIMS) * 4 * 3 * 2 * len(wi.BEAMS) * 2 * 2) and len(want) == 1 + 18 * 3
    got = unit("walkgrid", ",".join(str(d) for d in wi.DIMS), ",".join(str(e) for e in wi.BEAMS)).splitlines()
    assert got == want, [pair for pair in zip(got, want) if pair[0] != pair[1]]
