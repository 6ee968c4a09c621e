"""The census of the projection kernel instances without a device: gbnns_debug_project_plan names what every case of
tests/projection_instances.py launches, the names cover the instance list less the unreachable ones exactly, the instance list is what the
built code object holds, no knob, shape or flight state reaches an instance the table calls unreachable, and at another CU count the
one-launch kernel still gets a strip whose LDS fits.  tests/test_gpu_projection_instances.py runs what is proven here."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import pytest

import projection_instances as pi

INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gbnns_dim_red_amd", "lib", "libgbnns_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/"


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def _plan(g, c, cus=pi.CUS):
    return g.project_plan(c.d, c.dh, c.dl, c.nq, cus, c.flight, c.mfma, **c.knob_dict)


def _args(name):
    return [int(a) if a.isdigit() else a == "true" for a in name[name.index("<") + 1:-1].split(", ")]


def test_exports(g):
    from gbnns_dim_red_amd import binding
    for name in ("gbnns_debug_project_plan", "gbnns_index_project_last"):
        assert name in binding.SYMBOLS and hasattr(g.load_library(), name), name
    assert callable(g.project_plan) and callable(g.Index.project_last)


def test_every_case_launches_the_instances_it_names(g):
    assert len({c.id for c in pi.CASES}) == len(pi.CASES)
    for c in pi.CASES:
        assert _plan(g, c) == c.names, c.id


def test_the_names_cover_every_reachable_instance_exactly():
    want = pi.instance_names()
    assert {f: len(v) for f, v in want.items()} == {"net": 16, "slab": 20, "layer": 3, "vec": 3, "sw": 2, "narrow": 3, "mfma_layer": 2,
                                                   "mfma_net": 3, "normalize": 1}
    every = set().union(*want.values())
    assert sum(len(v) for v in want.values()) == len(every) == 53
    assert set(pi.UNREACHABLE) <= every and len(pi.UNREACHABLE) == 6 and all(pi.UNREACHABLE.values())
    got = {n for c in pi.CASES for n in c.names}
    assert got == every - set(pi.UNREACHABLE), (sorted(every - set(pi.UNREACHABLE) - got), sorted(got - every))
    # the one-launch kernel: every (form, A) with a d_low of either B3, and B3 = 4 with one pass (<= 64) and with two (> 64) in either form
    for half in (False, True):
        dls = {c.dl for c in pi.CASES if c.names[0].startswith("mlp_net_kernel") and c.flight == half}
        assert {16, 32} <= dls and dls & {48, 64} and {72, 128} <= dls, (half, dls)
    assert any(c.dl % 4 for c in pi.CASES if c.names[0].startswith("mlp_net_kernel"))
    # calls in flight are the half-CU form, plain calls the whole-CU form: no case forces a form by knob
    for c in pi.CASES:
        if c.names[0].startswith("mlp_net_kernel"):
            assert (_args(c.names[0])[0] == 4) == c.flight and not c.knobs, c.id
    # the SIFT net once per form at A = 5, and at RB = 3
    sift = {c.names[0] for c in pi.CASES if (c.d, c.dh, c.dl) == (128, 256, 32)}
    assert sift == {"mlp_net_kernel<8, 5, 8, 2, 2>", "mlp_net_kernel<4, 5, 8, 2, 4>", "mlp_mfma_net_kernel<3>"}


def test_shapes():
    """The rules of the module's docstring, case by case."""
    for c in pi.CASES:
        first = c.names[0]
        if first.startswith("mlp_net_kernel"):
            nw, a, bh, b3, go = _args(first)
            gq, q = 16 // go, 16 // go * a
            lo = {2: 2048, 3: 4097, 4: 6145, 5: 8193}[a]
            assert lo <= c.nq < lo + 64 and c.d % 8 == 0 and c.dh % 8 == 0, c.id
            assert (c.nq % q == 0) == (c.nq == pi.NET_WHOLE_BLOCKS) and (c.nq % q == 0 or c.nq % q % gq), c.id
        elif first.startswith("mlp_mfma_net_kernel"):
            rows = pi.mfma_rows(c.nq)
            assert _args(first)[0] == -(-rows // 16) and (c.nq % rows or rows == 1), c.id
            dst, src = pi.copy_rows(c.nq)
            if c.nq in pi.MFMA_NQ.values():   # copies in every row block of workgroup 1's share and in the last, partial workgroup
                assert {d // 16 for d in (dst[dst < 2 * rows] - rows).tolist()} == set(range(-(-rows // 16))), c.id
                assert (dst >= (c.nq - 1) // rows * rows).any() and (src < min(rows, 16)).all() and (dst < c.nq).all(), c.id
        for name in c.names:
            if name.startswith("mlp_slab_kernel"):
                nw, a, relu, norm = _args(name)
                assert c.nq % (8 * a), (c.id, name)     # a partial last strip
                if nw == 8:   # the class's range of batches for the layer's columns
                    gy = -(-(c.dh if relu else c.dl) // 128)
                    top = pi.SLAB_WIDE_MAX[gy]
                    assert top.get(a - 1, 0) < c.nq <= top[a], (c.id, name)
                else:
                    assert pi.SLAB_NARROW_MAX.get(a - 1, 0) < c.nq <= pi.SLAB_NARROW_MAX[a], (c.id, name)
        assert c.nq == pi.NET_WHOLE_BLOCKS or (c.nq % 64 and c.nq % 32), c.id     # a partial last tile of every tile size
    # widths per family of exact instances: one d with d % 16 == 8 and one multiple of 64; hidden widths that are and are not whole passes
    for family in ("mlp_net_kernel<8", "mlp_net_kernel<4", "mlp_slab_kernel<8", "mlp_layer_vec_kernel", "mlp_mfma_net_kernel"):
        ds = {c.d for c in pi.CASES if any(n.startswith(family) for n in c.names)}
        assert any(d % 16 == 8 for d in ds) and any(d % 64 == 0 for d in ds), (family, ds)
    for family in ("mlp_net_kernel<8", "mlp_net_kernel<4", "mlp_slab_kernel<8"):
        dhs = {c.dh for c in pi.CASES if any(n.startswith(family) for n in c.names)}
        assert any(dh % 128 for dh in dhs) and any(dh % 128 == 0 for dh in dhs), (family, dhs)
    assert any(c.d % 4 and c.dh % 4 for c in pi.CASES if c.names[0].startswith("mlp_layer_kernel"))
    assert any(c.dh <= 32 for c in pi.CASES if "mlp_narrow_kernel<true, false>" in c.names)


def _demangle(name):
    """__cxa_demangle of the C++ runtime every process here has loaded."""
    cxx = C.CDLL("libstdc++.so.6")
    cxx.__cxa_demangle.restype = C.c_void_p
    cxx.__cxa_demangle.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    status = C.c_int(-1)
    p = cxx.__cxa_demangle(name.encode(), None, None, C.byref(status))
    assert status.value == 0 and p, name
    text = C.string_at(p).decode()
    C.CDLL(None).free(C.c_void_p(p))
    return text


def test_instance_list_is_the_code_objects(tmp_path):
    """instance_names() against the kernel names of the built library's gfx950 code object (names only)."""
    if not os.path.exists(LIB):
        pytest.fail(LIB + " is missing: run __graft_entry__.build() first")
    tools = [LLVM + t for t in ("llvm-objdump", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm llvm tools not found")
    lib = shutil.copy(LIB, tmp_path)
    subprocess.run([tools[0], "--offloading", lib], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    mangled = set()
    for f in os.listdir(tmp_path):
        if f.endswith("gfx950"):
            text = subprocess.run([tools[1], "--notes", os.path.join(tmp_path, f)], check=True, capture_output=True, text=True).stdout
            mangled |= set(re.findall(r"\.name:\s+(\S+)", text))
    plain = "\n".join(_demangle(m) for m in sorted(mangled) if "mlp_" in m or "normalize_kernel" in m)
    found = set()
    for m in re.finditer(r"\b(mlp_(?:net|slab|layer|layer_vec|layer_sw|narrow|layer_mfma|mfma_net)_kernel<[^>]*>|normalize_kernel)\(", plain):
        found.add(m.group(1))
    want = set().union(*pi.instance_names().values())
    assert found == want, (sorted(want - found), sorted(found - want))


def _thresholds(cus, dh, dl):
    """Batch sizes at every threshold of the rules, +- 1: the tiles, the one-launch kernel's domain and strips (16 A CUs), the row blocks
    of the matrix-core kernel, "mlp_small" and 32 times it, and the slab kernel's classes (8 A floor(CUs / gy)) for the columns gy of the
    net's own layers."""
    t = {1, 32, 64, 2048, 4096, 32 * 4096, 200000, 200001}
    for a in (1, 2, 3, 4, 5):
        t.add(16 * a * cus)
        for width in (dh, dl):
            t.add(8 * a * (cus // -(-width // (128 if width > 64 else 64))))
    return sorted({v + e for v in t for e in (-1, 0, 1) if 1 <= v + e <= 200001})


def test_no_unreachable_instance_ever_comes_out(g):
    """A grid over widths 8 .. 1 032 of every % 4 / % 8 / % 16 class, batches of 1 .. 200 001 queries at every threshold +- 1, both flight
    states, every value of the three knobs ("mlp_small": never, always, the default; it is read in flight only), the matrix-core option
    (which reads no knob) and two CU counts."""
    lib = g.load_library()
    buf = C.create_string_buffer(512)
    ds = (8, 9, 10, 12, 40, 64, 264, 1032)
    dhs = (8, 10, 12, 33, 64, 72, 512, 1032)
    dls = (8, 10, 12, 32, 46, 64, 65, 128, 129)
    for vals in (ds, dhs, dls):
        assert {v % 4 for v in vals} >= {0, 1, 2} and {v % 8 for v in vals} >= {0, 4} and {v % 16 for v in vals} >= {0, 8}, vals
    plain = [(n, s, 4096) for n in (0, 1, 2, 3) for s in (0, 1, 2)]
    flying = [(n, s, m) for n in (0, 1, 2, 3) for s in (0, 1, 2) for m in (0, 1, 4096)]
    bad = {n.encode() for n in pi.UNREACHABLE}
    every = {n.encode() for n in set().union(*pi.instance_names().values())}
    seen, calls = set(), 0
    for cus in (256, 304):
        for d, dh, dl in itertools.product(ds, dhs, dls):
            for nq in _thresholds(cus, dh, dl):
                for flight, mfma, knobs in ((0, 0, plain), (1, 0, flying), (0, 1, plain[:1]), (1, 1, flying[-1:])):
                    for n, s, m in knobs:
                        assert lib.gbnns_debug_project_plan(d, dh, dl, nq, cus, flight, mfma, n, s, m, buf, 512) == 0
                        calls += 1
                        if buf.value not in seen:
                            seen.add(buf.value)
                            names = set(buf.value.split(b"\n"))
                            assert names <= every and not names & bad, (d, dh, dl, nq, cus, flight, mfma, n, s, m, buf.value)
    print("plans asked:", calls, "distinct:", len(seen))
    # ... and the grid reaches every other instance
    assert {n for s in seen for n in s.split(b"\n")} == every - bad


def test_strips_fit_the_lds_at_another_cu_count(g):
    """Whatever A the plan picks for 64 .. 304 compute units, a workgroup of that form and strip fits its LDS (gbnns_debug_net_lds), and
    the instance is one of the sixteen."""
    lib = g.load_library()
    size, ok = C.c_uint64(), C.c_int()
    nets = sorted({(c.d, c.dh, c.dl) for c in pi.CASES if c.names[0].startswith("mlp_net_kernel")} | {(128, 320, 32), (256, 448, 64), (128, 384, 32)})
    picked = set()
    for cus in (64, 104, 128, 228, 256, 304):
        for d, dh, dl in nets:
            for nq in (2048, 2049, 3000, 4097, 6145, 8193, 10000, 10241, 20000, 200000):
                for flight in (False, True):
                    names = g.project_plan(d, dh, dl, nq, cus, flight)
                    assert len(names) == 1 and names[0] in pi.instance_names()["net"], (cus, d, dh, dl, nq, flight, names)
                    nw, a, bh, b3, go = _args(names[0])
                    assert lib.gbnns_debug_net_lds(d, dh, dl, int(go == 4), a, C.byref(size), C.byref(ok)) == 0
                    assert ok.value and size.value <= (80 if go == 4 else 160) * 1024, (cus, d, dh, dl, nq, names, size.value)
                    assert b3 == (2 if dl <= 32 else 4)
                    picked.add((go, a))
    assert picked == {(go, a) for go in (2, 4) for a in (2, 3, 4, 5)}
    # (nets whose half-CU workgroup does not fit keep the whole-CU form in flight)
    assert g.project_plan(128, 384, 32, 3000, 256, True) == ("mlp_net_kernel<8, 2, 8, 2, 2>",)


def test_project_plan_refusals(g):
    lib = g.load_library()
    buf = C.create_string_buffer(512)
    ok = (128, 256, 32, 10000, 256, 0, 0, 1, 1, 4096)
    assert lib.gbnns_debug_project_plan(*ok, buf, 512) == 0 and buf.value == b"mlp_net_kernel<8, 5, 8, 2, 2>"
    assert lib.gbnns_debug_project_plan(*ok, None, 512) == INVALID and lib.gbnns_debug_project_plan(*ok, buf, 0) == INVALID
    for i, v in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 1 << 31), (4, 0), (7, 4), (7, -1), (8, 3), (9, -1)):
        bad = list(ok)
        bad[i] = v
        assert lib.gbnns_debug_project_plan(*bad, buf, 512) == INVALID, bad
    short = C.create_string_buffer(b"x" * 8, 8)
    assert lib.gbnns_debug_project_plan(*ok, short, 8) == 0 and short.value == b"mlp_net"
    assert lib.gbnns_index_project_last(None, buf, 512) == INVALID
    # the defaults of the binding are the library's
    assert g.project_plan(128, 256, 32, 10000) == ("mlp_net_kernel<8, 5, 8, 2, 2>",)
    assert g.project_plan(128, 256, 32, 10000, in_flight=True) == ("mlp_net_kernel<4, 5, 8, 2, 4>",)
    assert g.project_plan(128, 256, 32, 10000, in_flight=True, mlp_net=2) == ("mlp_net_kernel<8, 5, 8, 2, 2>",)
    assert g.project_plan(128, 256, 32, 10000, mlp_net=3) == ("mlp_net_kernel<4, 5, 8, 2, 4>",)
    assert g.project_plan(128, 256, 32, 10000, mfma=True) == ("mlp_mfma_net_kernel<3>",)
    assert g.project_plan(128, 256, 32, 10000, mlp_net=0) == ("mlp_layer_vec_kernel<true, false>",) * 2 + ("mlp_narrow_kernel<false, true>",)
    assert g.project_plan(960, 1024, 64, 1000) == ("mlp_slab_kernel<8, 4, true, false>",) * 2 + ("mlp_slab_kernel<4, 1, false, true>",)
    assert g.project_plan(960, 1024, 64, 1000, in_flight=True)[:2] == ("mlp_layer_vec_kernel<true, false>",) * 2   # (wide slabs wait for a CU to drain)
    assert g.project_plan(960, 1024, 64, 1000, in_flight=True, mlp_slab=2)[:2] == ("mlp_slab_kernel<8, 4, true, false>",) * 2
