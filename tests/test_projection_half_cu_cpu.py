"""The half-CU form of the one-launch projection (csrc/mlp_net.hip), host side and code object (CPU test: no GPU needed).

A workgroup of the form is four wavefronts and at most 80 KB of LDS, so that one fits a CU as soon as the walks of the other
batches in flight have left half of it: a SIMD that still holds four 64-register walk wavefronts has 256
vector registers free -- the form is held to 240 --, sixteen walk wavefronts of 5 120 bytes leave 81 920 bytes of LDS.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

import gbnns_dim_red_amd as g
from gbnns_dim_red_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gbnns_dim_red_amd", "lib", "libgbnns_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
HALF_LDS = 80 * 1024


@pytest.fixture(scope="module")
def lib():
    g.build_library()
    return g.load_library()


def test_mlp_net_knob_takes_the_four_values(lib):
    """gbnns_debug_knob("mlp_net", v) accepts 0 (never), 1 (the rule), 2 (whole-CU form), 3 (half-CU form where it fits).  In a
    child process: the value set would be the default of every handle this process creates afterwards."""
    script = ("import ctypes, sys\n"
              "lib = ctypes.CDLL(sys.argv[1])\n"
              "lib.gbnns_debug_knob.argtypes = [ctypes.c_char_p, ctypes.c_int]\n"
              "print([lib.gbnns_debug_knob(b'mlp_net', v) for v in (0, 1, 2, 3)])\n")
    p = subprocess.run([sys.executable, "-c", script, binding._LIB_PATH], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == "[0, 0, 0, 0]", p.stdout


def _net_lds(lib, d, dh, dl, form, a):
    size, ok = ctypes.c_uint64(), ctypes.c_int()
    rc = lib.gbnns_debug_net_lds(d, dh, dl, form, a, ctypes.byref(size), ctypes.byref(ok))
    assert rc == 0, lib.gbnns_last_error()
    return size.value, bool(ok.value)


def test_half_cu_footprint(lib):
    """Two activation images of 4 x net_gstride(256, 5) floats and four staging pairs of 9 216 bytes: 78 080 bytes for the SIFT
    net at five queries per lane; two such blocks fit a CU's 160 KB.  The form takes exactly the nets whose block of 16 queries
    (four per lane, as the whole-CU form's rule counts them) stays within 80 KB."""
    assert _net_lds(lib, 128, 256, 32, 1, 5) == (2 * 4 * (256 * 5 + 8) * 4 + 4 * 9216, True)
    assert _net_lds(lib, 128, 256, 32, 1, 5)[0] == 78080 and 2 * 78080 <= 160 * 1024
    admitted = {(128, 256, 32): True, (200, 72, 32): True, (96, 128, 64): True, (960, 256, 64): False, (128, 320, 32): True,
                (128, 384, 32): False, (256, 512, 64): False}
    for (d, dh, dl), want in admitted.items():
        size4, ok = _net_lds(lib, d, dh, dl, 1, 4)
        assert ok == want and ok == (size4 <= HALF_LDS), (d, dh, dl, size4, ok)
        if ok:   # whatever strip the launcher then picks among those that fit, a block is half a CU's at most
            assert min(_net_lds(lib, d, dh, dl, 1, a)[0] for a in (2, 3, 4, 5)) <= size4 <= HALF_LDS
    # the whole-CU form's footprint is what it was: eight groups, eight staging pairs of 4 608 bytes
    assert _net_lds(lib, 128, 256, 32, 0, 5)[0] == 2 * 8 * (256 * 5 + 8) * 4 + 8 * 4608
    assert lib.gbnns_debug_net_lds(128, 256, 32, 2, 5, ctypes.byref(ctypes.c_uint64()), ctypes.byref(ctypes.c_int())) == 1
    assert lib.gbnns_debug_net_lds(128, 256, 32, 1, 6, ctypes.byref(ctypes.c_uint64()), ctypes.byref(ctypes.c_int())) == 1


def test_half_cu_instances_in_the_code_object(tmp_path):
    """The shipped code object holds 256-thread instances of mlp_net_kernel -- the one for five queries per lane among them --, each
    within 240 vector registers (accumulation registers included), with no scratch and nothing spilled."""
    if not os.path.exists(LIB):
        pytest.fail(LIB + " is missing: run __graft_entry__.build() first")
    if not os.path.exists(READELF) or not os.path.exists(OBJDUMP):
        pytest.skip("ROCm llvm tools not found")
    lib = shutil.copy(LIB, tmp_path)
    subprocess.run([OBJDUMP, "--offloading", lib], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    half = {}
    for f in os.listdir(tmp_path):
        if not f.endswith("gfx950"):
            continue
        text = subprocess.run([READELF, "--notes", os.path.join(tmp_path, f)], check=True, capture_output=True, text=True).stdout
        for block in text.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if not name or "mlp_net_kernel" not in name.group(1):
                continue
            v = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                 for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "max_flat_workgroup_size")
                 if re.search(r"\.%s:\s+(\d+)" % k, block)}
            v["agpr_count"] = int(block.split()[0])
            if v["max_flat_workgroup_size"] == 256:
                half[name.group(1)] = v
    assert half, "no 256-thread mlp_net_kernel instance in the code objects"
    # mlp_net_kernel<NW = 4, A = 5, BH = 8, B3, GO = 4>
    assert any(re.search(r"mlp_net_kernelILi4ELi5ELi8ELi[24]ELi4EE", k) for k in half), sorted(half)
    for k, v in half.items():
        assert v["vgpr_count"] <= 240 and v["agpr_count"] == 0, (k, v)
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (k, v)
