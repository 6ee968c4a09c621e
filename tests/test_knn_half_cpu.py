"""gbnns_exact_knn_half without a device: the exports, knn_half_plan over the shapes that take different paths, and the refusals (before
any HIP call, in the order the header gives them)."""
import numpy as np
import pytest

import knn_bytes_util as ku

INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_exports(g):
    from gbnns_dim_red_amd import binding
    lib = g.load_library()
    for name in ("gbnns_exact_knn_half", "gbnns_index_exact_knn_half", "gbnns_debug_knn_half_plan"):
        assert name in binding.SYMBOLS and hasattr(lib, name), name


# (d, k, metric, stride) -> path, packed, the kernel's name; n = 2 085 rows, knobs: knn_filter = 2, pools from k = 64
PLANS = [
    ((32, 1, ku.L2, 0), ("filter", False, "knn_half_sweep_kernel<2, 4, false>")),
    ((96, 10, ku.L2, 0), ("filter", False, "knn_half_sweep_kernel<6, 1, false>")),
    ((104, 10, ku.L2, 0), ("filter", False, "knn_half_sweep_kernel<7, 1, false>")),   # 13 chunks in 7 K steps: the clamped last chunk
    ((128, 100, ku.L2, 0), ("pool", False, "knn_half_sweep_kernel<8, 1, false>")),
    ((100, 10, ku.L2, 0), ("filter", True, "knn_half_sweep_kernel<7, 1, false>")),    # a caller's array, d % 8 == 4: the copy
    ((100, 100, ku.L2, 104), ("pool", False, "knn_half_sweep_kernel<7, 1, false>")),  # the same rows on a handle (d_pad = 104): in place
    ((30, 10, ku.L2, 0), ("scan", False, "knn_scan_kernel<0, 8, 2, false, half>")),
    ((136, 100, ku.L2, 0), ("scan", False, "knn_scan_wide_kernel<0, 16, false, half>")),
    ((32, 10, ku.NEG_DOT, 0), ("scan", False, "knn_scan_kernel<1, 8, 2, false, half>")),
    ((128, 600, ku.L2, 0), ("scan", False, "knn_scan_kernel<0, 32, 1, false, half>")),  # n <= 4 k
]


@pytest.mark.parametrize("shape,want", PLANS)
def test_plan(g, shape, want):
    d, k, metric, stride = shape
    with ku.knobs(g, knn_filter=2, knn_pool_min_k=64):
        p = g.knn_half_plan(2085, 130, d, k, metric, stride)
        assert (p["path"], p["packed"], p["kernel"]) == want
        assert g.knn_half_plan(2085, 130, d, k, metric, stride, tagged=True)["kernel"] == want[2].replace("false", "true")
    with ku.knobs(g, knn_filter=0):
        assert g.knn_half_plan(2085, 130, d, k, metric, stride)["path"] == "scan"


def test_refusals(g):
    lib = g.load_library()
    b, q, t = np.zeros((8, 16), np.float16), np.zeros((2, 16), np.float32), np.zeros(8, np.uint32)
    ids = np.zeros((2, 1), np.uint32)

    def call(base=b, queries=q, d=16, metric=ku.L2, row_tags=None, query_tags=None, out=ids):
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = lib.gbnns_exact_knn_half(0, ptr(base), 8, ptr(queries), 2, d, 1, metric, -1, ptr(row_tags), ptr(query_tags), ptr(out), None, 0, None)
        return rc, lib.gbnns_last_error().decode()

    assert call(base=None) == (INVALID, "null argument")
    assert call(queries=None) == (INVALID, "null argument")
    assert call(out=None) == (INVALID, "null argument")
    rc, msg = call(d=8200)
    assert rc == UNSUPPORTED and "d <= 8192" in msg
    rc, msg = call(d=12, metric=ku.NEG_DOT)
    assert rc == UNSUPPORTED and "d % 8 == 0" in msg
    for one in (dict(row_tags=t), dict(query_tags=t[:2])):
        rc, msg = call(**one)
        assert rc == INVALID and "both NULL or both set" in msg
    assert lib.gbnns_index_exact_knn_half(None, q.ctypes.data, 2, None, 1, -1, ids.ctypes.data, None, 0, None) == INVALID
    with pytest.raises(TypeError):   # the query is never rounded
        g.exact_knn(b, q.astype(np.float16), 1)
    with pytest.raises(g.GbnnsError) as e:
        g.knn_half_plan(2085, 130, 12, 1, ku.NEG_DOT)
    assert e.value.code == UNSUPPORTED
