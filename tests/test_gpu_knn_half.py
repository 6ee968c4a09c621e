"""gbnns_exact_knn_half on a device: binary16 rows against float32 queries, ids and distance bytes equal to a plain reference -- the
reference's ordered float32 sums on the widened rows, then numpy's sort of (distance, id) (tests/knn_half_util.py).  Not another call of
the library.  (Every kernel instance: tests/test_gpu_knn_half_instances.py; the sweep's edges: tests/test_gpu_knn_half_edges.py.)
n = 2 085 rows (no multiple of 32 or 64) in several chunks, every eighth row a duplicate of the row before it; three magnitude classes,
the queries at the rows' scale: unit, rows x 2^-20 (most halves subnormal: pins that the f16 matrix cores keep subnormal operands, which
the sweep's error bound assumes) and rows x 2^13."""
import functools

import numpy as np
import pytest

import knn_bytes_util as ku
from knn_half_util import F32, SCALE, half_rows, knn_of, ordered_dist, same

pytestmark = pytest.mark.gpu

N, NQ = 2085, 130


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@functools.lru_cache(maxsize=None)
def data(d, cls, n=N):
    rng = np.random.default_rng(1000 * d + SCALE[cls] + n)
    rows = half_rows(rng, n, d, cls)            # (every eighth row a duplicate: ties)
    q = rng.standard_normal((NQ, d)).astype(F32) * F32(2.0 ** SCALE[cls])
    q[:4] = rows[10:14].astype(F32)             # distance 0 to a row and its duplicate's neighbourhood
    return rows, q


@functools.lru_cache(maxsize=None)
def reference(d, cls, metric, n=N):
    rows, q = data(d, cls, n)
    return ordered_dist(rows, q, metric)


def knobs(g):
    return ku.knobs(g, knn_filter=2, knn_chunk=512, knn_pool_min_k=64)


# (metric, d, the sweep takes it, from a copy)
SHAPES = [(ku.L2, 32, True, False), (ku.L2, 96, True, False), (ku.L2, 104, True, False), (ku.L2, 128, True, False), (ku.L2, 100, True, True),
          (ku.L2, 30, False, False), (ku.L2, 136, False, False), (ku.NEG_DOT, 32, False, False)]


@pytest.mark.parametrize("cls", list(SCALE))
@pytest.mark.parametrize("k", (1, 10, 100))
@pytest.mark.parametrize("metric,d,swept,packed", SHAPES)
def test_parity(g, metric, d, swept, packed, k, cls):
    rows, q = data(d, cls)
    with knobs(g):
        p = g.knn_half_plan(N, NQ, d, k, metric)
        assert (p["path"], p["packed"]) == ((("pool" if k >= 64 else "filter") if swept else "scan"), packed), p
        got = g.exact_knn(rows, q, k, metric=metric, want_dist=True)
    same(got, knn_of(reference(d, cls, metric), k), f"d {d} k {k} {cls} {p['kernel']}")


def test_overflow_falls_back_to_the_half_row_scan(g):
    """Rows sorted farthest first: every row of a later chunk (512 rows at this size, lists of 256) is nearer than all rows before it."""
    n, d, k = 8200, 32, 10
    rows, q = data(d, "unit", n)
    q = (q * F32(0.01)).astype(F32)
    rows = rows[np.argsort(-(rows.astype(np.float64) ** 2).sum(1), kind="stable")]
    with knobs(g):
        assert g.knn_half_plan(n, NQ, d, k)["path"] == "filter"
        got = g.exact_knn(rows, q, k, want_dist=True)
    same(got, knn_of(ordered_dist(rows, q, ku.L2), k), "overflow")


@pytest.mark.parametrize("k", (10, 100))
def test_tagged(g, k):
    rows, q = data(96, "unit")
    T = np.where(np.arange(N) % 2 == 0, 1, 2).astype(np.uint32)
    Q = np.array([1, 2, 3], np.uint32)[np.arange(NQ) % 3]
    Q[0] = 0   # may see nothing: padding only
    with knobs(g):
        assert g.knn_half_plan(N, NQ, 96, k, tagged=True)["kernel"].startswith("knn_half_sweep_kernel<6, 1, true>")
        got = g.exact_knn(rows, q, k, want_dist=True, row_tags=T, query_tags=Q)
    assert (got[0][0] == ku.NONE_ID).all() and np.isinf(got[1][0]).all()
    same(got, knn_of(reference(96, "unit", ku.L2), k, allowed=(T[None, :] & Q[:, None]) != 0), "tagged")


def test_self_offset(g):
    rows, _ = data(32, "unit")
    q = rows[5:5 + NQ].astype(F32)
    with knobs(g):
        got = g.exact_knn(rows, q, 10, want_dist=True, self_offset=5)
    same(got, knn_of(ordered_dist(rows, q, ku.L2), 10, self_offset=5), "self_offset")


def test_handle_and_device_tensors(g):
    """Index(db=<float16>).exact_knn(half_scan=True) over the resident table (d = 100: d_pad = 104 halves, swept in place) with and
    without set_tags, HOST and DEVICE buffers, and exact_knn on torch.float16 device tensors (there: the copy) -- all the free call's bytes."""
    import torch
    d, k = 100, 10
    rows, q = data(d, "unit")
    off, nbr = np.arange(N + 1, dtype=np.uint64), ((np.arange(N) + 1) % N).astype(np.uint32)
    T = np.where(np.arange(N) % 2 == 0, 1, 2).astype(np.uint32)
    Q = np.array([1, 2, 3], np.uint32)[np.arange(NQ) % 3]
    dq = torch.from_numpy(q).cuda()
    with knobs(g):
        assert g.knn_half_plan(N, NQ, d, k, stride=104)["packed"] is False
        want = g.exact_knn(rows, q, k, want_dist=True)
        want_t = g.exact_knn(rows, q, k, want_dist=True, row_tags=T, query_tags=Q)
        same(want, knn_of(reference(d, "unit", ku.L2), k), "free call")
        same(g.exact_knn(torch.from_numpy(rows).cuda(), dq, k, want_dist=True), want, "device tensors")
        ix = g.Index(rows, off, nbr, db_low=rows[:, :8].astype(F32))
        assert ix.is_half_base
        same(ix.exact_knn(q, k, want_dist=True, half_scan=True), want, "handle, HOST")
        same(ix.exact_knn(dq, k, want_dist=True, half_scan=True), want, "handle, DEVICE")
        ix.set_tags(T)
        same(ix.exact_knn(q, k, want_dist=True, half_scan=True), want, "handle with a tag table, untagged")
        same(ix.exact_knn(q, k, query_tags=Q, want_dist=True, half_scan=True), want_t, "handle, tagged, HOST")
        same(ix.exact_knn(dq, k, query_tags=torch.from_numpy(Q.view(np.int32)).cuda(), want_dist=True, half_scan=True), want_t, "handle, tagged, DEVICE")
        ix.close()
