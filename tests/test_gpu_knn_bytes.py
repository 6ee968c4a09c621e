"""gbnns_exact_knn_bytes on the device: ids and distance bit patterns of EVERY query of every case against the oracle over the widened
arrays (the reference's float arithmetic restated) and against gbnns_exact_knn over the widened arrays.  The distances come from
v_mfma_i32_32x32x32_i8 alone -- nothing is rescored -- so a wrong operand lane map, a wrong signed shift, a padded column that is not a
signed zero, a `<` where the threshold needs `<=`, or a key lost or offered twice in a chunk that is swept again shows as a wrong id or a
wrong bit here.  The data is asymmetric (uniform random bytes, values >= 128 everywhere), so a transposed or permuted operand cannot
cancel out."""
import numpy as np
import pytest

import knn_bytes_util as ku

pytestmark = pytest.mark.gpu

N_MAX, NQ_MAX, K_MAX = 6000, 300, 200
NS, NQS, KS = (5, 1037, 6000), (1, 70, 300), (1, 10, 63, 64, 200)   # n below one row block; n_q off a multiple of 32; k > n padding; both sides of the pool switch


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _same(got, want, what):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.nonzero((np.asarray(gi, np.uint32) != wi).any(1) | (ku.bits(gd) != ku.bits(wd)).any(1))[0]
    assert bad.size == 0, (what, "queries that differ:", bad[:8], gi[bad[0]][:8], wi[bad[0]][:8], gd[bad[0]][:8], wd[bad[0]][:8])


_REF = {}


def _shape_case(orc, metric, d):
    """Base, queries and the oracle's K_MAX-lists for every (n, n_q) of the shape test -- computed once per (metric, d), never changed.
    Queries 0 / 1 are all 255 / all 0, base rows 0 / 1 all 0 / all 255: the largest distance the dimension allows."""
    key = (metric, d)
    if key not in _REF:
        base, q = ku.random_bytes(100 + d + metric, N_MAX, d), ku.random_bytes(200 + d + metric, NQ_MAX, d)
        q[0], q[1] = 255, 0
        ref = {n: orc.exact_knn(ku.widen(base[:n]), ku.widen(q), K_MAX, metric, threads=8) for n in NS}
        for a in (base, q):
            a.setflags(write=False)
        _REF[key] = (base, q, ref)
    return _REF[key]


@pytest.mark.parametrize("metric,d", [(ku.L2, d) for d in (4, 30, 64, 100, 128, 192, 256)] + [(ku.NEG_DOT, d) for d in (8, 128, 256)])
def test_shapes(g, orc, metric, d):
    """L2 at d = 4 .. 256 (the ignored d % 4 tail, partial K steps, the 2^24 edge), the negative dot at d = 8 / 128 / 256; n = 5 / 1 037 /
    6 000 rows against 1 / 70 / 300 queries; k = 1 / 10 / 63 / 64 / 200.  knn_chunk at its smallest: 1 037 rows are five chunks and more."""
    base, q, ref = _shape_case(orc, metric, d)
    with ku.knobs(g, knn_chunk=64):
        for n in NS:
            oi, od = ref[n]
            fi, fd = g.exact_knn(ku.widen(base[:n]), ku.widen(q), K_MAX, metric=metric, want_dist=True)
            _same((fi, fd), (oi, od), ("float call vs oracle", n))
            assert n < 1037 or len(ku.chunk_plan(g.knn_bytes_plan(n, NQ_MAX, d, 10), n)) >= 5   # (at k = 10; the longest lists: two chunks)
            for nq in NQS:
                for k in KS:
                    got = g.exact_knn(base[:n], q[:nq], k, metric=metric, want_dist=True)
                    assert got[0].dtype == np.uint32 and got[1].dtype == np.float32
                    _same(got, (oi[:nq, :k], od[:nq, :k]), ("oracle", metric, d, n, nq, k))
                    _same(got, (fi[:nq, :k], fd[:nq, :k]), ("float call", metric, d, n, nq, k))
                    if n < k:
                        assert (got[0][:, n:] == ku.NONE_ID).all() and np.isposinf(got[1][:, n:]).all()
    if d == 256 and metric == ku.L2:   # the edge itself is among the lists compared: all 255 against all 0, 16 646 400 of 2^24 = 16 777 216
        assert ref[5][0][0][4] == 0 and ref[5][1][0][4] == np.float32(255 * 255 * 256)


@pytest.mark.parametrize("pool", (False, True))
@pytest.mark.parametrize("metric", (ku.L2, ku.NEG_DOT))
def test_ties(g, orc, metric, pool):
    """Bytes in {0, 1, 2}, every row three times, k = 40, with and without self_offset = 0: every rank is a mass of equal distances, so the
    `<=` at the threshold and the order of the ids are visible.  On heaps (k below the pool switch) and, the switch lowered, on pools."""
    d, k = 16, 40
    rows = np.random.default_rng(7).integers(0, 3, (340, d), dtype=np.uint8)
    base = np.ascontiguousarray(np.repeat(rows, 3, axis=0)[np.random.default_rng(8).permutation(1020)])
    q = base[:200].copy()
    with ku.knobs(g, knn_chunk=64, knn_pool_min_k=1 if pool else 64):
        assert g.knn_bytes_plan(1020, 200, d, k)["pool"] == pool
        for so in (-1, 0):
            want = orc.exact_knn(ku.widen(base), ku.widen(q), k, metric, self_offset=so, threads=8)
            assert (np.diff(want[1], axis=1) == 0).mean() > 0.5   # (the precondition: most neighbouring ranks tie)
            _same(ku.int_knn(base, q, k, metric, self_offset=so), want, ("integer yardstick", so))
            _same(g.exact_knn(base, q, k, metric=metric, self_offset=so, want_dist=True), want, ("oracle", metric, pool, so))
            _same(g.exact_knn(base, q, k, metric=metric, self_offset=so, want_dist=True),
                  g.exact_knn(ku.widen(base), ku.widen(q), k, metric=metric, self_offset=so, want_dist=True), ("float call", metric, pool, so))


@pytest.mark.parametrize("k", (30, 100))
def test_overflowing_chunks_are_swept_again(g, orc, k):
    """Rows sorted farthest first from tightly clustered queries: every row of every chunk beats the thresholds, so every chunk longer than
    a key list overflows it and is swept again in pieces -- nothing lost, nothing offered twice.  k = 30 on heaps, k = 100 on pools."""
    d, n, nq = 32, 12000, 40
    rng = np.random.default_rng(k)
    centre = np.full(d, 128, np.uint8)
    base = rng.integers(0, 256, (n, d), dtype=np.uint8)
    dist = ((base.astype(np.int64) - 128) ** 2).sum(1)
    base = np.ascontiguousarray(base[np.lexsort((np.arange(n), -dist))])
    q = np.tile(centre, (nq, 1))
    q[1:, 0] += rng.integers(0, 2, nq - 1).astype(np.uint8)   # query 0 is the centre itself: for it the order is farthest first for certain
    with ku.knobs(g, knn_chunk=512):
        plan = g.knn_bytes_plan(n, nq, d, k)
        assert plan["max_chunk"] >= 4 * plan["cap"] and plan["pool"] == (k >= 64)
        chunks = ku.chunk_plan(plan, n)
        assert sum(rows > plan["cap"] for _, rows in chunks) >= 4 and max(rows for _, rows in chunks) == plan["max_chunk"]
        d0 = ((base.astype(np.int64) - 128) ** 2).sum(1)
        assert (np.diff(d0) <= 0).all()   # every row is at least as near to query 0 as all rows before it: it is kept, whatever the threshold
        want = orc.exact_knn(ku.widen(base), ku.widen(q), k, ku.L2, threads=8)
        _same(g.exact_knn(base, q, k, want_dist=True), want, ("oracle", k))
        _same(g.exact_knn(base, q, k, want_dist=True), g.exact_knn(ku.widen(base), ku.widen(q), k, want_dist=True), ("float call", k))


def test_query_slices_with_self_offset(g, orc):
    """A set over itself in two query slices (self_offset 0 and 3 000) equals the oracle's one call."""
    base = ku.random_bytes(31, 6000, 64)
    want = orc.exact_knn(ku.widen(base), ku.widen(base), 10, ku.L2, self_offset=0, threads=8)
    a = g.exact_knn(base, base[:3000].copy(), 10, self_offset=0, want_dist=True)
    b = g.exact_knn(base, base[3000:].copy(), 10, self_offset=3000, want_dist=True)
    _same((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), want, "slices")
    assert not (want[0] == np.arange(6000)[:, None]).any()


@pytest.mark.parametrize("metric,k", [(ku.L2, 10), (ku.L2, 100), (ku.NEG_DOT, 10)])
def test_memory_kinds_agree(g, orc, metric, k):
    """GBNNS_MEM_HOST (numpy) and GBNNS_MEM_DEVICE (torch uint8 tensors on the device) give the same lists."""
    import torch
    base, q = ku.random_bytes(41, 3000, 128), ku.random_bytes(42, 130, 128)
    want = orc.exact_knn(ku.widen(base), ku.widen(q), k, metric, threads=8)
    _same(g.exact_knn(base, q, k, metric=metric, want_dist=True), want, "host")
    ti, td = g.exact_knn(torch.from_numpy(base).cuda(), torch.from_numpy(q).cuda(), k, metric=metric, want_dist=True)
    assert ti.is_cuda and td.is_cuda and ti.dtype == torch.int32 and td.dtype == torch.float32
    _same((ti.cpu().numpy().view(np.uint32), td.cpu().numpy()), want, "device")
    with pytest.raises(TypeError):
        g.exact_knn(torch.from_numpy(base).cuda(), torch.from_numpy(ku.widen(q)).cuda(), k)


def test_scale_against_the_float_call(g):
    """A size nearer use, default knobs: 200 000 x 128 bytes, 4 096 of its own rows as queries, k = 10, self_offset = 0, against
    gbnns_exact_knn on the widened copy (which takes its matrix-core filter at this size)."""
    base = ku.random_bytes(51, 200000, 128)
    q = base[:4096].copy()
    got = g.exact_knn(base, q, 10, self_offset=0, want_dist=True)
    wide = ku.widen(base)
    want = g.exact_knn(wide, wide[:4096].copy(), 10, self_offset=0, want_dist=True)
    _same(got, want, "float call")
    assert not (got[0] == np.arange(4096)[:, None]).any() and (got[0] != ku.NONE_ID).all()
