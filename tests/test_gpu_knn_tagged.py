"""gbnns_exact_knn_tagged / gbnns_exact_knn_bytes_tagged / gbnns_index_exact_knn on the device: ids and distance bit patterns of EVERY
query of every case against the CPU oracle over the allowed rows (tests/knn_tagged_util.py), the byte form against the float form on the
widened arrays, the handle form against the free functions.  A tag test on the wrong row of a tile, a disallowed pair that still takes a
slot of a key list, a threshold taken from a list that holds disallowed rows, tag words read at the wrong stride or from the wrong chunk
show as a wrong id or a wrong bit here."""
import contextlib

import numpy as np
import pytest

import datagen
import knn_bytes_util as ku
import knn_tagged_util as tu

pytestmark = pytest.mark.gpu

KS_SCAN, KS_LISTS = (1, 10, 200), (10, 64, 200)


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@contextlib.contextmanager
def knobs(g, knn_filter=None, **kw):
    """knn_bytes_util.knobs plus "knn_filter" (2: the matrix-core filter of the float call whenever the shape allows); defaults restored."""
    lib = g.load_library()
    try:
        if knn_filter is not None:
            assert lib.gbnns_debug_knob(b"knn_filter", knn_filter) == 0
        with ku.knobs(g, **kw):
            yield
    finally:
        lib.gbnns_debug_knob(b"knn_filter", 1)


_CASES = {}


def _case(orc, kind, metric, d):
    """Base, queries, tags and the oracle's K_MAX-lists for every n of a shape test -- computed once per (kind, metric, d), never changed;
    a case with fewer queries or a shorter list is a prefix of these."""
    key = (kind, metric, d)
    if key not in _CASES:
        base, q = tu.byte_case(metric, d) if kind == "bytes" else tu.float_case(metric, d)
        Q = tu.query_words(tu.NQ_MAX)
        ref = {}
        for n in tu.NS:
            T = tu.tag_table(n + d, n)
            ref[n] = (T, tu.expected(orc, base[:n], q, T, Q, tu.K_MAX, metric))
            T.setflags(write=False)
        for a in (base, q, Q):
            a.setflags(write=False)
        _CASES[key] = (base, q, Q, ref)
    return _CASES[key]


def _sweep_shapes(g, case, metric, ks, also=None):
    base, q, Q, ref = case
    for n in tu.NS:
        T, (ei, ed) = ref[n]
        for nq in tu.NQS:
            for k in ks:
                got = g.exact_knn(base[:n], q[:nq], k, metric=metric, want_dist=True, row_tags=T, query_tags=Q[:nq])
                assert got[0].dtype == np.uint32 and got[1].dtype == np.float32
                tu.same(got, (ei[:nq, :k], ed[:nq, :k]), ("oracle", metric, base.shape[1], n, nq, k))
                if also is not None:
                    fi, fd = also[n]
                    tu.same(got, (fi[:nq, :k], fd[:nq, :k]), ("float call", metric, base.shape[1], n, nq, k))


@pytest.mark.parametrize("metric,d", [(ku.L2, 30), (ku.L2, 128), (ku.L2, 192), (ku.NEG_DOT, 8), (ku.NEG_DOT, 128)])
def test_float_scan(g, orc, metric, d):
    """The exact scan with the tag test beside the self test: knn_scan_kernel at d <= 128, knn_scan_wide_kernel at d = 192; n below one
    tile, off a multiple of the tile, many tiles; 1 / 70 / 300 queries; k = 1 / 10 / 200 (more than bit 9, bit 8 or n = 5 allow)."""
    case = _case(orc, "float", metric, d)
    _sweep_shapes(g, case, metric, KS_SCAN)
    base, q, Q, ref = case
    T = ref[1037][0]
    want = tu.expected(orc, base[:1037], q[:70], T, Q[:70], 10, metric, self_offset=5)   # a set "over itself": row i + 5 dropped, allowed or not
    tu.same(g.exact_knn(base[:1037], q[:70], 10, metric=metric, self_offset=5, want_dist=True, row_tags=T, query_tags=Q[:70]), want, "self_offset")


@pytest.mark.parametrize("d", (32, 128))
def test_float_filter_paths(g, orc, d):
    """The matrix-core filter forced on ("knn_filter" = 2) with chunks of 64 rows: the heap filter at k = 10 (first rows and overflowing
    chunks through the tagged scan, the rest through the tagged knn_filter_kernel), the pool path at k = 64 and 200."""
    case = _case(orc, "float", ku.L2, d)
    with knobs(g, knn_filter=2, knn_chunk=64):
        _sweep_shapes(g, case, ku.L2, KS_LISTS)


@pytest.mark.parametrize("metric,d", [(ku.L2, 4), (ku.L2, 100), (ku.L2, 128), (ku.L2, 256), (ku.NEG_DOT, 128)])
def test_bytes(g, orc, metric, d):
    """knn_bytes_sweep_kernel's tagged instances, heaps (k = 10) and pools (k = 64, 200), chunks of 4 x 64 rows: the oracle's answer, and
    the float tagged call's on the widened arrays."""
    case = _case(orc, "bytes", metric, d)
    base, q, Q, ref = case
    with knobs(g, knn_chunk=64):
        also = {n: g.exact_knn(ku.widen(base[:n]), ku.widen(q), tu.K_MAX, metric=metric, want_dist=True, row_tags=ref[n][0], query_tags=Q) for n in tu.NS}
        _sweep_shapes(g, case, metric, KS_LISTS, also=also)


@pytest.mark.parametrize("path", ("bytes_sweep", "float_filter", "scan", "scan_wide"))
def test_lane_map(g, orc, path):
    """T[j] = 1 << (j % 32), Q[i] = 1 << (i % 32): one allowed row per block of 32, at a position that differs per query, k = 1 and 5."""
    d = {"bytes_sweep": 64, "float_filter": 32, "scan": 32, "scan_wide": 192}[path]
    if path == "bytes_sweep":
        base, q = tu.byte_case(ku.L2, d)
    else:
        base, q = tu.float_case(ku.L2, d)
    with knobs(g, knn_filter=2 if path == "float_filter" else 0, knn_chunk=64):
        for n, nq in ((1037, 70), (6000, 300)):
            T, Q = tu.lane_map_tags(n, nq)
            want = tu.expected(orc, base[:n], q[:nq], T, Q, 5, ku.L2)
            assert ((want[0] % 32) == (np.arange(nq) % 32)[:, None]).all()
            for k in (1, 5):
                got = g.exact_knn(base[:n], q[:nq], k, want_dist=True, row_tags=T, query_tags=Q)
                tu.same(got, (want[0][:, :k], want[1][:, :k]), (path, n, nq, k))


@pytest.mark.parametrize("pool", (False, True))
@pytest.mark.parametrize("metric", (ku.L2, ku.NEG_DOT))
def test_ties(g, orc, metric, pool):
    """test_gpu_knn_bytes.test_ties' data with the lowest id of every triple of equal rows disallowed, with and without self_offset = 0."""
    k = 40
    base, q, T, Q, _ = tu.tie_case()
    with knobs(g, knn_chunk=64, knn_pool_min_k=1 if pool else 64):
        assert g.knn_bytes_plan(1020, 200, 16, k)["pool"] == pool
        for so in (-1, 0):
            want = tu.expected(orc, base, q, T, Q, k, metric, self_offset=so)
            got = g.exact_knn(base, q, k, metric=metric, self_offset=so, want_dist=True, row_tags=T, query_tags=Q)
            tu.same(got, want, ("oracle", metric, pool, so))
            assert (T[got[0]] == 1).all()
            tu.same(g.exact_knn(ku.widen(base), ku.widen(q), k, metric=metric, self_offset=so, want_dist=True, row_tags=T, query_tags=Q), want,
                    ("float call", metric, pool, so))


@pytest.mark.parametrize("k", (30, 100))
def test_overflowing_chunks_are_swept_again(g, orc, k):
    """Rows farthest first, half of them allowed, knn_chunk = 512: chunks whose ALLOWED hits overflow a key list are swept again in pieces."""
    base, q, T, Q = tu.overflow_case(k)
    with knobs(g, knn_chunk=512):
        want = tu.expected(orc, base, q, T, Q, k, ku.L2)
        tu.same(g.exact_knn(base, q, k, want_dist=True, row_tags=T, query_tags=Q), want, ("oracle", k))
    with knobs(g, knn_filter=2, knn_chunk=512):
        tu.same(g.exact_knn(ku.widen(base), ku.widen(q), k, want_dist=True, row_tags=T, query_tags=Q), want, ("float call", k))


def test_all_ones_is_the_untagged_call_and_zero_is_padding(g):
    n, nq = 3000, 130
    ones_t, ones_q = np.full(n, tu.ALL, np.uint32), np.full(nq, tu.ALL, np.uint32)
    bb, bq = tu.byte_case(ku.L2, 128)
    fb, fq = tu.float_case(ku.L2, 128)
    pairs = [(bb[:n], bq[:nq], dict()), (fb[:n], fq[:nq], dict()), (fb[:n], fq[:nq], dict(knn_filter=2, knn_chunk=64))]
    for base, q, kn in pairs:
        with knobs(g, **kn):
            for k, so in ((10, -1), (100, 7)):
                a = g.exact_knn(base, q, k, self_offset=so, want_dist=True)
                b = g.exact_knn(base, q, k, self_offset=so, want_dist=True, row_tags=ones_t, query_tags=ones_q)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (base.dtype, kn, k)
                z = g.exact_knn(base, q, k, self_offset=so, want_dist=True, row_tags=ones_t, query_tags=np.zeros(nq, np.uint32))
                assert (z[0] == tu.NONE_ID).all() and np.isposinf(z[1]).all()


@pytest.mark.parametrize("kind", ("bytes", "float"))
def test_memory_kinds_agree(g, orc, kind):
    import torch
    base, q, Q, ref = _case(orc, kind, ku.L2, 128)
    n, nq = 1037, 70
    T, (ei, ed) = ref[n]
    tT, tQ = torch.from_numpy(T.view(np.int32).copy()).cuda(), torch.from_numpy(Q[:nq].view(np.int32).copy()).cuda()
    tb, tq = torch.from_numpy(base[:n].copy()).cuda(), torch.from_numpy(q[:nq].copy()).cuda()
    for k in (10, 100):
        want = (ei[:nq, :k], ed[:nq, :k])
        tu.same(g.exact_knn(base[:n], q[:nq], k, want_dist=True, row_tags=T, query_tags=Q[:nq]), want, "host")
        ti, td = g.exact_knn(tb, tq, k, want_dist=True, row_tags=tT, query_tags=tQ)
        assert ti.is_cuda and td.is_cuda and ti.dtype == torch.int32 and td.dtype == torch.float32
        tu.same((ti.cpu().numpy(), td.cpu().numpy()), want, "device")
    with pytest.raises(TypeError):
        g.exact_knn(tb, tq, 5, row_tags=T, query_tags=tQ)   # a host tag array beside device inputs


@pytest.mark.parametrize("kind,d", [("float", 128), ("float", 30), ("bytes", 128), ("bytes", 100)])
def test_index_exact_knn(g, orc, kind, d):
    """Index.exact_knn over the resident table (d = 30: float rows of 32 floats; d = 100: byte rows of 112 bytes): tags from set_tags, then a
    partial set_tags(first=...), each answer equal to the free function's on the same arrays and to the oracle's; untagged with
    query_tags=None; device queries; the two refusals; and the handle's searches are what they were."""
    import torch
    n, nq, dlow = 1037, 70, 16
    base, q, Q, ref = _case(orc, kind, ku.L2, d)
    base, q, Q = np.ascontiguousarray(base[:n]), np.ascontiguousarray(q[:nq]), np.ascontiguousarray(Q[:nq])
    rng = np.random.default_rng(d)
    off, nbr = datagen.random_graph(rng, n, 6, 20)
    db_low, q_low = datagen.full_mantissa(rng, n, dlow), datagen.full_mantissa(rng, nq, dlow)
    ix = g.Index(base, off, nbr, db_low=db_low)
    try:
        assert ix.is_bytes == (kind == "bytes")
        search = lambda: ix.search(q, 32, mode=g.MODE_LOWQ, queries_low=q_low, want=("hops", "dist_calc", "cand"))
        before = search()
        with pytest.raises(g.GbnnsError) as e:   # no tag table yet
            ix.exact_knn(q, 5, query_tags=Q)
        assert e.value.code == 1
        for k in (10, 100):   # untagged: needs no tag table
            want = orc.exact_knn(ku.widen(base), ku.widen(q), k, ku.L2, threads=8)
            tu.same(ix.exact_knn(q, k, want_dist=True), want, ("untagged", k))
            assert ix.exact_knn(q, k).tobytes() == g.exact_knn(base, q, k).tobytes()
        T = ref[n][0].copy()
        ix.set_tags(T)
        steps = [T.copy()]
        T[500:600] = tu.tag_table(77, 100)
        steps.append(T.copy())
        for step, tags in enumerate(steps):
            if step:
                ix.set_tags(tags[500:600], first=500)
            for k, so in ((10, -1), (100, 3)):
                want = tu.expected(orc, base, q, tags, Q, k, ku.L2, self_offset=so)
                got = ix.exact_knn(q, k, query_tags=Q, self_offset=so, want_dist=True)
                tu.same(got, want, ("oracle", step, k))
                free = g.exact_knn(base, q, k, self_offset=so, want_dist=True, row_tags=tags, query_tags=Q)
                assert got[0].tobytes() == free[0].tobytes() and got[1].tobytes() == free[1].tobytes(), (step, k)
        # device queries and tags, on the current stream, behind a set_tags enqueued there
        ix.set_tags(torch.from_numpy(steps[0].view(np.int32).copy()).cuda())
        ti, td = ix.exact_knn(torch.from_numpy(q.copy()).cuda(), 10, query_tags=torch.from_numpy(Q.view(np.int32).copy()).cuda(), want_dist=True)
        tu.same((ti.cpu().numpy(), td.cpu().numpy()), tu.expected(orc, base, q, steps[0], Q, 10, ku.L2), "device")
        # the two refusals
        if kind == "float":
            with pytest.raises(TypeError):
                ix.exact_knn(q.astype(np.uint8), 5)
            lib, ids = g.load_library(), np.zeros((nq, 5), np.uint32)
            qb = np.zeros((nq, d), np.uint8)
            assert lib.gbnns_index_exact_knn(ix._h, None, qb.ctypes.data, nq, None, 5, -1, ids.ctypes.data, None, 0, None) == 1
        else:
            with pytest.raises(g.GbnnsError) as e:
                ix.exact_knn(ku.widen(q), 5)
            assert e.value.code == 5 and "mixed-pair" in str(e.value)
        after = search()
        for name in ("ids", "hops", "dist_calc", "cand"):
            assert np.array_equal(before[name], after[name]), name
    finally:
        ix.close()
