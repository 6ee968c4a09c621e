"""The query-slab loop of gbnns_exact_knn_bytes and of gbnns_exact_knn's pool path (graph_api.cpp: `for (q0 = 0; q0 < nq; q0 += slab)`)
with more than one slab, and the lists these calls exist for (k = 1 000 .. 4 096), on the device.  "knn_slab" = 128 makes 300 queries
three slabs of 128, 128 and 44 -- the last short and not a multiple of 32 -- so that everything a later slab does differently from the
first one runs: self_offset + q0, the tag words, queries and outputs at q0, the re-pack of the query operands over the previous slab's,
the reset of keys / pool / root / heap, of the thresholds and of the counts.  The fixtures (tests/knn_slabs_util.py) are built so that
none of these can cancel out, and assert that from the oracle's output before anything runs on the device.  Every comparison is ids AND
distance bit patterns of EVERY query, against the oracle and against the same call in one slab ("knn_slab" = 0)."""
import contextlib

import numpy as np
import pytest

import datagen
import knn_bytes_util as ku
import knn_slabs_util as su
import knn_tagged_util as tu

pytestmark = pytest.mark.gpu

_same = tu.same   # (test_gpu_knn_bytes._same that also takes int32 ids of device results)


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@contextlib.contextmanager
def knobs(g, knn_filter=None, **kw):
    """knn_bytes_util.knobs (knn_chunk, knn_pool_min_k, knn_slab) plus "knn_filter"; defaults restored."""
    lib = g.load_library()
    try:
        if knn_filter is not None:
            assert lib.gbnns_debug_knob(b"knn_filter", knn_filter) == 0
        with ku.knobs(g, **kw):
            yield
    finally:
        lib.gbnns_debug_knob(b"knn_filter", 1)


def _np(r):
    return tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in r)


def _slabbed(g, call, want, nq, k, is_bytes, what, min_slabs=3, **kn):
    """call() in one slab and in slabs of 128 under the knobs kn: both the oracle's `want` (None: the one-slab answer alone), bit for bit.
    From the plan: one slab without the knob; with it at least three, the last partial and not a multiple of 32."""
    with knobs(g, knn_slab=0, **kn):
        assert g.knn_slab(nq, k, bytes=is_bytes) == nq
        one = _np(call())
    with knobs(g, knn_slab=su.SLAB, **kn):
        parts = ku.slabs(g.knn_slab(nq, k, bytes=is_bytes), nq)
        assert len(parts) >= min_slabs and parts[0][1] == su.SLAB and 0 < parts[-1][1] < su.SLAB and parts[-1][1] % 32 != 0, parts
        got = _np(call())
    assert g.knn_slab(nq, k, bytes=is_bytes) == nq   # (the knob is back at 0)
    if want is not None:
        _same(got, want, (what, "slabs against the oracle"))
        _same(one, want, (what, "one slab against the oracle"))
    _same(got, one, (what, "slabs against one slab"))
    return got


_CASES = {}


def _case(orc, kind, metric, d):
    """Base, shuffled queries and tags of a (kind, metric, d) -- made once, never changed -- and the oracle, for _ordered's references."""
    key = (kind, metric, d)
    if key not in _CASES:
        base, q, T, Q, _ = su.byte_case(metric, d, 700 + d + metric) if kind == "bytes" else su.float_case(d, 800 + d)
        for a in (base, q, T, Q):
            a.setflags(write=False)
        _CASES[key] = (base, q, T, Q, {}, orc, metric)
    return _CASES[key]


def _ordered(case, k, tagged, metric=ku.L2):
    """su.ordered on a case: queries by ascending k-th distance and descending threshold (strictly, at stride 128: asserted), the tag words
    moved along and, for a tagged run, checked to differ -- with the rows they allow -- from the word 128 positions earlier.  The oracle's
    K_MAX-lists of the shuffled queries, untagged or over the allowed rows, are computed once per case and kept unchanged."""
    base, q, T, Q, refs, orc, case_metric = case
    assert metric == case_metric
    if tagged not in refs:
        refs[tagged] = tu.expected(orc, base, q, T, Q, su.K_MAX, metric) if tagged else orc.exact_knn(ku.widen(base), ku.widen(q), su.K_MAX, metric, threads=8)
        for a in refs[tagged]:
            a.setflags(write=False)
    qo, Qo, want = su.ordered(q, Q, refs[tagged], k, metric=metric)
    if tagged:
        su.check_tag_offsets(T, Qo)
    return qo, Qo, want


@pytest.mark.parametrize("tagged", (False, True))
@pytest.mark.parametrize("k", (10, 64, 200))
@pytest.mark.parametrize("metric,d", [(ku.L2, 64), (ku.L2, 100), (ku.NEG_DOT, 128)])
def test_byte_slabs(g, orc, metric, d, k, tagged):
    """gbnns_exact_knn_bytes / _tagged over 6 000 rows, chunks of 4 x 64 rows: heaps (k = 10), pools (k = 64, 200)."""
    case = _case(orc, "bytes", metric, d)
    base, T = case[0], case[2]
    assert g.knn_bytes_plan(su.N, su.NQ, d, k)["pool"] == (k >= 64)
    q, Q, want = _ordered(case, k, tagged, metric)
    kw = dict(row_tags=T, query_tags=Q) if tagged else {}
    _slabbed(g, lambda: g.exact_knn(base, q, k, metric=metric, want_dist=True, **kw), want, su.NQ, k, True, (metric, d, k, tagged), knn_chunk=64)


@pytest.mark.parametrize("d", (32, 128))
def test_float_pool_slabs(g, orc, d):
    """gbnns_exact_knn / _tagged on its pool path ("knn_filter" = 2; n > 4 k): k = 64, and k = 7 with "knn_pool_min_k" = 1."""
    case = _case(orc, "float", ku.L2, d)
    base, T = case[0], case[2]
    for k, kn in ((64, {}), (7, dict(knn_pool_min_k=1))):
        for tagged in (False, True):
            q, Q, want = _ordered(case, k, tagged)
            kw = dict(row_tags=T, query_tags=Q) if tagged else {}
            _slabbed(g, lambda: g.exact_knn(base, q, k, want_dist=True, **kw), want, su.NQ, k, False, (d, k, tagged), knn_filter=2, knn_chunk=64, **kn)


@pytest.mark.parametrize("path,k", [("bytes", 10), ("bytes", 64), ("float", 64)])
def test_self_offsets(g, orc, path, k):
    """A set of 340 rows over itself (self_offset 0: slabs of 128, 128 and 84) and queries 1 000 .. 1 299 of 1 400 rows (self_offset 1 000:
    q0 adds to an offset that is not 0), untagged and tagged: no list holds its own row, nor does the oracle's."""
    base, _, T = _case(orc, path, ku.L2, 64 if path == "bytes" else 32)[:3]
    kn = dict(knn_chunk=64) if path == "bytes" else dict(knn_filter=2, knn_chunk=64)
    Q = np.random.default_rng(k).choice(np.array([0x01, 0x02, 0x04, 0x0C, 0x10, 0x20], np.uint32), 340).astype(np.uint32)
    for n, first, nq in ((340, 0, 340), (1400, 1000, 300)):
        b, q = np.ascontiguousarray(base[:n]), np.ascontiguousarray(base[first:first + nq])
        own = np.arange(first, first + nq)[:, None]
        for tagged in (False, True):
            if tagged:
                want = tu.expected(orc, b, q, T[:n], Q[:nq], k, ku.L2, self_offset=first)
                kw = dict(row_tags=np.ascontiguousarray(T[:n]), query_tags=np.ascontiguousarray(Q[:nq]))
            else:
                want = orc.exact_knn(ku.widen(b), ku.widen(q), k, ku.L2, self_offset=first, threads=8)
                kw = {}
            assert not (want[0] == own).any() and (want[0] != ku.NONE_ID).all()
            # (the row itself is at distance 0 and allowed wherever its word allows anything: dropped by the self test alone)
            got = _slabbed(g, lambda: g.exact_knn(b, q, k, self_offset=first, want_dist=True, **kw), want, nq, k, path == "bytes", (path, k, n, tagged), **kn)
            assert not (got[0] == own).any()


@pytest.mark.parametrize("k", (50, 64))
def test_padding_across_slabs(g, orc, k):
    """40 rows against 300 queries, k = 50 (heaps) and 64 (pools): positions 40 and beyond are 0xFFFFFFFF / +inf in EVERY slab -- keys left
    from the slab before would fill them.  Queries by ascending 40th distance."""
    base, q, T, Q = _case(orc, "bytes", ku.L2, 64)[:4]
    b = np.ascontiguousarray(base[:40])
    q, _, want = su.ordered(q, Q, orc.exact_knn(ku.widen(b), ku.widen(q), k, ku.L2, threads=8), k, rank=40)
    assert (want[0][:, :40] != ku.NONE_ID).all() and (want[0][:, 40:] == ku.NONE_ID).all() and np.isposinf(want[1][:, 40:]).all()
    assert g.knn_bytes_plan(40, su.NQ, 64, k)["pool"] == (k >= 64)
    got = _slabbed(g, lambda: g.exact_knn(b, q, k, want_dist=True), want, su.NQ, k, True, ("padding", k))
    assert (got[0][:, 40:] == ku.NONE_ID).all() and np.isposinf(got[1][:, 40:]).all()


@pytest.mark.parametrize("kind", ("bytes", "float"))
def test_device_buffers(g, orc, kind):
    """GBNNS_MEM_DEVICE: torch tensors in, torch tensors out, tagged, k = 64, three slabs."""
    import torch
    d, k = (64, 64) if kind == "bytes" else (32, 64)
    case = _case(orc, kind, ku.L2, d)
    q, Q, want = _ordered(case, k, True)
    tb, tq = torch.from_numpy(case[0].copy()).cuda(), torch.from_numpy(q).cuda()
    tT, tQ = torch.from_numpy(case[2].view(np.int32).copy()).cuda(), torch.from_numpy(Q.view(np.int32).copy()).cuda()
    kn = dict(knn_chunk=64) if kind == "bytes" else dict(knn_filter=2, knn_chunk=64)

    def call():
        ti, td = g.exact_knn(tb, tq, k, want_dist=True, row_tags=tT, query_tags=tQ)
        assert ti.is_cuda and td.is_cuda and ti.dtype == torch.int32 and td.dtype == torch.float32
        return ti, td

    _slabbed(g, call, want, su.NQ, k, kind == "bytes", ("device", kind), **kn)


@pytest.mark.parametrize("kind", ("bytes", "float"))
def test_index_exact_knn(g, orc, kind):
    """Index.exact_knn with 300 queries over the resident table -- a byte handle at d = 100 (rows of 112 bytes), a float handle at d = 32
    with the filter forced on --, untagged and tagged (set_tags), heaps and pools on the byte handle, pools on the float handle."""
    d = 100 if kind == "bytes" else 32
    case = _case(orc, kind, ku.L2, d)
    base, T = case[0], case[2]
    rng = np.random.default_rng(d)
    off, nbr = datagen.random_graph(rng, su.N, 6, 20)
    ix = g.Index(np.ascontiguousarray(base), off, nbr, db_low=datagen.full_mantissa(rng, su.N, 16))
    try:
        assert ix.is_bytes == (kind == "bytes")
        ix.set_tags(T.copy())
        kn = dict(knn_chunk=64) if kind == "bytes" else dict(knn_filter=2, knn_chunk=64)
        for k in ((10, 64) if kind == "bytes" else (64,)):
            for tagged in (False, True):
                q, Q, want = _ordered(case, k, tagged)
                _slabbed(g, lambda: ix.exact_knn(q, k, query_tags=Q if tagged else None, want_dist=True), want, su.NQ, k, kind == "bytes",
                         ("index", kind, k, tagged), **kn)
    finally:
        ix.close()


@pytest.mark.parametrize("tagged", (False, True))
@pytest.mark.parametrize("k,kind", [pytest.param(30, "bytes", id="30"), pytest.param(100, "bytes", id="100"), pytest.param(100, "float", id="float-100")])
def test_overflowing_chunks_are_swept_again_in_every_slab(g, orc, k, kind, tagged):
    """test_gpu_knn_bytes.test_overflowing_chunks_are_swept_again's rows (farthest first) against 300 queries, knn_chunk = 512: chunks that
    overflow a key list are swept again in pieces inside the second and third slab too.  k = 30 on heaps, k = 100 on pools; all rows, and
    half of them allowed.  "float": the same rows widened, on gbnns_exact_knn's pool path ("knn_filter" = 2), whose chunks are a sixteenth
    of the set -- 768 rows of 12 000, 1 280 of the tagged input's 20 000 -- against cap = 464 (tests/test_knn_slabs_cpu.py counts the hits)."""
    if kind == "float":
        base, q, T, Q = su.overflow_case(k, n=su.FLOAT_OVERFLOW_N[tagged])
        n, nq = base.shape[0], q.shape[0]
        plan = su.float_pool_plan(n, k, 512)
        kn = dict(knn_filter=2, knn_chunk=512)
    else:
        base, q, T, Q = su.overflow_case(k)
        n, nq = base.shape[0], q.shape[0]
        kn = dict(knn_chunk=512)
        with knobs(g, **kn):
            plan = g.knn_bytes_plan(n, nq, 32, k)
        assert plan["max_chunk"] >= 4 * plan["cap"] and plan["pool"] == (k >= 64)
    assert sum(rows > plan["cap"] for _, rows in ku.chunk_plan(plan, n)) >= 4
    d0 = ((base.astype(np.int64) - 128) ** 2).sum(1)
    assert (q[0] == 128).all() and (np.diff(d0) <= 0).all()   # (query 0: every row at least as near as all rows before it)
    if kind == "float":
        base, q = ku.widen(base), ku.widen(q)
    if tagged:
        want = tu.expected(orc, base, q, T, Q, k, ku.L2)
        _slabbed(g, lambda: g.exact_knn(base, q, k, want_dist=True, row_tags=T, query_tags=Q), want, nq, k, kind == "bytes", ("overflow, tagged", kind, k), **kn)
    else:
        want = orc.exact_knn(ku.widen(base), ku.widen(q), k, ku.L2, threads=8)
        _slabbed(g, lambda: g.exact_knn(base, q, k, want_dist=True), want, nq, k, kind == "bytes", ("overflow", kind, k), **kn)


# ---- the long lists: k = 1 000 .. 4 096 (one slab unless said otherwise) ----

LONG_KS, LONG_NQ, LONG_ORACLE_NQ = (1000, 2500, 4096), 70, 16
_LONG = {}


def _long_case(g, orc, n, d):
    """Random bytes [n x d], 70 queries, and their 4 096-lists (shorter lists are prefixes): the oracle's for the first 16 queries, the
    float call's on the widened arrays (default knobs: the exact scan) for all -- computed once per shape, never changed."""
    if (n, d) not in _LONG:
        base, q = ku.random_bytes(900 + d, 20000, d)[:n], ku.random_bytes(901 + d, LONG_NQ, d)
        k = LONG_KS[-1]
        oi, od = orc.exact_knn(ku.widen(base), ku.widen(q[:LONG_ORACLE_NQ]), k, ku.L2, threads=8)
        fi, fd = g.exact_knn(ku.widen(base), ku.widen(q), k, want_dist=True)
        _same((fi[:LONG_ORACLE_NQ], fd[:LONG_ORACLE_NQ]), (oi, od), ("float call against the oracle", n, d))
        for a in (base, q, oi, od, fi, fd):
            a.setflags(write=False)
        _LONG[(n, d)] = (np.ascontiguousarray(base), q, (oi, od), (fi, fd))
    return _LONG[(n, d)]


@pytest.mark.parametrize("k", LONG_KS)
@pytest.mark.parametrize("n,d", [(20000, 32), (6000, 128), (4100, 32), (3000, 32)])
def test_byte_long_lists(g, orc, n, d, k):
    """gbnns_exact_knn_bytes at k = 1 000 / 2 500 / 4 096 (pools beyond one selection round, a k that is no power of two, the largest
    lists and key slots it takes) on 20 000 x 32 and 6 000 x 128 bytes; n = 4 100, barely more than 4 096, and n = 3 000 with a padded tail."""
    base, q, (oi, od), (fi, fd) = _long_case(g, orc, n, d)
    plan = g.knn_bytes_plan(n, LONG_NQ, d, k)
    assert plan["pool"] and plan["cap"] == 4 * k + 64 and plan["slab"] == LONG_NQ
    got = g.exact_knn(base, q, k, want_dist=True)
    _same((got[0][:LONG_ORACLE_NQ], got[1][:LONG_ORACLE_NQ]), (oi[:, :k], od[:, :k]), ("oracle", n, d, k))
    _same(got, (fi[:, :k], fd[:, :k]), ("float call", n, d, k))
    if k > n:
        assert (got[0][:, :n] != ku.NONE_ID).all() and (got[0][:, n:] == ku.NONE_ID).all() and np.isposinf(got[1][:, n:]).all()
    else:
        assert (got[0] != ku.NONE_ID).all()


def test_byte_long_lists_overflow_and_slabs(g, orc):
    """k = 1 000 over 20 000 x 32 rows sorted farthest first, knn_chunk = 2 048: chunks longer than cap = 4 064 overflow and are swept
    again; 200 queries at "knn_slab" = 128: slabs of 128 and 72 with pools of 1 000."""
    k, nq = 1000, 200
    base, q, _, _ = su.overflow_case(k, nq=nq, n=20000)
    with knobs(g, knn_chunk=2048):
        plan = g.knn_bytes_plan(20000, nq, 32, k)
        assert plan["pool"] and plan["cap"] == 4064 and sum(rows > plan["cap"] for _, rows in ku.chunk_plan(plan, 20000)) >= 1
    want = orc.exact_knn(ku.widen(base), ku.widen(q), k, ku.L2, threads=8)
    _slabbed(g, lambda: g.exact_knn(base, q, k, want_dist=True), want, nq, k, True, "k = 1000, overflow, slabs", min_slabs=2, knn_chunk=2048)


def test_byte_long_lists_tagged(g, orc):
    """k = 1 000 with one row in eight allowed (2 500 of 20 000): the oracle over the allowed rows for 16 queries, the float tagged call
    on the widened arrays for all 70."""
    k = 1000
    base, q, _, _ = _long_case(g, orc, 20000, 32)
    T, Q = tu.tag_table(77, 20000), np.full(LONG_NQ, 1 << 3, np.uint32)
    assert 2000 < np.count_nonzero(T & Q[0]) < 3000
    got = g.exact_knn(base, q, k, want_dist=True, row_tags=T, query_tags=Q)
    want = tu.expected(orc, base, q[:LONG_ORACLE_NQ], T, Q[:LONG_ORACLE_NQ], k, ku.L2)
    _same((got[0][:LONG_ORACLE_NQ], got[1][:LONG_ORACLE_NQ]), want, "oracle")
    _same(got, g.exact_knn(ku.widen(base), ku.widen(q), k, want_dist=True, row_tags=T, query_tags=Q), "float call")
    assert ((T[got[0]] & Q[0]) != 0).all()


def test_float_pool_longest_lists(g, orc):
    """gbnns_exact_knn's pool path at its largest k, 4 096, on 20 000 x 32 full-mantissa rows: "knn_filter" = 2 against "knn_filter" = 0
    (the exact scan), and the oracle on 16 queries."""
    k = 4096
    rng = np.random.default_rng(4096)
    base, q = datagen.full_mantissa(rng, 20000, 32), datagen.full_mantissa(rng, LONG_NQ, 32)
    with knobs(g, knn_filter=0):
        scan = g.exact_knn(base, q, k, want_dist=True)
    with knobs(g, knn_filter=2):
        pool = g.exact_knn(base, q, k, want_dist=True)
    _same(pool, scan, "pool path against the exact scan")
    want = orc.exact_knn(base, q[:LONG_ORACLE_NQ], k, ku.L2, threads=8)
    _same((pool[0][:LONG_ORACLE_NQ], pool[1][:LONG_ORACLE_NQ]), want, "oracle")
