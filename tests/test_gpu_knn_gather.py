"""gbnns_index_exact_knn_gather on the device: every output byte against the CPU oracle over the allowed rows (tests/knn_tagged_util.py) and
against gbnns_index_exact_knn on the same handle.  Full-mantissa floats make a wrong summation order show; a list handed to the wrong group, a
row id taken from the wrong list entry, a list tail offered beyond its end, a result that depends on the order the fill's atomics gave, or a
round that reads the list buffer of the round before show as a wrong id or a wrong bit.  Nothing here has a tolerance."""
import numpy as np
import pytest

import datagen
import knn_bytes_util as ku
import knn_gather_util as gu
import knn_tagged_util as tu

pytestmark = pytest.mark.gpu

KS = (1, 10, 200)


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


_CASES = {}


def _case(orc, kind, metric, d):
    """Base, queries, words and per n the tags with the oracle's K_MAX-lists -- computed once per (kind, metric, d), never changed."""
    key = (kind, metric, d)
    if key not in _CASES:
        base, q = tu.byte_case(metric, d) if kind == "bytes" else tu.float_case(metric, d)
        Q = gu.query_words(tu.NQ_MAX)
        ref = {}
        for n in tu.NS:
            T = gu.tag_table(n + d, n)
            ref[n] = (T, tu.expected(orc, base[:n], q, T, Q, tu.K_MAX, metric))
            T.setflags(write=False)
        for a in (base, q, Q):
            a.setflags(write=False)
        _CASES[key] = (base, q, Q, ref)
    return _CASES[key]


def _index(g, base, metric, seed=0):
    """A handle the way test_index_exact_knn builds it: a random graph and full-mantissa db_low beside the table."""
    n = base.shape[0]
    rng = np.random.default_rng(1000 + seed + n)
    off, nbr = datagen.random_graph(rng, n, min(6, n - 1), min(20, n - 1))
    return g.Index(np.ascontiguousarray(base), off, nbr, db_low=datagen.full_mantissa(rng, n, 16), metric=metric)


def _bytes_equal(a, b, what):
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), what


SHAPES = [("float", ku.L2, 30), ("float", ku.L2, 128), ("float", ku.NEG_DOT, 8), ("float", ku.NEG_DOT, 128),
          ("bytes", ku.L2, 100), ("bytes", ku.L2, 128), ("bytes", ku.NEG_DOT, 128)]


@pytest.mark.parametrize("kind,metric,d", SHAPES)
def test_shapes(g, orc, kind, metric, d):
    """Every instance family (S = 8 / 32 steps, both metrics, float and byte rows): n below one tile, off a multiple of the tile, many tiles;
    1 / 70 / 300 queries (300 > W at d > 64); k = 1 / 10 / 200.  The 15 words' lists are 0, 7, 40, 64, 128, n and the fractions' lengths."""
    base, q, Q, ref = _case(orc, kind, metric, d)
    assert g.gather_plan(kind == "bytes", metric, d, 10)[0].startswith("knn_gather_kernel<")
    for n in tu.NS:
        T, (ei, ed) = ref[n]
        ix = _index(g, base[:n], metric)
        try:
            ix.set_tags(T.copy())
            for nq in tu.NQS:
                for k in KS:
                    got = ix.exact_knn(q[:nq], k, query_tags=Q[:nq], gather=True, want_dist=True)
                    assert got[0].dtype == np.uint32 and got[1].dtype == np.float32
                    tu.same(got, (ei[:nq, :k], ed[:nq, :k]), ("oracle", kind, metric, d, n, nq, k))
                    _bytes_equal(got, ix.exact_knn(q[:nq], k, query_tags=Q[:nq], want_dist=True), ("ungathered", kind, metric, d, n, nq, k))
        finally:
            ix.close()


@pytest.mark.parametrize("kind", ("float", "bytes"))
def test_fallback(g, orc, kind):
    """d = 192: the plan names the existing scan, and the call returns its bytes (and the oracle's)."""
    d, n, nq, k = 192, 1037, 70, 10
    name, w = g.gather_plan(kind == "bytes", ku.L2, d, k)
    assert w == 0 and name.startswith("knn_bytes_sweep_kernel<" if kind == "bytes" else "knn_scan_wide_kernel<")
    base, q = tu.byte_case(ku.L2, d) if kind == "bytes" else tu.float_case(ku.L2, d)
    base, q, Q, T = base[:n], q[:nq], gu.query_words(nq), gu.tag_table(n + d, n)
    ix = _index(g, base, ku.L2)
    try:
        ix.set_tags(T)
        got = ix.exact_knn(q, k, query_tags=Q, gather=True, want_dist=True)
        _bytes_equal(got, ix.exact_knn(q, k, query_tags=Q, want_dist=True), kind)
        tu.same(got, tu.expected(orc, base, q, T, Q, k, ku.L2), kind)
    finally:
        ix.close()


@pytest.mark.parametrize("kind", ("float", "bytes"))
def test_lane_map(g, orc, kind):
    """32 distinct words, each allowing one row in 32 at a position of its own: a list handed to the wrong group gives wrong ids."""
    d, n, nq = 32, 1037, 70
    base, q = tu.byte_case(ku.L2, d) if kind == "bytes" else tu.float_case(ku.L2, d)
    base, q = base[:n], q[:nq]
    T, Q = tu.lane_map_tags(n, nq)
    ix = _index(g, base, ku.L2)
    try:
        ix.set_tags(T)
        for k in (1, 40):   # 32 or 33 rows allowed: k = 40 pads
            tu.same(ix.exact_knn(q, k, query_tags=Q, gather=True, want_dist=True), tu.expected(orc, base, q, T, Q, k, ku.L2), (kind, k))
    finally:
        ix.close()


def test_ties(g, orc):
    """Every row three times, the lowest id of a triple disallowed: k below and above the number of equal rows, and three calls with
    identical bytes -- the fill's order is free, the result must not depend on it."""
    base, q, T, Q, group = tu.tie_case()
    ix = _index(g, base, ku.L2)
    try:
        ix.set_tags(T)
        for k in (1, 2, 5, 100):
            want = tu.expected_int(base, q, T, Q, k, ku.L2)
            runs = [ix.exact_knn(q, k, query_tags=Q, gather=True, want_dist=True) for _ in range(3)]
            tu.same(runs[0], want, ("ties", k))
            tu.same(runs[0], tu.expected(orc, base, q, T, Q, k, ku.L2), ("ties, oracle", k))
            _bytes_equal(runs[0], runs[1], k)
            _bytes_equal(runs[0], runs[2], k)
            _bytes_equal(runs[0], ix.exact_knn(q, k, query_tags=Q, want_dist=True), ("ungathered", k))
    finally:
        ix.close()


@pytest.mark.parametrize("kind,d", [("float", 30), ("bytes", 100)])
def test_rounds(g, orc, kind, d):
    """gather_budget = n: the schedule tests/test_knn_gather_cpu.py shows to have at least three rounds on this batch -- one list buffer
    filled and scanned round after round -- against the default budget's single round and the oracle.  The knob is restored."""
    n, nq, k = gu.N_ROUNDS, gu.NQ_ROUNDS, 10
    base, q, Q, ref = _case(orc, kind, ku.L2, d)
    T, (ei, ed) = ref[n]
    sched = g.gather_schedule(Q, gu.census(T, Q), n, budget=n, W=g.gather_plan(kind == "bytes", ku.L2, d, k)[1])
    assert sched["rounds"] >= 3
    ix = _index(g, base[:n], ku.L2)
    try:
        ix.set_tags(T.copy())
        default = ix.knob_get("gather_budget")
        assert default == g.binding.GATHER_BUDGET
        one_round = ix.exact_knn(q, k, query_tags=Q, gather=True, want_dist=True)
        try:
            ix.knob("gather_budget", 1)   # never below n: the call runs with n
            ix.knob("gather_timing", 1)
            rounds = ix.exact_knn(q, k, query_tags=Q, gather=True, want_dist=True)
            assert ix.knob_get("gather_rounds") == sched["rounds"]
        finally:
            ix.knob("gather_budget", default)
            ix.knob("gather_timing", 0)
        _bytes_equal(rounds, one_round, kind)
        tu.same(rounds, (ei[:, :k], ed[:, :k]), kind)
        assert ix.knob_get("gather_budget") == default
    finally:
        ix.close()


@pytest.mark.parametrize("kind,d", [("float", 128), ("bytes", 100)])
def test_groups(g, orc, kind, d):
    """One word for 300 queries (more than W: several workgroups on one list), 300 distinct words (every group one query, one thread of a
    workgroup), a batch that may see nothing (padding only), and a single query."""
    n, nq, k = 1037, 300, 10
    base, q, _, ref = _case(orc, kind, ku.L2, d)
    base, T = base[:n], ref[n][0]
    assert g.gather_plan(kind == "bytes", ku.L2, d, k)[1] < nq
    ix = _index(g, base, ku.L2)
    try:
        ix.set_tags(T.copy())
        distinct = (np.arange(nq, dtype=np.uint32) * 8 + 2).astype(np.uint32)   # bit 1 and a varying set of others
        assert np.unique(distinct).size == nq
        for what, Q in (("one word", np.full(nq, 1 << 2, np.uint32)), ("distinct", distinct), ("nothing", np.zeros(nq, np.uint32))):
            got = ix.exact_knn(q, k, query_tags=Q, gather=True, want_dist=True)
            tu.same(got, tu.expected(orc, base, q, T, Q, k, ku.L2), (kind, what))
            if what == "nothing":
                assert (got[0] == tu.NONE_ID).all() and np.isposinf(got[1]).all()
        Q1 = np.array([1 << 3], np.uint32)
        tu.same(ix.exact_knn(q[:1], k, query_tags=Q1, gather=True, want_dist=True), tu.expected(orc, base, q[:1], T, Q1, k, ku.L2), (kind, "nq = 1"))
    finally:
        ix.close()


@pytest.mark.parametrize("kind,d", [("float", 30), ("bytes", 100)])
def test_self_offset(g, orc, kind, d):
    """The queries are rows of the table: self_offset 3 and 0, the query's own row allowed for some queries and disallowed for others."""
    n, nq, k = 1037, 70, 10
    base, _, _, ref = _case(orc, kind, ku.L2, d)
    base, T, Q = base[:n], ref[n][0], gu.query_words(nq)
    for so in (3, 0):
        q = np.ascontiguousarray(base[so:so + nq])
        own = (T[so:so + nq] & Q) != 0
        assert own.any() and (~own).any()
        ix = _index(g, base, ku.L2)
        try:
            ix.set_tags(T.copy())
            got = ix.exact_knn(q, k, query_tags=Q, self_offset=so, gather=True, want_dist=True)
            tu.same(got, tu.expected(orc, base, q, T, Q, k, ku.L2, self_offset=so), (kind, so))
            assert (got[0] != (np.arange(nq) + so)[:, None]).all()
            _bytes_equal(got, ix.exact_knn(q, k, query_tags=Q, self_offset=so, want_dist=True), (kind, so))
        finally:
            ix.close()


@pytest.mark.parametrize("kind,d", [("float", 30), ("bytes", 100)])
def test_nothing_cached_and_memory_kinds(g, orc, kind, d):
    """set_tags, call, a partial set_tags(first=500), call again: each answer is the oracle's on the table of that moment.  Then device queries
    and tags on the current stream: the host call's bytes; a host tag array beside device queries is a TypeError; gather without tags a
    ValueError; and a LOWQ search on the handle returns what it returned before the gathered calls."""
    import torch
    n, nq, k = 1037, 70, 10
    base, q, Q, ref = _case(orc, kind, ku.L2, d)
    base, q, Q = base[:n], np.ascontiguousarray(q[:nq]), np.ascontiguousarray(Q[:nq])
    ix = _index(g, base, ku.L2)
    try:
        q_low = datagen.full_mantissa(np.random.default_rng(5), nq, 16)
        search = lambda: ix.search(q, 32, mode=g.MODE_LOWQ, queries_low=q_low, want=("hops", "dist_calc", "cand"))
        before = search()
        with pytest.raises(g.GbnnsError) as e:   # no tag table yet
            ix.exact_knn(q, k, query_tags=Q, gather=True)
        assert e.value.code == 1
        with pytest.raises(ValueError):
            ix.exact_knn(q, k, gather=True)
        T = ref[n][0].copy()
        ix.set_tags(T)
        steps = [T.copy()]
        T[500:600] = gu.tag_table(77, 100)
        steps.append(T.copy())
        for step, tags in enumerate(steps):
            if step:
                ix.set_tags(tags[500:600], first=500)
            got = ix.exact_knn(q, k, query_tags=Q, gather=True, want_dist=True)
            tu.same(got, tu.expected(orc, base, q, tags, Q, k, ku.L2), (kind, "step", step))
        host = got
        ti, td = ix.exact_knn(torch.from_numpy(q.copy()).cuda(), k, query_tags=torch.from_numpy(Q.view(np.int32).copy()).cuda(), gather=True, want_dist=True)
        torch.cuda.synchronize()
        _bytes_equal((ti.cpu().numpy(), td.cpu().numpy()), host, (kind, "device"))
        with pytest.raises(TypeError):
            ix.exact_knn(torch.from_numpy(q.copy()).cuda(), k, query_tags=Q, gather=True)
        after = search()
        for name in ("ids", "hops", "dist_calc", "cand"):
            assert np.array_equal(before[name], after[name]), name
    finally:
        ix.close()


@pytest.mark.parametrize("kind,d", [("float", 30), ("bytes", 100)])
def test_routed(g, orc, kind, d):
    """search_auto with FLAG_SCAN_GATHER against the same call without it, at scan_below = 0 (only the queries that may see nothing scan), a
    value that splits the batch, and 2^64 - 1 (every query scans): every entry of the dict identical, route and allowed included; the same
    with FLAG_TAG_BRIDGE beside it.  Outside search_auto the flag is refused like FLAG_TAG_BRIDGE outside the tagged calls."""
    n, nq, k, ef = 1037, 70, 10, 32
    base, q, Q, ref = _case(orc, kind, ku.L2, d)
    base, q, Q, T = base[:n], np.ascontiguousarray(q[:nq]), np.ascontiguousarray(Q[:nq]), ref[n][0]
    ix = _index(g, base, ku.L2)
    try:
        ix.set_tags(T.copy())
        q_low = datagen.full_mantissa(np.random.default_rng(6), nq, 16)
        allowed = gu.census(T, Q)
        split = int(np.median(allowed))
        assert 0 < np.count_nonzero(allowed <= split) < nq
        want = ("hops", "dist_calc", "cand", "cand_dist")
        for bridge in (0, g.FLAG_TAG_BRIDGE):
            for below in (0, split, 2 ** 64 - 1):
                plain = ix.search_auto(q, ef, k, Q, scan_below=below, mode=g.MODE_LOWQ, queries_low=q_low, want=want, flags=bridge)
                gathered = ix.search_auto(q, ef, k, Q, scan_below=below, mode=g.MODE_LOWQ, queries_low=q_low, want=want, flags=bridge | g.FLAG_SCAN_GATHER)
                assert set(plain) == set(gathered) and {"top_ids", "top_dist", "route", "allowed"} <= set(plain)
                for name in plain:
                    assert plain[name].tobytes() == gathered[name].tobytes(), (kind, bridge, below, name)
                assert np.array_equal(plain["route"], (allowed <= below).astype(np.uint8)) and np.array_equal(plain["allowed"], allowed)
                scan = plain["route"] == 1
                ei, ed = tu.expected(orc, base, q, T, Q, k, ku.L2)
                tu.same((gathered["top_ids"][scan], gathered["top_dist"][scan]), (ei[scan], ed[scan]), (kind, bridge, below))
        for call in (lambda: ix.search(q, ef, mode=g.MODE_LOWQ, queries_low=q_low, flags=g.FLAG_SCAN_GATHER),
                     lambda: ix.search(q, ef, mode=g.MODE_LOWQ, queries_low=q_low, flags=g.FLAG_SCAN_GATHER, query_tags=Q, top_k=k)):
            with pytest.raises(g.GbnnsError) as e:
                call()
            assert e.value.code == 1 and "GBNNS_FLAG_SCAN_GATHER" in str(e.value)
    finally:
        ix.close()
