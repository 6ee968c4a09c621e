"""Byte queries on a byte handle (gbnns_search_byte_queries, Index.search(queries=<uint8>)) without a device: the exactness argument of the
integer first pass on every fixture, that the fixtures of tests/test_gpu_byte_query.py tell wrong distances apart, gbnns_debug_byte_query_plan,
the hand-over precondition, the exports and what argument validation alone refuses.

Measured on the fixtures here: at every beam the three wrong distances change the candidate lists of 96 / 88 (bytes read as int8), 96 / 88
(partner's chunks; 96 on the ties fixture) and 96 / 92 (row term left out) of the 96 queries of the random / extremes fixture; the oracle's
dist_calc on the random fixture is above 128 for every query at ef 64 and ef 200 on either graph.
"""
import ctypes as C

import numpy as np
import pytest

import byte_query_util as bq
import byte_walk_util as bw


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def _oracle_bits(orc, wide, queries):
    """[nq x n] uint32: the oracle's L2 bit pattern of every (query, row) pair (its exact kNN with k = n lists them all)."""
    ids, dists = orc.exact_knn(wide, queries, len(wide), threads=8)
    out = np.empty(dists.shape, np.uint32)
    np.put_along_axis(out, ids.astype(np.int64), np.ascontiguousarray(dists, np.float32).view(np.uint32), axis=1)
    return out


# ---- 1. the integer distance has the oracle's bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bq.FIXTURES)
def test_integer_distance_has_the_oracles_bits(orc, name):
    """sum q^2 + sum x^2 - 2 sum q x in uint32, converted to float32, for every (query, row) pair of the fixture; the fixture itself is what its
    description says (markers, extremes, a quarter of all coordinates >= 128 on both sides)."""
    c = bq.fixture(name)
    assert c["base"].dtype == np.uint8 and c["queries_u8"].dtype == np.uint8 and c["base"].shape == (bq.N, 128) and c["queries_u8"].shape == (bq.NQ, 128)
    assert np.array_equal(c["queries"], c["queries_u8"].astype(np.float32)) and np.array_equal(c["wide"], c["base"].astype(np.float32))
    assert (c["base"] >= 128).mean() >= 0.25 and ((c["queries_u8"] >= 128).mean() >= 0.25 or name == "ties")
    want = _oracle_bits(orc, c["wide"], c["queries"])
    assert want[0, 7] == np.float32(orc.l2(c["wide"][7], c["queries"][0])).view(np.uint32)
    for qi in range(bq.NQ):
        assert np.array_equal(bq.int_l2_bits(c["base"], c["queries_u8"][qi]), want[qi]), (name, qi)
    if name != "ties":
        assert all((c["queries_u8"] == m).any() and (c["base"] == m).any() for m in bq.MARKS)
    if name == "extremes":
        assert (c["base"][list(bq.EXTREME_255)] == 255).all() and (c["base"][list(bq.EXTREME_0)] == 0).all()
        assert (c["queries_u8"][:4] == 0).all() and (c["queries_u8"][4:8] == 255).all() and (c["queries_u8"][8:12] == 0).all() and (c["queries_u8"][12:16] == 255).all()
        far = np.float32(bq.FAR).view(np.uint32)
        assert bq.FAR == 8323200 and want[0, bq.EXTREME_255[0]] == far and want[4, bq.EXTREME_0[0]] == far and want[0, bq.EXTREME_0[0]] == 0
        # ... and it comes out: the lists of queries 0 .. 7 hold it, at every beam, next to the zero distance
        for graph in (1, 2):
            w = bq.expected(orc, name, graph, 200, 200)
            for qi in range(8):
                d = np.ascontiguousarray(w["dists"][qi, :w["count"][qi]], np.float32)
                assert w["count"][qi] == 8 and sorted(set(d.tolist())) == [0.0, float(bq.FAR)], (graph, qi)


def test_integer_distance_at_d256():
    """The largest case the argument covers: d = 256, all 255 against all 0 -- 256 * 255^2 = 16 646 400 < 2^24, exact in float32."""
    x, q = np.full((1, 256), 255, np.uint8), np.zeros(256, np.uint8)
    assert 256 * 255 * 255 == 16646400 < 1 << 24
    for a, b in ((x, q), (q[None, :], x[0])):
        bits = bq.int_l2_bits(a, b)
        assert bits[0] == np.float32(16646400.0).view(np.uint32) and float(bits.view(np.float32)[0]) == 16646400.0
    # ... and float32 sums of the squares agree in any order (here: forwards, backwards, pairwise)
    e = ((x[0].astype(np.float32) - q.astype(np.float32)) ** 2).astype(np.float32)
    fwd = np.float32(0)
    for v in e:
        fwd = np.float32(fwd + v)
    bwd = np.float32(0)
    for v in e[::-1]:
        bwd = np.float32(bwd + v)
    assert fwd == bwd == np.float32(e.reshape(2, 128).sum(axis=0, dtype=np.float32).sum(dtype=np.float32)) == np.float32(16646400.0)


# ---- 2. the fixtures discriminate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["int8", "partner", "no_row"])
def test_wrong_distances_change_the_lists(orc, variant):
    """Bytes read as int8, a lane consuming its partner's chunks of the row, the row term left out: on the random and on the extremes fixture
    each changes the candidate list of at least one query (measured: of nearly all) at every beam.  On the ties fixture every row of a group
    is a permutation of one multiset of bytes against a constant query: a distance that is symmetric in the coordinates -- int8, the row term
    left out -- ties them all again, by construction, and the id decides as before; there the swapped chunks with their weights must show."""
    for name in ("random", "extremes") + (("ties",) if variant == "partner" else ()):
        for ef in bq.BEAMS:
            want = bq.expected(orc, name, 1, ef, ef)["ids"]
            got = bq.wrong_walk(orc, variant, name, 1, ef)
            changed = int((want != got).any(axis=1).sum())
            print("wrong distance", variant, name, "ef", ef, "changes", changed, "of", bq.NQ, "lists")
            assert changed >= 1, (variant, name, ef)


def test_ties_fixture_ties(orc):
    """Every row of a group has one and the same distance from the group's query, an integer: the id decides every comparison."""
    c = bq.fixture("ties")
    bits = _oracle_bits(orc, c["wide"], c["queries"])
    t = bw.contest(0, 128, True)
    per = bq.N // (int(t["qg"].max()) + 1)
    for qi in range(bq.NQ):
        grp = int(t["qg"][qi])
        assert len(np.unique(bits[qi, grp * per:(grp + 1) * per])) == 1, qi


# ---- 3. plans ------------------------------------------------------------------------------------------------------------------------------
INSIDE = [(8, 32), (64, 32), (100, 32), (128, 32), (200, 32), (1024, 32), (64, 48), (64, 64), (100, 48), (100, 64), (200, 48), (1024, 64)]


@pytest.mark.parametrize("ef,stride", INSIDE)
def test_plan_inside_the_domain(g, ef, stride):
    """The integer instance exactly where byte_walk_plan names a byte-walk instance, with its R / ONE_CHUNK / ONE_PASS."""
    walk = g.byte_walk_plan(0, 128, bq.N, stride, ef)
    want = walk.replace("walk_reg_big_bytes_kernel", "beam_u8_big_kernel").replace("walk_reg_bytes_kernel", "beam_u8_kernel")
    assert walk.startswith("walk_reg_") and want.startswith("beam_u8_") and want != walk
    assert g.byte_query_plan(0, 128, bq.N, stride, ef) == want
    assert not any(s in want for s in ("walk_", "rerank_", "knn_scan", "gd_prune"))  # (the ISA contract's name filter does not apply to it)


@pytest.mark.parametrize("what,kw", [
    ("dim 48", dict(dim=48)), ("dim 100", dict(dim=100)), ("dim 96", dict(dim=96)), ("dim 256", dict(dim=256)), ("negative dot", dict(metric=1)),
    ("negative dot d 45", dict(metric=1, dim=45)), ("three entry points", dict(n_entries=3)), ("auxiliary graph", dict(aux_stride=16)),
    ("force_wide", dict(wide=True)), ("tagged", dict(tagged=True)), ("ef 1 025", dict(ef=1025)), ("n = 2^24", dict(n=1 << 24))],
    ids=lambda v: v if isinstance(v, str) else None)
def test_plan_outside_the_domain(g, what, kw):
    for ef in (64, 100, 200):
        a = dict(metric=0, dim=128, n=bq.N, ell_stride=32, ef=ef)
        a.update(kw)
        args = (a.pop("metric"), a.pop("dim"), a.pop("n"), a.pop("ell_stride"), a.pop("ef"))
        assert g.byte_query_plan(*args, **a) == "walk_general_kernel" == g.byte_walk_plan(*args, **a), (what, ef)


def test_plan_refuses_what_is_no_index(g):
    for bad in ((0, 128, bq.N, 33, 64), (2, 128, bq.N, 32, 64), (0, 0, bq.N, 32, 64), (0, 128, bq.N, 32, 0)):
        with pytest.raises(g.GbnnsError) as e:
            g.byte_query_plan(*bad)
        assert e.value.code == 1, bad


def test_other_plans_are_unchanged(g):
    """byte_walk_plan and gbnns_debug_walk_plan on a sample of shapes: the literals of tests/test_byte_walk_cpu.py, from before this change."""
    import test_byte_walk_cpu as t
    for ef, stride, want in [(8, 32, "walk_reg_bytes_kernel<1, true>"), (100, 32, "walk_reg_bytes_kernel<2, true>"), (200, 32, "walk_reg_big_bytes_kernel<true>"),
                             (64, 48, "walk_reg_bytes_kernel<1, false>"), (100, 64, "walk_reg_bytes_kernel<2, false>"), (1024, 64, "walk_reg_big_bytes_kernel<false>")]:
        assert g.byte_walk_plan(0, 128, bq.N, stride, ef) == want
    for args, walk, byte in t.PARENT_PLANS:
        metric, dim, n, stride, ef, n_entries, wide, pas = args
        assert t._walk_plan(g, metric, dim, n, stride, ef, n_entries, wide, pas) == walk
        if byte is not None:
            assert g.byte_plan(metric, dim, n, stride, ef, n_entries=n_entries, wide=bool(wide)) == byte
    # the byte-walk instance's LDS is what it was; the integer twin's is the query area (128 floats) less
    def lds(fn, ef):
        name, n = C.create_string_buffer(128), C.c_uint64(0)
        assert fn(0, 128, bq.N, 32, 0, ef, 1, 0, 0, name, 128, C.byref(n)) == 0
        return n.value
    lib = g.load_library()
    for ef, want in ((64, 1168), (100, 1680), (200, 3216)):
        assert lds(lib.gbnns_debug_byte_walk_plan, ef) == want and lds(lib.gbnns_debug_byte_query_plan, ef) == want - 512


# ---- 4. the hand-over precondition ---------------------------------------------------------------------------------------------------------
def test_hand_over_precondition(orc):
    """A visited set of 128 entries: on the random fixture the oracle's dist_calc exceeds 128 for at least three quarters of the queries at
    ef 64 and ef 200, on either graph -- `general_queries` of the GPU test is a condition, not an observation."""
    for graph in (1, 2):
        for ef in (64, 200):
            w = bq.expected(orc, "random", graph, ef, ef)
            over = int((w["dist_calc"] > 128).sum())
            print("random fixture graph", graph, "ef", ef, "dist_calc > 128 for", over, "of", bq.NQ)
            assert over * 4 >= 3 * bq.NQ, (graph, ef, over)


# ---- 5. exports and what needs no device ---------------------------------------------------------------------------------------------------
def test_exports(g):
    from gbnns_dim_red_amd import binding
    lib = g.load_library()
    for name in ("gbnns_search_byte_queries", "gbnns_debug_byte_query_plan"):
        assert name in binding.SYMBOLS and hasattr(lib, name), name
    assert callable(g.byte_query_plan) and callable(binding.byte_query_plan)


def test_refusals_that_need_no_device(g):
    """Argument validation alone: a null index or null args, and a non-NULL args->queries (refused before the handle is looked at) give
    GBNNS_ERR_INVALID with a message; Index.search refuses uint8 queries on a float handle with TypeError before any call into the library."""
    from gbnns_dim_red_amd import binding
    lib = g.load_library()
    q8 = np.zeros((2, 128), np.uint8)
    qf = np.zeros((2, 128), np.float32)
    ids = np.zeros(2, np.uint32)
    a = binding._SearchArgs(struct_size=C.sizeof(binding._SearchArgs), mode=g.MODE_PLAIN, ef=8, k=1, mem_kind=binding.MEM_HOST, n_q=2,
                            out_ids=ids.ctypes.data, flags=g.FLAG_BYTE_WALK)
    assert lib.gbnns_search_byte_queries(None, C.byref(a), q8.ctypes.data, None, 0, None, None) == 1 and lib.gbnns_last_error()
    assert lib.gbnns_search_byte_queries(None, None, q8.ctypes.data, None, 0, None, None) == 1 and lib.gbnns_last_error()
    a.queries = qf.ctypes.data
    assert lib.gbnns_search_byte_queries(None, C.byref(a), q8.ctypes.data, None, 0, None, None) == 1
    assert b"args->queries must be NULL" in lib.gbnns_last_error()

    class FloatHandle:  # (what Index.search looks at before it touches the library)
        is_bytes = False
        d = 128
    with pytest.raises(TypeError):
        binding.Index.search(FloatHandle(), q8, 8, mode=g.MODE_PLAIN, flags=g.FLAG_BYTE_WALK)
    import torch
    with pytest.raises(TypeError):
        binding.Index.search(FloatHandle(), torch.zeros((2, 128), dtype=torch.uint8), 8, mode=g.MODE_PLAIN, flags=g.FLAG_BYTE_WALK)
