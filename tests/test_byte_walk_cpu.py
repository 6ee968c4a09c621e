"""The byte-row PLAIN walk (FLAG_BYTE_WALK) without a device: the exports, gbnns_debug_byte_walk_plan -- which flagged calls get a byte-walk
first pass and which run whole on the general kernel's byte-walk instance --, that the other plan functions answer as before, and the
preconditions that keep tests/test_gpu_byte_walk.py from passing vacuously.

Measured on the fixtures here (oracle, widened table), random bytes d = 128 / 48 / 100: the bit patterns of an evaluation whose lane pairs
never exchange sums differ from the oracle's on 0.468 / 0.326 / 0.406 of the (query, row) pairs; at ef 64 every query of the d = 128 fixture
computes more than 128 distances on either graph.
"""
import ctypes as C

import numpy as np
import pytest

import byte_rows_util as bu
import byte_walk_util as bw


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_exports(g):
    """Fails on the parent commit."""
    from gbnns_dim_red_amd import binding
    assert "gbnns_debug_byte_walk_plan" in binding.SYMBOLS and hasattr(g.load_library(), "gbnns_debug_byte_walk_plan")
    assert g.FLAG_BYTE_WALK == 2048 and binding.FLAG_BYTE_WALK == 2048
    assert callable(g.byte_walk_plan)


@pytest.mark.parametrize("ef,stride,want", [
    (8, 32, "walk_reg_bytes_kernel<1, true>"), (64, 32, "walk_reg_bytes_kernel<1, true>"), (100, 32, "walk_reg_bytes_kernel<2, true>"),
    (200, 32, "walk_reg_big_bytes_kernel<true>"), (1024, 32, "walk_reg_big_bytes_kernel<true>"),
    (64, 48, "walk_reg_bytes_kernel<1, false>"), (64, 64, "walk_reg_bytes_kernel<1, false>"), (100, 48, "walk_reg_bytes_kernel<2, false>"),
    (100, 64, "walk_reg_bytes_kernel<2, false>"), (200, 48, "walk_reg_big_bytes_kernel<false>"), (1024, 64, "walk_reg_big_bytes_kernel<false>")])
def test_plan_inside_the_domain(g, ef, stride, want):
    """L2, dim 128, 2 048 rows: one list register up to ef 64, two up to 128, the two-list kernel up to 1 024; adjacency rows of one 32-slot
    pass get the forms without the pass loop."""
    assert g.byte_walk_plan(0, 128, bw.N, stride, ef) == want


@pytest.mark.parametrize("what,kw", [
    ("dim 48", dict(dim=48)), ("dim 100", dict(dim=100)), ("dim 96", dict(dim=96)), ("negative dot", dict(metric=1)),
    ("two entry points", dict(n_entries=2)), ("auxiliary graph", dict(aux_stride=16)), ("force_wide", dict(wide=True)), ("tagged", dict(tagged=True)),
    ("ef 1 025", dict(ef=1025)), ("n = 2^24", dict(n=1 << 24))], ids=lambda v: v if isinstance(v, str) else None)
def test_plan_outside_the_domain(g, what, kw):
    a = dict(metric=0, dim=128, n=bw.N, ell_stride=32, ef=64)
    a.update(kw)
    assert g.byte_walk_plan(a.pop("metric"), a.pop("dim"), a.pop("n"), a.pop("ell_stride"), a.pop("ef"), **a) == "walk_general_kernel", what
    # ... and at a two-list beam
    if "ef" not in kw:
        a = dict(metric=0, dim=128, n=bw.N, ell_stride=32, ef=200)
        a.update(kw)
        assert g.byte_walk_plan(a.pop("metric"), a.pop("dim"), a.pop("n"), a.pop("ell_stride"), a.pop("ef"), **a) == "walk_general_kernel", what


def test_plan_refuses_what_is_no_index(g):
    with pytest.raises(g.GbnnsError) as e:
        g.byte_walk_plan(0, 128, bw.N, 33, 64)
    assert e.value.code == 1
    with pytest.raises(g.GbnnsError) as e:
        g.byte_walk_plan(2, 128, bw.N, 32, 64)
    assert e.value.code == 1


def _walk_plan(g, metric, dim, n, stride, ef, n_entries=1, wide=0, pas=0):
    name, lds = C.create_string_buffer(128), C.c_uint64(0)
    assert g.load_library().gbnns_debug_walk_plan(metric, dim, (dim + 3) // 4 * 4, n, stride, 0, ef, n_entries, wide, 0, 0, 0, pas, 0, name, 128,
                                                  C.byref(lds)) == 0
    return name.value.decode(), lds.value


# (metric, dim, n, stride, ef, n_entries, wide, pass) -> what gbnns_debug_walk_plan answered before this flag existed (name, LDS bytes), and
# (name, fused) of gbnns_debug_byte_plan for the first-pass rows: literals taken from a build of the commit before the flag
PARENT_PLANS = [
    ((0, 128, 2048, 32, 8, 1, 0, 0), ("walk_reg_kernel<0, 0, true, false, 1, true, false>", 1168), ("walk_reg_kernel<0, 0, true, false, 1, true, false>", False)),
    ((0, 128, 2048, 32, 64, 1, 0, 0), ("walk_reg_kernel<0, 0, true, false, 1, true, false>", 1168), ("walk_reg_kernel<0, 0, true, false, 1, true, false>", False)),
    ((0, 128, 2048, 32, 100, 1, 0, 0), ("walk_reg_kernel<0, 0, true, false, 2, false, false>", 1680), ("walk_reg_kernel<0, 0, true, false, 2, false, false>", False)),
    ((0, 128, 2048, 32, 200, 1, 0, 0), ("walk_reg_big_kernel<0, 0, true, false, false, true, false>", 3216), ("walk_reg_big_kernel<0, 0, true, false, false, true, false>", False)),
    ((0, 128, 2048, 48, 300, 1, 0, 0), ("walk_reg_big_kernel<0, 32, true, false, false, false, false>", 3728), ("walk_reg_big_kernel<0, 32, true, false, false, false, false>", False)),
    ((0, 128, 2048, 32, 1025, 1, 0, 0), ("walk_fast_kernel<0, 0, false, true>", 9728), ("walk_fast_kernel<0, 0, false, true>", False)),
    ((0, 32, 2048, 32, 64, 1, 0, 0), ("walk_hot_kernel", 784), ("walk_hot_bytes_kernel", True)),
    ((0, 32, 2048, 32, 100, 1, 0, 0), ("walk_hot2_kernel", 1168), ("walk_hot2_bytes_kernel", True)),
    ((0, 32, 2048, 32, 200, 1, 0, 0), ("walk_hot_big_kernel", 2704), ("walk_hot_big_kernel", False)),
    ((0, 48, 2048, 32, 64, 1, 0, 0), ("walk_reg_wide_kernel<12, false>", 848), ("walk_reg_wide_kernel<12, false>", False)),
    ((1, 45, 2048, 32, 64, 1, 0, 0), ("walk_reg_kernel<1, 0, true, false, 1, true, false>", 848), ("walk_reg_kernel<1, 0, true, false, 1, true, false>", False)),
    ((1, 128, 2048, 32, 64, 2, 0, 0), ("walk_general_kernel", 1168), ("walk_general_kernel", False)),
    ((0, 128, 2048, 32, 64, 1, 1, 0), ("walk_reg_kernel<0, 0, false, false, 1, false, false>", 1168), ("walk_reg_kernel<0, 0, false, false, 1, false, false>", False)),
    ((0, 128, 2048, 32, 64, 1, 0, 2), ("walk_reg_kernel<0, 0, true, true, 1, false, false>", 1168), None),
    ((0, 32, 2048, 32, 400, 1, 0, 1), ("walk_bitmap_big_kernel<0, 8, true, false>", 4368), None),
    ((0, 128, 16777216, 32, 64, 1, 0, 0), ("walk_reg_kernel<0, 0, false, false, 1, false, false>", 1168), ("walk_reg_kernel<0, 0, false, false, 1, false, false>", False)),
    ((0, 100, 2048, 64, 100, 1, 0, 0), ("walk_reg_kernel<0, 0, true, false, 2, false, false>", 1568), ("walk_reg_kernel<0, 0, true, false, 2, false, false>", False)),
]


@pytest.mark.parametrize("args,walk,byte", PARENT_PLANS, ids=["m%d_d%d_n%d_s%d_ef%d_e%d_w%d_p%d" % a for a, _, _ in PARENT_PLANS])
def test_other_plan_functions_answer_as_before(g, args, walk, byte):
    metric, dim, n, stride, ef, n_entries, wide, pas = args
    assert _walk_plan(g, metric, dim, n, stride, ef, n_entries, wide, pas) == walk
    if byte is not None:
        assert g.byte_plan(metric, dim, n, stride, ef, n_entries=n_entries, wide=bool(wide)) == byte


# ---- fixture soundness: the GPU tests cannot pass vacuously -------------------------------------------------------------------------
@pytest.mark.parametrize("d", bw.RANDOM_DIMS)
def test_random_bytes_make_the_order_of_the_sums_visible(orc, d):
    """On 8 queries x all rows the oracle's L2 bits differ from an evaluation in which the two lanes of a pair never exchange sums on at least
    a quarter of the pairs: a kernel that adds a lane's chunks up on their own cannot return the expected rows."""
    c = bw.random_bytes(d)
    assert c["base"].dtype == np.uint8 and c["ent"][0] == bw.N - 1 and len(c["queries"]) == bw.NQ
    assert all((c["base"] == m).any() for m in bw.MARKS)
    assert c["queries"].min() >= 0.0 and c["queries"].max() <= 255.0 and not np.array_equal(c["queries"], np.round(c["queries"]))
    differ = total = 0
    for qi in range(8):
        want = bw.oracle_l2_bits(orc, c["wide"], c["queries"][qi])
        differ += int((bw.l2_bits_lanes_never_meet(c["wide"], c["queries"][qi]) != want).sum())
        total += len(want)
    print("random bytes d %d: lanes that never meet differ on %.3f of the pairs" % (d, differ / total))
    assert differ * 4 >= total, (d, differ, total)
    # the graphs: one 32-slot pass / two passes
    deg1, deg2 = np.diff(c["graphs"][1][0].astype(np.int64)), np.diff(c["graphs"][2][0].astype(np.int64))
    assert deg1.max() <= 32 and deg2.min() > 32 and deg2.max() <= 64


@pytest.mark.parametrize("graph", (1, 2))
def test_random_bytes_lists_hold_distinct_distances(orc, graph):
    """d = 128, every beam: every list is full, holds distinct distances and differs between queries; walks are longer than the beam.
    Measured: hops 9 .. 20 / 65 .. 88 / 101 .. 122 / 200 .. 210 and dist_calc 101 .. 1 688 on the one-pass graph, dist_calc 336 .. 2 039 on the
    two-pass graph."""
    c = bw.random_bytes(128)
    off, nbr = c["graphs"][graph]
    for ef in bw.BEAMS:
        w = bw.expected(orc, ("rb128", graph), c["queries"], c["wide"], off, nbr, ef, ef, c["ent"])
        assert (w["count"] == ef).all(), ef
        bits = np.ascontiguousarray(w["dists"]).view(np.uint32)
        # (among 200 float32 distances of one list a bit-equal pair turns up in a few lists -- 3 and 5 of 96 here: a tie the id breaks)
        assert all(len(np.unique(row)) >= (ef if ef <= 100 else ef - 1) for row in bits), ef
        assert len({row.tobytes() for row in w["ids"]}) == bw.NQ, ef
        assert (w["hops"] >= ef).all() or ef == 8, ef
        print("random bytes d 128 graph %d ef %d: hops %d .. %d, dist_calc %d .. %d" % (graph, ef, w["hops"].min(), w["hops"].max(),
                                                                                         w["dist_calc"].min(), w["dist_calc"].max()))


def test_hand_over_precondition(orc):
    """A visited set of 128 entries hands a query over once it has computed about 60 distances: at ef 64 the oracle's dist_calc exceeds 128
    for at least three quarters of the queries (here: for all of them), so `general_queries` of the GPU test is no accident."""
    c = bw.random_bytes(128)
    for graph in (1, 2):
        off, nbr = c["graphs"][graph]
        for ef in (64, 200):
            w = bw.expected(orc, ("rb128", graph), c["queries"], c["wide"], off, nbr, ef, ef, c["ent"])
            assert int((w["dist_calc"] > 128).sum()) * 4 >= 3 * bw.NQ, (graph, ef)


@pytest.mark.parametrize("metric,d,integer", bw.CONTESTS, ids=["m%d_d%d%s" % (m, d, "_int" if i else "") for m, d, i in bw.CONTESTS])
def test_contest_fixtures_are_sound(orc, metric, d, integer):
    """Every group holds distances that differ in their bits and a bit-equal pair (the integer form: one distance only -- the id decides),
    and the bytes 0, 127, 128, 255."""
    c = bw.contest(metric, d, integer)
    bits = bu.group_distance_bits(orc, c["base"], c["gq"], metric)
    print("byte contest", metric, d, integer, [len(np.unique(b)) for b in bits])
    for grp in range(bu.GROUPS):
        b = bits[grp]
        if integer:
            assert len(np.unique(b)) == 1, grp
        else:
            assert len(np.unique(b)) >= 2, ("one distance only", grp)
            assert len(np.unique(b)) < len(b), ("no bit-equal pair", grp)
        rows = c["base"][grp * bu.PER:(grp + 1) * bu.PER]
        assert all((rows == m).any() for m in bw.MARKS), grp
