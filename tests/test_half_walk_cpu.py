"""The half-row PLAIN walk (FLAG_HALF_WALK) without a device: the exports, gbnns_debug_half_walk_plan -- which flagged calls get a half-walk
first pass and which run whole on the general kernel's half-walk instance --, and the preconditions that keep
tests/test_gpu_half_walk.py from passing vacuously: on every fixture the order of the sums an instance could wrongly take is visible in
the bits of the distances.
"""
import re

import numpy as np
import pytest

import half_base_util as hb
import half_walk_util as hw


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_exports(g):
    """Fails on the parent commit."""
    import os
    from gbnns_dim_red_amd import binding
    assert "gbnns_debug_half_walk_plan" in binding.SYMBOLS and hasattr(g.load_library(), "gbnns_debug_half_walk_plan")
    assert g.FLAG_HALF_WALK == 8192 and binding.FLAG_HALF_WALK == 8192
    assert callable(g.half_walk_plan)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gbnns.h")).read()
    assert re.search(r"#define\s+GBNNS_FLAG_HALF_WALK\s+8192u", header)
    assert "gbnns_debug_half_walk_plan(" in header
    # the flag is a bit of its own
    flags = [int(v) for v in re.findall(r"#define\s+GBNNS_FLAG_\w+\s+(\d+)u", header)]
    assert len(flags) == len(set(flags)) and flags.count(8192) == 1


# d = 96: one list register up to ef 64 (over one- and two-pass adjacency rows), two up to 128 (one-pass rows only), the two-list kernel up
# to 1 024 (without and with the pass loop) -- the instance set the float path has for 24 steps
@pytest.mark.parametrize("ef,stride,want", [
    (8, 32, "walk_reg_hwalk_kernel<24, 1, true>"), (64, 32, "walk_reg_hwalk_kernel<24, 1, true>"), (100, 32, "walk_reg_hwalk_kernel<24, 2, true>"),
    (200, 32, "walk_reg_big_hwalk_kernel<24, true>"), (1024, 32, "walk_reg_big_hwalk_kernel<24, true>"),
    (8, 64, "walk_reg_hwalk_kernel<24, 1, false>"), (64, 48, "walk_reg_hwalk_kernel<24, 1, false>"), (64, 64, "walk_reg_hwalk_kernel<24, 1, false>"),
    (200, 48, "walk_reg_big_hwalk_kernel<24, false>"), (200, 64, "walk_reg_big_hwalk_kernel<24, false>"), (1024, 64, "walk_reg_big_hwalk_kernel<24, false>"),
    (1024, 80, "walk_reg_big_hwalk_kernel<24, false>")])
def test_plan_d96(g, ef, stride, want):
    assert g.half_walk_plan(0, 96, hw.N, stride, ef) == want


@pytest.mark.parametrize("ef,stride", [(100, 48), (100, 64), (128, 64), (64, 80), (100, 80)])
def test_plan_d96_without_a_24_step_instance(g, ef, stride):
    """Two list registers over two-pass adjacency rows, and register lists over longer rows: the float path has no 24-step instance there
    either; the general instance takes the batch."""
    assert g.half_walk_plan(0, 96, hw.N, stride, ef) == "walk_general_kernel"


@pytest.mark.parametrize("d", [128, 300, 404, 960])
@pytest.mark.parametrize("ef,stride,want", [
    (8, 32, "walk_reg_hwalk_kernel<0, 1, true>"), (64, 64, "walk_reg_hwalk_kernel<0, 1, true>"), (64, 80, "walk_reg_hwalk_kernel<0, 1, false>"),
    (100, 32, "walk_reg_hwalk_kernel<0, 2, false>"), (100, 64, "walk_reg_hwalk_kernel<0, 2, false>"),
    (200, 32, "walk_reg_big_hwalk_kernel<0, true>"), (200, 64, "walk_reg_big_hwalk_kernel<0, true>"), (1024, 80, "walk_reg_big_hwalk_kernel<0, false>")])
def test_plan_long_rows(g, d, ef, stride, want):
    """d >= 128, d % 4 == 0: the run-time-length instances; their passes are 64 slots wide."""
    assert g.half_walk_plan(0, d, hw.N, stride, ef) == want


@pytest.mark.parametrize("what,kw", [
    ("dim 45", dict(dim=45)), ("dim 40", dict(dim=40)), ("dim 8", dict(dim=8)), ("dim 12", dict(dim=12)), ("dim 100", dict(dim=100)),
    ("dim 130", dict(dim=130)), ("negative dot", dict(metric=1)), ("negative dot, dim 128", dict(metric=1, dim=128)),
    ("two entry points", dict(n_entries=2)), ("auxiliary graph", dict(aux_stride=16)), ("force_wide", dict(wide=True)), ("tagged", dict(tagged=True)),
    ("ef 1 025", dict(ef=1025)), ("n = 2^24", dict(n=1 << 24))], ids=lambda v: v if isinstance(v, str) else None)
def test_plan_outside_the_domain(g, what, kw):
    for dim in (96, 128, 960):
        for ef in (64, 100, 200):
            a = dict(metric=0, dim=dim, n=hw.N, ell_stride=32, ef=ef)
            a.update(kw)
            assert g.half_walk_plan(a.pop("metric"), a.pop("dim"), a.pop("n"), a.pop("ell_stride"), a.pop("ef"), **a) == "walk_general_kernel", (what, dim, ef)


def test_plan_a_half_table_of_4_gib_is_not_compact(g):
    """n x round_up(d, 8) x 2 bytes: 2^21 rows of 960 halves are 3.75 GiB, 2^22 rows are not a compact index any more."""
    assert g.half_walk_plan(0, 960, 1 << 21, 32, 64) == "walk_reg_hwalk_kernel<0, 1, true>"
    assert g.half_walk_plan(0, 960, 1 << 22, 32, 64) == "walk_general_kernel"


def test_plan_refuses_what_is_no_index(g):
    with pytest.raises(g.GbnnsError) as e:
        g.half_walk_plan(0, 96, hw.N, 33, 64)
    assert e.value.code == 1
    with pytest.raises(g.GbnnsError) as e:
        g.half_walk_plan(2, 96, hw.N, 32, 64)
    assert e.value.code == 1


def test_unflagged_plans_do_not_move(g):
    """The plan of an unflagged call over float rows of the same dimensions names what it named before the flag existed (literals taken
    from a build of the commit before it; tests/golden/walk_plan_grid.txt pins the whole grid)."""
    import ctypes as C

    def walk_plan(dim, stride, ef):
        name, lds = C.create_string_buffer(128), C.c_uint64(0)
        assert g.load_library().gbnns_debug_walk_plan(0, dim, dim, hw.N, stride, 0, ef, 1, 0, 0, 0, 0, 0, 0, name, 128, C.byref(lds)) == 0
        return name.value.decode()

    assert walk_plan(96, 32, 64) == "walk_reg_kernel<0, 24, true, false, 1, true, false>"
    assert walk_plan(96, 32, 200) == "walk_reg_big_kernel<0, 24, true, false, false, true, false>"
    assert walk_plan(128, 32, 64) == "walk_reg_kernel<0, 0, true, false, 1, true, false>"
    assert walk_plan(128, 32, 200) == "walk_reg_big_kernel<0, 0, true, false, false, true, false>"


# ---- fixture soundness: the GPU tests cannot pass vacuously -------------------------------------------------------------------------
@pytest.mark.parametrize("d", hw.PAIR_DIMS + hw.LONG_DIMS)
def test_contest_groups_show_the_order_of_the_sums(orc, d):
    """In every contest group at least 64 of the 256 rows change their distance bits under the wrong order an instance of that dimension
    could take -- d = 96: the two lanes' halves of the row summed apart and added at the end; the long rows: alternate 16-byte chunks
    summed apart -- and under the other one as well.  The same NumPy restatement in the reference's order reproduces the oracle's bits."""
    c = hw.contest(0, d)
    assert c["base"].dtype == np.float16 and all(hb.marks_present(c["base"], d, 0))
    want = hb.group_distance_bits(orc, c["base"], c["gq"], 0)
    low = {}
    for grp in range(hw.GROUPS):
        rows = c["wide"][grp * hw.PER:(grp + 1) * hw.PER]
        assert np.array_equal(hw.l2_bits_reference_order(rows, c["gq"][grp]), want[grp]), grp
        for name, order in (("lane halves", hw.lane_halves), ("alternate chunks", hw.alternate_chunks)):
            differ = int((hw.l2_bits_summed_apart(rows, c["gq"][grp], order) != want[grp]).sum())
            low[name] = min(low.get(name, hw.PER), differ)
            assert differ >= 64, (d, grp, name, differ)
        # ... and the group holds distances that differ in their bits and a bit-equal pair (the three exact copies)
        assert 2 <= len(np.unique(want[grp])) < hw.PER, grp
    print("half contest d %d: rows of 256 whose bits change, the least over the groups: %s" % (d, low))


@pytest.mark.parametrize("d", hw.RANDOM_DIMS)
def test_random_halves_make_the_order_of_the_sums_visible(orc, d):
    """On 8 queries x all rows the oracle's L2 bits differ from both wrong orders on at least a quarter of the pairs; every row value is a
    finite binary16 with an odd mantissa field, every query coordinate a float32 with its last mantissa bit set."""
    c = hw.random_halves(d)
    bits = hb.bits_of(c["base"])
    assert c["base"].dtype == np.float16 and (bits & 1).all() and ((bits & 0x7C00) != 0x7C00).all()
    assert (c["queries"].view(np.uint32) & 1).all() and c["ent"][0] == hw.N - 1 and len(c["queries"]) == hw.NQ
    for name, order in (("lane halves", hw.lane_halves), ("alternate chunks", hw.alternate_chunks)):
        differ = total = 0
        for qi in range(8):
            want = hw.oracle_l2_bits(orc, c["wide"], c["queries"][qi])
            assert np.array_equal(hw.l2_bits_reference_order(c["wide"], c["queries"][qi]), want)
            differ += int((hw.l2_bits_summed_apart(c["wide"], c["queries"][qi], order) != want).sum())
            total += len(want)
        print("random halves d %d: %s summed apart differ on %.3f of the pairs" % (d, name, differ / total))
        assert differ * 4 >= total, (d, name, differ, total)
    deg1, deg2 = np.diff(c["graphs"][1][0].astype(np.int64)), np.diff(c["graphs"][2][0].astype(np.int64))
    assert deg1.max() <= 32 and deg2.min() > 32 and deg2.max() <= 64


@pytest.mark.parametrize("d", hw.RANDOM_DIMS)
@pytest.mark.parametrize("graph", (1, 2))
def test_random_halves_lists_hold_distinct_distances(orc, d, graph):
    """Every beam: every list is full, holds distinct distances (among the 100 or 200 float32 distances of one list a bit-equal pair turns up
    in a few lists: a tie the id breaks) and differs between queries."""
    c = hw.random_halves(d)
    off, nbr = c["graphs"][graph]
    for ef in hw.BEAMS:
        w = hw.expected(orc, ("hw random", d, graph), c["queries"], c["wide"], off, nbr, ef, ef, c["ent"])
        assert (w["count"] == ef).all(), ef
        bits = np.ascontiguousarray(w["dists"]).view(np.uint32)
        assert all(len(np.unique(row)) >= (ef if ef < 100 else ef - 1) for row in bits), ef
        assert len({row.tobytes() for row in w["ids"]}) == hw.NQ, ef
        print("random halves d %d graph %d ef %d: hops %d .. %d, dist_calc %d .. %d" % (d, graph, ef, w["hops"].min(), w["hops"].max(),
                                                                                       w["dist_calc"].min(), w["dist_calc"].max()))


@pytest.mark.parametrize("d", (96, 300))
def test_hand_over_precondition(orc, d):
    """A visited set of 128 entries hands a query over once it has computed about 60 distances: at ef 64 and 200 over the two-pass graph the
    oracle's dist_calc exceeds 128 for at least three quarters of the queries, so `general_queries` of the GPU test is no accident."""
    c = hw.random_halves(d)
    off, nbr = c["graphs"][2]
    for ef in (64, 200):
        w = hw.expected(orc, ("hw random", d, 2), c["queries"], c["wide"], off, nbr, ef, ef, c["ent"])
        assert int((w["dist_calc"] > 128).sum()) * 4 >= 3 * hw.NQ, (d, ef)
