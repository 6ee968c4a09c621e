"""gbnns_index_tag_census / gbnns_search_tagged_auto without a device: the NumPy census against the definition, the fixture's conditions
(the table of tests/tag_auto_util.py; a query sent down the wrong route would be visible), the composed expectation's self-consistency, and
the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import gbnns_dim_red_amd as g
import knn_tagged_util as kt
import tag_auto_util as au
import tag_util as tg
from gbnns_dim_red_amd import binding


@pytest.fixture(scope="module")
def lib():
    return g.load_library()


def test_census_of_the_fixture_is_the_documented_table():
    T, Q = tg.row_tags(), au.query_words()
    allowed, first = g.tag_census(T, Q)
    assert allowed.dtype == np.uint32 and first.dtype == np.uint32
    for i, q in enumerate(Q):
        assert (int(allowed[i]), int(first[i])) == au.CENSUS[int(q)], (i, hex(int(q)))
    loops = au.census_loops(T, Q[:len(au.WORDS)])
    assert np.array_equal(allowed[:len(au.WORDS)], loops[0]) and np.array_equal(first[:len(au.WORDS)], loops[1])


@pytest.mark.parametrize("n", [5, 1037, 6000])
def test_census_equals_the_double_loop(n):
    T, Q = kt.tag_table(n, n), kt.query_words(13)
    got, want = g.tag_census(T, Q), au.census_loops(T, Q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert 0 in want[0] and n in want[0]   # word 0, and all ones


def test_census_of_the_lane_map():
    T, Q = kt.lane_map_tags(1037, 40)
    got, want = g.tag_census(T, Q), au.census_loops(T, Q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[1], np.arange(40) % 32)


def test_census_of_nothing():
    a, f = g.tag_census(tg.row_tags(), np.zeros(0, np.uint32))
    assert a.shape == (0,) and f.shape == (0,)


def test_scan_below_values_split_the_words_as_documented():
    allowed, _ = g.tag_census(tg.row_tags(), np.array(au.WORDS, np.uint32))
    scans = {sb: tuple(au.routes(allowed, sb)) for sb in au.SCAN_BELOW}
    #                          0x0F   0x01   0xFF   0x02   0xF0   0x100  0
    assert scans[0] == (False, False, False, False, False, True, True)
    assert scans[300] == (False, True, False, True, False, True, True)
    assert scans[1023] == scans[300]
    assert scans[1024] == (True, True, False, True, True, True, True)
    assert scans[2 ** 64 - 1] == (True,) * 7


def test_configurations_cover_every_beam_k_metric_and_walk():
    for m in (0, 1):
        assert {ef for mm, ef, _, _ in au.CONFIGS if mm == m} == set(au.EFS)
        assert {k for mm, _, k, _ in au.CONFIGS if mm == m} == set(au.KS)
        assert {b for mm, _, _, b in au.CONFIGS if mm == m} == {False, True}
    assert all(set(au.scan_below_of(64)) == set(au.SCAN_BELOW) and 300 in au.scan_below_of(ef) for ef in au.EFS)


@pytest.mark.parametrize("metric,ef,k,bridge", au.CONFIGS, ids=["m%d_ef%d_k%d_bridge%d" % s for s in au.CONFIGS])
def test_the_two_routes_give_different_rows(orc, metric, ef, k, bridge):
    """The condition on the fixture, for every configuration the device tests run: for at least three quarters of the queries of every
    non-empty word the walk's top-k row (entered at the lowest allowed row) differs from the exact row -- a query sent down the wrong
    route shows, in either direction."""
    c = au.fixture(metric)
    walk, scan = au.both_routes(orc, ("fixture", metric), c, ef, k, metric, bridge=bridge)
    differ = (walk != scan).any(axis=1)
    for q in au.WORDS:
        sel = c["Q"] == q
        if au.CENSUS[q][0] == 0:
            assert not differ[sel].any(), hex(q)   # nothing allowed: the empty row on both routes
        else:
            assert 4 * differ[sel].sum() >= 3 * sel.sum() > 0, (hex(q), int(differ[sel].sum()), int(sel.sum()))


@pytest.mark.parametrize("bridge", [False, True])
def test_composed_expectation_is_self_consistent(orc, bridge):
    metric, ef, k = 0, 64, 10
    c = au.fixture(metric)
    for sb in (0, 300, 2 ** 64 - 1):
        e = au.expected(orc, ("fixture", metric), c, ef, k, metric, sb, bridge=bridge)
        scan = e["route"] == 1
        assert np.array_equal(scan, au.routes(e["allowed"], sb))
        # a walk row: column 0 of the k-answer row is the re-ranked answer, and every id is allowed
        assert np.array_equal(e["top_ids"][~scan, 0], e["want"][~scan]) and np.array_equal(e["ids"][~scan], e["want"][~scan])
        assert (e["ids"][~scan] != au.NONE).all()   # entered at an allowed row: no walk-routed query gets the empty row
        # a scan row: the bad-entry row in the walk's outputs, column 0 as the answer
        assert (e["cand"][scan] == au.NONE).all() and np.isinf(e["cand_dist"][scan]).all()
        assert (e["hops"][scan] == 0).all() and (e["dist_calc"][scan] == 0).all()
        assert np.array_equal(e["ids"][scan], e["top_ids"][scan, 0])
        seen = e["top_ids"] != au.NONE
        assert ((c["T"][np.where(seen, e["top_ids"], 0)] & c["Q"][:, None]) != 0)[seen].all()
        empty = e["allowed"] == 0
        assert (e["top_ids"][empty] == au.NONE).all() and scan[empty].all()
    # with the fixture's random entry points some walk-routed queries may not see their entry: they get the empty row
    e = au.expected(orc, ("fixture", metric), c, ef, k, metric, 300, ent=c["ent"], bridge=bridge)
    walk = e["route"] == 0
    bad = walk & ~tg.entry_ok(c["T"], c["Q"], c["ent"])
    assert bad.any() and (e["ids"][bad] == au.NONE).all() and (e["top_ids"][bad] == au.NONE).all()
    assert (e["ids"][walk & ~bad] != au.NONE).all()


def test_new_symbols_are_declared_and_exported(lib):
    for name in ("gbnns_index_tag_census", "gbnns_search_tagged_auto"):
        assert name in binding.SYMBOLS and hasattr(lib, name)
    assert g.tag_census is binding.tag_census


def test_null_arguments_are_refused_without_a_device(lib):
    q = np.ones(4, np.uint32)
    out = np.zeros(4, np.uint32)
    assert lib.gbnns_index_tag_census(None, q.ctypes.data, 4, out.ctypes.data, out.ctypes.data, binding.MEM_HOST, None) == 1
    a = binding._SearchArgs(struct_size=C.sizeof(binding._SearchArgs), mode=binding.MODE_LOWQ, ef=8, k=8, n_q=4)
    assert lib.gbnns_search_tagged_auto(None, C.byref(a), None, q.ctypes.data, 1, 0, out.ctypes.data, None, None, None) == 1
    assert b"null" in lib.gbnns_last_error()
    assert lib.gbnns_search_tagged_auto(None, None, None, q.ctypes.data, 1, 0, out.ctypes.data, None, None, None) == 1
