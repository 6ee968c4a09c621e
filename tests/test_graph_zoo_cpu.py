"""The graph zoo on the CPU (no device): tests/graph_zoo.py holds what it says, the planned kernel names of the census are unchanged by it,
and the oracle is a valid expectation on every graph -- its walk on the raw CSR, its walk on the de-duplicated rows (the claim of
build_ell's comment) and the compiled reference's walk are the same bytes.  What tests/test_gpu_graph_zoo.py asserts about short lists,
dead ends, retry hand-overs and edge counts are therefore conditions the kernels have to meet, not observations.
"""
import ctypes

import numpy as np
import pytest

import golden_util as gu
import graph_zoo as gz
import walk_instances as wi

N = 3000
BEAMS = (1, 8, 64, 200, 1100)
KEY = (0, 32)            # the seed key of the L2 / 32-float census set
NAMES = ("ids", "dists", "count", "hops", "dist_calc")


@pytest.fixture(scope="module")
def lib():
    import gbnns_dim_red_amd as g
    return g.load_library()


def _lens(off):
    return np.diff(np.asarray(off).astype(np.int64))


def _same(a, b):
    """Names of the walk outputs that differ between two walks, byte for byte (distances by bit pattern)."""
    return [k for k in NAMES if (gu.bits(a[k]) if k == "dists" else a[k]).tobytes() != (gu.bits(b[k]) if k == "dists" else b[k]).tobytes()]


_MEMO = {}


def _walk(orc, topo, cap, ef, n=N):
    key = (topo, cap, ef, n)
    if key not in _MEMO:
        v = wi.vectors(0, 32, n)
        off, nbr = gz.zoo(topo, n, cap, KEY)
        _MEMO[key] = orc.walk(v["q_low"], v["db_low"], off, nbr, ef, entries=gz.entries(topo, n, cap, KEY), threads=8)
    return _MEMO[key]


@pytest.mark.parametrize("cap", gz.CAPS)
def test_every_topology_has_the_cap_and_the_stride_of_its_degree_class(cap):
    for n in (3000, 6000):
        for topo in gz.TOPOLOGIES:
            off, nbr = gz.zoo(topo, n, cap, KEY)
            assert len(off) == n + 1 and int(off[-1]) == len(nbr) and (nbr < n).all()
            assert _lens(off).max() == cap, (topo, n)
            assert (cap + 15) // 16 * 16 == wi.ELL_STRIDE[gz.DEG_OF_CAP[cap]]
            assert _lens(gz.zoo_dedup(topo, n, cap, KEY)[0]).max() <= cap
            aoff, _ = gz.zoo_aux(topo, n, cap, KEY)
            assert (_lens(aoff).max() + 15) // 16 * 16 == wi.AUX_STRIDE and (_lens(aoff)[::2] == 0).all()
            ent = gz.entries(topo, n, cap, KEY)
            assert ent[0] == n - 1 and ent.shape == (gz.NQ,) and (ent < n).all()


def test_the_planned_names_of_the_census_are_the_zoo_s(lib):
    """The plan takes the stride, never the rows: with max(row length) == cap every census case's plan_args are unchanged, and the plan
    still names case.first and case.retry."""
    def plan(args):
        name, lds = ctypes.create_string_buffer(128), ctypes.c_uint64()
        assert lib.gbnns_debug_walk_plan(*args, name, 128, ctypes.byref(lds)) == 0
        return name.value.decode()
    for c in wi.CASES:
        off, _, _ = gz.case_graph(c, "ragged")
        assert (int(_lens(off).max()) + 15) // 16 * 16 == c.plan_args(0)[4]
        assert plan(c.plan_args(c.first_pass)) == c.first, c
        if c.hash_capacity:
            assert plan(c.plan_args(2)) == c.retry, c


def test_the_feature_instances_named_on_the_zoo_are_the_plan_s(lib):
    """tag_util.tag_kernel / bridge_util.bridge_kernel, which the device suite asserts, against gbnns_debug_tag_plan /
    gbnns_debug_bridge_plan at the zoo's strides; the tagged batch keeps dead-end entries and has entries its word does not allow."""
    import bridge_util as bru
    import gbnns_dim_red_amd as g
    import tag_util as tg
    for cap in (32, 64):
        for ef in (8, 64, 100, 200):
            assert g.tag_plan(0, 32, N, cap, ef) == tg.tag_kernel(0, 32, ef, cap == 32)
            assert g.bridge_plan(0, 32, N, cap, ef) == bru.bridge_kernel(0, 32, ef)
            assert g.byte_plan(0, 32, N, cap, ef)[1] == (cap == 32 and ef <= 128)   # the fused byte re-rank runs on the one-pass rows
            assert g.byte_walk_plan(0, 128, N, cap, ef) != "walk_general_kernel" != g.byte_query_plan(0, 128, N, cap, ef)
        T, Q = tg.row_tags(N), tg.query_tags(gz.NQ)
        for topo in ("ragged", "islands", "star"):
            ent = gz.entries(topo, N, cap, KEY)
            tent = gz.tagged_entries(ent, T, Q)
            ok = tg.entry_ok(T, Q, tent)
            assert sorted(np.flatnonzero(~ok)) == list(gz.DISALLOWED)
            lens = _lens(gz.zoo(topo, N, cap, KEY)[0])
            assert (lens[tent[ok]] == 0).sum() >= 2 and (tent[Q == 0xFF] == ent[Q == 0xFF]).all()


@pytest.mark.parametrize("cap", gz.CAPS)
def test_ragged_holds_the_edge_cases_it_claims(cap):
    off, nbr = gz.zoo("ragged", N, cap, KEY)
    rows, lens = gz.rows(off, nbr), _lens(off)
    for want in (0, 1, cap - 1, cap):
        assert (lens == want).any(), want
    loops = [(i, int(s)) for i, r in enumerate(rows) for s in np.flatnonzero(r == i)]
    assert any(s == 0 for _, s in loops) and any(s == len(rows[i]) - 1 and s > 0 for i, s in loops)
    inside = across = 0
    for i, r in enumerate(rows):
        if i % 5 == 0 and len(r) >= 4:
            assert r[len(r) // 2] == r[0] and r[-1] == r[1], i
        for val in np.unique(r):
            s = np.flatnonzero(r == val)
            if len(s) > 1:
                inside += int(s[0] // 32 == s[1] // 32)
                across += int(s[0] // 32 != s[-1] // 32)
    assert inside > 0 and (across > 0 or cap == 32)
    doff, dnbr = gz.zoo_dedup("ragged", N, cap, KEY)
    assert 10 * int((_lens(doff) < lens).sum()) >= N
    for r, d in zip(rows[:200], gz.rows(doff, dnbr)[:200]):   # dedup against a plain restatement of build_ell's loop
        seen = []
        for x in r:
            if x not in seen:
                seen.append(x)
        assert list(d) == seen
    ent = gz.entries("ragged", N, cap, KEY)
    assert int((lens[ent] == 0).sum()) >= 8 and (lens[ent[1:1 + gz.DEAD_ENTRIES]] == 0).all() and lens[ent[0]] == cap
    aoff, anbr = gz.zoo_aux("ragged", N, cap, KEY)
    arows = gz.rows(aoff, anbr)
    assert all(list(arows[i][:min(3, len(rows[i]))]) == list(rows[i][:3][::-1]) for i in range(1, N, 2))


@pytest.mark.parametrize("topo", ("islands", "star"))
def test_small_component_topologies_are_what_they_claim(topo):
    for cap in gz.CAPS:
        off, nbr = gz.zoo(topo, N, cap, KEY)
        rows, lens = gz.rows(off, nbr), _lens(off)
        assert (lens == 0).any() and all(i not in r and len(np.unique(r)) == len(r) for i, r in enumerate(rows))
        if topo == "islands":
            start, size = gz.island_of(N, cap)
            assert set(size[:-97].tolist()) == set(gz.island_sizes(cap))
            assert all((r >= start[i]).all() and (r < start[i] + size[i]).all() and len(r) == min(size[i] - 1, cap) for i, r in enumerate(rows))
        else:
            hub = np.arange(N) - np.arange(N) % (cap + 1)
            assert all((r == hub[i]).all() if i != hub[i] else (hub[r] == i).all() for i, r in enumerate(rows))
            assert (lens[hub == np.arange(N)][:-1] == cap).all() and set(lens[hub != np.arange(N)].tolist()) == {0, 1}


def test_consequences_on_the_oracle_s_walks(orc):
    for cap in gz.CAPS:
        for ef in BEAMS:
            for topo in ("islands", "star", "funnel"):
                w = _walk(orc, topo, cap, ef)
                if ef >= 200:
                    assert (w["count"] < ef).all(), (topo, cap, ef)
                # no component within reach holds more rows: cap + 1, or the 65-row island whose rows are cut to cap
                assert w["dist_calc"].max() <= (max(cap + 1, 66) if topo == "islands" else cap + 1), (topo, cap, ef)
            if ef >= 8:
                w = _walk(orc, "ragged", cap, ef)
                assert 4 * int((w["count"] < ef).sum()) >= gz.NQ, (cap, ef)
                ent = gz.entries("ragged", N, cap, KEY)
                assert (w["count"][1:1 + gz.DEAD_ENTRIES] == 1).all() and (w["hops"][1:1 + gz.DEAD_ENTRIES] == 1).all()
                w = _walk(orc, "path", cap, ef)
                assert w["hops"].min() >= ef and (w["dist_calc"] <= w["hops"] + cap).all() and (w["count"] == ef).all(), (cap, ef)
        # funnel: every hop after the first finds nothing fresh
        w = _walk(orc, "funnel", cap, 1100)
        assert (w["dist_calc"] == w["count"]).all() and (w["hops"] == w["count"]).all() and w["count"].max() == cap + 1


def test_rows_past_count_are_padded_in_the_oracle_too(orc):
    """The padding the device suite asserts (0xFFFFFFFF ids; the oracle leaves no distance there) starts at `count`."""
    w = _walk(orc, "star", 32, 200)
    for i in range(gz.NQ):
        assert (w["ids"][i, :w["count"][i]] < N).all() and (w["ids"][i, w["count"][i]:] == gz.NONE).all()


@pytest.mark.parametrize("topo", gz.TOPOLOGIES)
def test_oracle_on_raw_rows_equals_oracle_on_deduplicated_rows_and_the_reference(orc, ref, topo):
    v = wi.vectors(0, 32, N)
    for cap in gz.CAPS:
        off, nbr = gz.zoo(topo, N, cap, KEY)
        doff, dnbr = gz.zoo_dedup(topo, N, cap, KEY)
        ent = gz.entries(topo, N, cap, KEY)
        for ef in BEAMS:
            w = _walk(orc, topo, cap, ef)
            d = orc.walk(v["q_low"], v["db_low"], doff, dnbr, ef, entries=ent, threads=8)
            r = ref.walk(v["q_low"], v["db_low"], off, nbr, ef, entries=ent, threads=8)
            assert not _same(w, d), (topo, cap, ef, "de-duplicated", _same(w, d))
            assert not _same(w, r), (topo, cap, ef, "reference", _same(w, r))


def test_oracle_equals_oracle_on_deduplicated_rows_without_the_reference(orc):
    """The same claim where the compiled reference is absent: ragged is the only topology with repeats."""
    v = wi.vectors(0, 32, N)
    for cap in gz.CAPS:
        doff, dnbr = gz.zoo_dedup("ragged", N, cap, KEY)
        for ef in BEAMS:
            d = orc.walk(v["q_low"], v["db_low"], doff, dnbr, ef, entries=gz.entries("ragged", N, cap, KEY), threads=8)
            assert not _same(_walk(orc, "ragged", cap, ef), d), (cap, ef)


@pytest.mark.parametrize("topo", ("ragged", "islands", "star", "knots"))
def test_repeated_entry_points_and_overlapping_auxiliary_rows_equal_the_reference(orc, ref, topo):
    """The inputs of the device suite's two-entry searches: [e, e], [e, e's first neighbour], [a dead end, e], alone and with the
    auxiliary graph that repeats ids of the main rows, LLF on and off, hops_bound 50 and 3."""
    v = wi.vectors(0, 32, N)
    for cap in (32, 96):
        off, nbr = gz.zoo(topo, N, cap, KEY)
        doff, dnbr = gz.zoo_dedup(topo, N, cap, KEY)
        aux = gz.zoo_aux(topo, N, cap, KEY)
        daux = gz.dedup(*aux)   # (an auxiliary row may repeat an id of its own: build_ell drops that too)
        for kind in gz.ENTRY_KINDS:
            ent = gz.two_entries(topo, N, cap, KEY, kind)
            assert ent.shape == (gz.NQ, 2)
            for ef in (1, 8, 64, 200):
                for use_aux, llf, hb in gz.ENTRY_RUNS:
                    kw = dict(aux=aux, llf=llf, hops_bound=hb) if use_aux else {}
                    dkw = dict(kw, aux=daux) if use_aux else {}
                    w = orc.walk(v["q_low"], v["db_low"], off, nbr, ef, entries=ent, threads=8, **kw)
                    d = orc.walk(v["q_low"], v["db_low"], doff, dnbr, ef, entries=ent, threads=8, **dkw)
                    r = ref.walk(v["q_low"], v["db_low"], off, nbr, ef, entries=ent, threads=8, **kw)
                    assert not _same(w, d) and not _same(w, r), (topo, cap, kind, ef, use_aux, llf, hb, _same(w, d), _same(w, r))


def test_ragged_retry_cases_outgrow_their_visited_set(orc):
    """test_walk_instance_retry_cases_outgrow_their_visited_set's criterion on ragged: at least half the batch computes more distances
    than the visited set holds -- a third of the batch are dead ends and short walks there, so the share is a half, not three quarters."""
    cases = [c for c in wi.CASES if c.hash_capacity]
    assert len({c.retry for c in cases}) == 77
    for c in cases:
        over = gz.over(orc, c)
        assert 2 * over >= gz.NQ, (c, over)
        assert over == int((gz.oracle_walk(orc, c, "ragged")[0]["dist_calc"] > c.hash_capacity).sum())


def test_a_short_list_s_edges_are_the_kept_degrees_of_its_rows(orc):
    """short_list_edges on every topology: its premise (a list that never fills has hops == count; asserted inside), agreement with
    degree x hops where both cover a query, and its power: raw degrees give another sum for some short list, so the device
    suite's comparison tells counting raw slots from counting kept ones (on knots at ef 200 for at least half the batch).  With the auxiliary graph and no LLF some queries stay covered."""
    v = wi.vectors(0, 32, N)
    for cap in gz.CAPS:
        for topo in gz.TOPOLOGIES:
            off, nbr = gz.zoo(topo, N, cap, KEY)
            ent = gz.entries(topo, N, cap, KEY)
            for ef in (8, 64, 200):
                w = _walk(orc, topo, cap, ef)
                exp, mask = gz.short_list_edges(gz.kept_degrees(topo, N, cap, KEY), w, ef)
                uni, covered = gz.expected_edges(topo, N, cap, KEY, ent, w["hops"])
                assert (exp[mask & covered] == uni[mask & covered]).all(), (topo, cap, ef)
                if topo == "knots":   # (ragged's short lists are dead ends and rows of one id: no repeat within their reach)
                    raw, _ = gz.short_list_edges(_lens(off), w, ef)
                    assert 2 * int((raw[mask] > exp[mask]).sum()) >= gz.NQ or ef < 200, (cap, ef, int(mask.sum()))
            for hb in (3, 50):
                w = orc.walk(v["q_low"], v["db_low"], off, nbr, 200, entries=ent, threads=8, aux=gz.zoo_aux(topo, N, cap, KEY), llf=False, hops_bound=hb)
                exp, mask = gz.short_list_edges(gz.kept_degrees(topo, N, cap, KEY, aux=True), w, 200, hops_bound=hb)
                assert mask.any() or topo in ("path", "funnel") or hb == 3, (topo, cap, hb)


def test_edge_counts_follow_from_hops_where_degrees_are_uniform(orc):
    """expected_edges' premise, checked against the graphs: on the covered queries every row within reach of the entry has one degree."""
    for cap in gz.CAPS:
        for ef in (8, 200):
            for topo in gz.TOPOLOGIES:
                off, nbr = gz.zoo(topo, N, cap, KEY)
                lens, ent = _lens(off), gz.entries(topo, N, cap, KEY)
                w = _walk(orc, topo, cap, ef)
                exp, mask = gz.expected_edges(topo, N, cap, KEY, ent, w["hops"])
                assert mask.all() == (topo in ("funnel", "islands")) and mask.any() == (topo in ("funnel", "islands", "path"))
                assert (_lens(gz.zoo_dedup(topo, N, cap, KEY)[0]) == lens).all() or topo in ("ragged", "knots")
                for i in np.flatnonzero(mask):
                    if topo == "path":
                        walked = np.arange(ent[i], ent[i] + w["hops"][i])
                        assert walked.max() < N - 1 and (lens[walked] == 1).all() and exp[i] == w["hops"][i]
                    elif topo == "funnel":
                        assert (lens == cap).all() and exp[i] == cap * w["hops"][i]
                    else:
                        start, size = gz.island_of(N, cap)
                        members = np.arange(start[ent[i]], start[ent[i]] + size[ent[i]])
                        assert (lens[members] == lens[ent[i]]).all() and exp[i] == lens[ent[i]] * w["hops"][i]
