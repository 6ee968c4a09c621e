"""Every distance form at every row-length class, bit for bit, on an MI355X (run with -m gpu): each entry point of the library runs at every
length of tests/dim_sweep.py's table -- which tests/test_dim_sweep_cpu.py proves to put 0, 1 and >= 2 trips on every rung of every distance
ladder and a length on each side of every switch between forms -- against the CPU oracle, which tests/golden/kats.npz pins to the compiled
reference at d = 0 .. 40.

One test per entry point; the lengths are looped inside, one Index per length, and mismatches are collected so that one run names every
failing length.  Nothing takes a tolerance: ids, distance bit patterns, hops and dist_calc are compared for equality with the oracle's
scalar l2 / negdot, orc.walk, orc.rerank and orc.exact_knn.  2 048 rows, 64 queries, candidate rows of 70 with counts cycling through
0, 1, 31, 32, 33, 64, 65, 70; full-mantissa data (a wrong rung changes >= 99 % of the distance bits, a wrong order >= 10 %: the CPU test),
and the equal-distance contests of datagen where named.  Which form a length takes is asked from the plan functions, and each test
prints the census of the forms it ran.
"""
import collections

import numpy as np
import pytest

import datagen
import dim_sweep as ds
import golden_util as gu
import knn_bytes_util as ku
import topk_util as tu

pytestmark = pytest.mark.gpu

NONE = ds.NONE
WANT = ("hops", "dist_calc", "cand", "cand_dist")


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _rows_differ(got_ids, got_dist, want_ids, want_dist, what):
    """What differs between two [nq x k] tables of ids and distances (bit patterns), as a list of strings."""
    bad = []
    rows = np.flatnonzero((got_ids != want_ids).any(axis=1))
    if rows.size:
        bad.append("%s ids: %d rows, first %d" % (what, rows.size, rows[0]))
    if got_dist is not None:
        n = int((gu.bits(got_dist) != gu.bits(want_dist)).sum())
        if n:
            bad.append("%s distance bits: %d differ" % (what, n))
    return bad


def _walk_differs(r, w, what):
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append(what + " candidate ids")
    if not np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])):
        bad.append(what + " distance bits (%d differ)" % int((gu.bits(r["cand_dist"]) != gu.bits(w["dists"])).sum()))
    if not np.array_equal(r["hops"], w["hops"]):
        bad.append(what + " hops")
    if not np.array_equal(r["dist_calc"], w["dist_calc"]):
        bad.append(what + " dist_calc")
    return bad


def _rerank_differs(orc, ix, base, q, cand, count, metric, what):
    """rerank_topk at k = the stride (every candidate's distance bits, every id column), column 0 against rerank, rerank against orc.rerank."""
    k = cand.shape[1]
    dist = tu.list_distances(orc, base, q, cand, count, metric)
    want_ids, want_dist = tu.expected_topk(dist, cand, count, k)
    ids, dd = ix.rerank_topk(q, cand, k, count)
    bad = _rows_differ(ids, dd, want_ids, want_dist, what)
    best = ix.rerank(q, cand, count)
    if not np.array_equal(ids[:, 0], best):
        bad.append(what + " column 0 against gbnns_rerank")
    some = count > 0
    nearest = np.full(len(count), NONE, np.uint32)
    nearest[some] = orc.rerank(q[some], cand[some], count[some], base, metric=metric, threads=8)
    if not np.array_equal(best, nearest):
        bad.append(what + " gbnns_rerank against getRealNearest (%d differ)" % int((best != nearest).sum()))
    return bad


def _report(name, census, failures):
    print(name, "census:", dict(sorted(census.items(), key=str)), "failures:", len(failures))
    assert not failures, failures


# ---- 1. the stand-alone re-rank over float rows --------------------------------------------------------------------------------------
def test_float_rerank_at_every_length(g, orc):
    """gbnns_rerank_topk at k = 70 and gbnns_rerank, both metrics, every length: the pair forms with DEEP = 8 and 24 (their 24-, 8- and
    4-loops, the remainder loop and the even lane's lone step in every combination, d = 4 where that step is the whole distance), and
    l2_ordered / negdot_ordered a lane per row with every tail and masked step.  Where the plan function names a pair form (d >= 8) the
    same on the equal-distance contest of that length, where only the order of the roundings tells the candidates apart."""
    off, nbr = ds.graph()
    cand, count = ds.candidates()
    census, failures = collections.Counter(), []
    for metric in (0, 1):
        for d in ds.DIMS:
            v = ds.vectors(d)
            form, deep, _ = ds.rerank_form(g, metric, d)
            census[(metric, g.rerank_plan(metric, d)[0], deep)] += 1
            ix = g.Index(v["base"], off, nbr, metric=metric)
            bad = _rerank_differs(orc, ix, v["base"], v["queries"], cand, count, metric, "full mantissa")
            ix.close()
            if form == "pairs" and d >= 8:
                base, gq, _ = (datagen.contest_dot if metric else datagen.contest_l2)(ds.rng_of(4, d, metric), 8, 128, d)
                ccand, ccount, qg = ds.contest_candidates(128, 8, d)
                ix = g.Index(base, *ds.graph(len(base)), metric=metric)
                bad += _rerank_differs(orc, ix, base, np.ascontiguousarray(gq[qg]), ccand, ccount, metric, "contest")
                ix.close()
            if bad:
                failures.append(((metric, d, form, deep, ds.rerank_trace(g, metric, d)[1]), bad))
    assert {k[1:] for k in census} == {("rerank_pair_kernel<0>", 8), ("rerank_pair_kernel<0>", 24), ("rerank_kernel<0>", 0),
                                      ("rerank_pair_kernel<1>", 8), ("rerank_kernel<1>", 0)}
    _report("float re-rank", census, failures)


# ---- 2. the stand-alone re-rank over byte rows ---------------------------------------------------------------------------------------
def test_byte_rerank_at_every_length(g, orc):
    """The same on a byte handle: uint8 rows against the widened table, every length, both metrics -- rerank_bytes_core (its 4-chunk-pair
    loop followed by leftover pairs and an odd chunk: d = 176; one pair alone: d = 32) and the lane-per-row form through ByteRow4.  Where the
    plan function names the chunk-pair form, the same on dim_sweep.byte_contest's equal-distance rows."""
    off, nbr = ds.graph()
    cand, count = ds.candidates()
    db_low = datagen.full_mantissa(ds.rng_of(5), ds.N, 8)
    census, failures = collections.Counter(), []
    for metric in (0, 1):
        for d in ds.DIMS:
            v = ds.byte_vectors(d)
            form, deep, _ = ds.rerank_form(g, metric, d, bytes=True)
            census[(metric, g.rerank_plan(metric, d, True)[0])] += 1
            ix = g.Index(v["base"], off, nbr, db_low=db_low, metric=metric)
            assert ix.is_bytes
            bad = _rerank_differs(orc, ix, v["base"].astype(np.float32), v["queries"], cand, count, metric, "bytes")
            ix.close()
            if form == "chunk_pairs":   # the pair form once more on the uint8 contest of the length
                cbase, gq = ds.byte_contest(d)
                ccand, ccount, qg = ds.contest_candidates(128, 8, d)
                ix = g.Index(cbase, *ds.graph(len(cbase)), db_low=db_low[:len(cbase)], metric=metric)
                bad += _rerank_differs(orc, ix, cbase.astype(np.float32), np.ascontiguousarray(gq[qg]), ccand, ccount, metric, "contest")
                ix.close()
            if bad:
                failures.append(((metric, d, form, ds.rerank_trace(g, metric, d, bytes=True)[1]), bad))
    assert {k[1] for k in census} == {"rerank_bytes_pair_kernel", "rerank_bytes_kernel<0>", "rerank_bytes_kernel<1>"}
    _report("byte re-rank", census, failures)


# ---- 3. the re-rank fused into the walk kernels ----------------------------------------------------------------------------------------
def test_fused_rerank_at_every_fused_length(g, orc):
    """MODE_LOWQ on a contest index -- 32 walked dimensions, the swept length as the original space -- at every length the plan function
    reports as fused: ef 64 (walk_hot), ef 200 on one wavefront (walk_hot_big) and on two (walk_coop), and ef 64 with the re-rank in its
    own launch.  The answers equal orc.rerank over the oracle's walk; candidate ids and their distance bits equal the walk's.  The walked
    table, graph, low-dimensional queries and entry points are shared by every length (four oracle walks in all); the original-space rows
    are the equal-distance contest of the length, the groups the graph's components."""
    groups, per = tu.GROUPS, tu.PER
    rng = ds.rng_of(6)
    db_low = datagen.full_mantissa(rng, groups * per, 32)
    off, nbr = datagen.contest_graph(rng, groups, per, 2, 30)
    qg = (np.arange(ds.NQ) // 8) % groups
    q_low = datagen.full_mantissa(rng, ds.NQ, 32)
    ent = (qg * per + rng.integers(0, per, size=ds.NQ)).astype(np.uint32)
    runs = ((64, -1, 0), (200, 0, 0), (200, 1, 0), (64, -1, g.FLAG_NO_FUSED_RERANK))
    census, failures = collections.Counter(), []
    for metric in (0, 1):
        walks = {ef: orc.walk(q_low, db_low, off, nbr, ef, entries=ent, metric=metric, threads=8) for ef in (64, 200)}
        for d in ds.DIMS:
            fused = ds.rerank_form(g, metric, d)[2]
            census[(metric, "fused" if fused else "own launch")] += 1
            if not fused:
                continue
            base, gq, _ = (datagen.contest_dot if metric else datagen.contest_l2)(ds.rng_of(7, d, metric), groups, per, d)
            queries = np.ascontiguousarray(gq[qg])
            ix = g.Index(base, off, nbr, db_low=db_low, metric=metric)
            ix.profile_enable(True)
            bad = []
            for ef, coop, flags in runs:
                w = walks[ef]
                want = orc.rerank(queries, w["ids"], w["count"], base, metric=metric, threads=8)
                ix.knob("coop", coop)
                ix.profile_read(reset=True)
                r = ix.search(queries, ef, mode=g.MODE_LOWQ, queries_low=q_low, entry_ids=ent, want=WANT, flags=flags)
                launched = ix.profile_read(reset=True)["walk_kernel"].split(" (")[0]
                census[(metric, ef, coop, flags, launched)] += 1
                what = "ef %d coop %d flags %d (%s)" % (ef, coop, flags, launched)
                bad += _walk_differs(r, w, what)
                if not np.array_equal(r["ids"], want):
                    bad.append(what + " answers (%d differ)" % int((r["ids"] != want).sum()))
            ix.close()
            if bad:
                failures.append(((metric, d, ds.rerank_trace(g, metric, d)[1]), bad))
        assert census[(metric, "fused")] >= 30 and census[(metric, "own launch")] >= 30
    _report("fused re-rank", census, failures)


# ---- 4. / 5. PLAIN walks over the swept rows -------------------------------------------------------------------------------------------
def _plain_walks(g, orc, efs, n_entries):
    off, nbr = ds.graph()
    census, failures = collections.Counter(), []
    for metric in (0, 1):
        for d in ds.DIMS:
            v = ds.vectors(d)
            ent = np.ascontiguousarray(v["ent"][:, :n_entries]) if n_entries > 1 else np.ascontiguousarray(v["ent"][:, 0])
            ix = g.Index(v["base"], off, nbr, metric=metric)
            ix.profile_enable(True)
            for kn, val in (("coop", 0), ("late_rows", 0), ("spec_min_nq", 0), ("spec_any_form", 0), ("spec_tail", 0)):
                ix.knob(kn, val)
            bad = []
            for ef in efs:
                planned = ds.walk_plan(g, metric, d, ds.N, ds.ELL_STRIDE, ef, n_entries)
                form = ds.walk_form(metric, d, planned)
                census[(metric, form)] += 1
                w = orc.walk(v["queries"], v["base"], off, nbr, ef, entries=ent, metric=metric, threads=8)
                ix.profile_read(reset=True)
                r = ix.search(v["queries"], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=WANT)
                launched = ix.profile_read(reset=True)["walk_kernel"].split(" (")[0]
                what = "ef %d %s %s" % (ef, form, ds.walk_trace(metric, d, form))
                bad += _walk_differs(r, w, what)
                if launched != planned:
                    bad.append("%s launched %s, planned %s" % (what, launched, planned))
            ix.close()
            if bad:
                failures.append(((metric, d), bad))
    return census, failures


def test_plain_walks_at_every_length(g, orc):
    """MODE_PLAIN with k = ef at ef 40 and 200, both metrics, every length: candidate ids in pop order, their distance bits, hops and
    dist_calc equal the oracle's, and the launched kernel is the one gbnns_debug_walk_plan names.  This runs the run-time-length instances a
    lane per row (l2_ordered / negdot_ordered at every remainder) and four lanes per row (l2_quad_rows: no masked batch, a masked batch of 1,
    2, 11 and 15 steps, ignored tails from d = 129 on), the compile-time pair forms, and at d < 4 under L2 the walk in which every distance
    is +0."""
    census, failures = _plain_walks(g, orc, (40, 200), 1)
    forms = {k[1] for k in census}
    assert {"lane", "quad"} <= forms and any(f.startswith("fixed") for f in forms), forms
    _report("PLAIN walks", census, failures)


def test_general_kernel_at_every_length(g, orc):
    """The same walks with two entry points per query at ef 40: the general kernel takes the whole batch and calls metric_dist with whatever
    length the index has."""
    census, failures = _plain_walks(g, orc, (40,), 2)
    assert {k[1] for k in census} == {"general"}
    _report("general kernel", census, failures)


# ---- 6. the exact scan ---------------------------------------------------------------------------------------------------------------
def test_exact_scan_at_every_length(g, orc):
    """exact_knn with k = 20, ids and distance bits, the matrix-core filter off ("knn_filter" 1 leaves shapes this small to the scan); where
    the library's own shape rule lets the filter take the shape under "knn_filter" = 2, once more with it.  The negative-dot form runs at
    d % 8 == 0 and is refused at every other length.  Every S class of knn_scan_kernel and the wide kernel are named across the sweep."""
    k = 20
    census, failures = collections.Counter(), []
    for metric in (0, 1):
        for d in ds.DIMS:
            v = ds.vectors(d)
            if metric == 1 and d % 8:
                with pytest.raises(g.GbnnsError) as e:
                    g.exact_knn(v["base"], v["queries"], k, metric, want_dist=True)
                assert e.value.code == 5 and "d % 8 == 0" in str(e.value), (d, str(e.value))
                census[(metric, "refused")] += 1
                continue
            want_ids, want_dist = orc.exact_knn(v["base"], v["queries"], k, metric, threads=8)
            name, _ = g.knn_plan(False, metric, ds.N, ds.NQ, d, k)
            census[(metric, name)] += 1
            ids, dd = g.exact_knn(v["base"], v["queries"], k, metric, want_dist=True)
            bad = _rows_differ(ids, dd, want_ids, want_dist, name)
            with ku.knobs(g, knn_filter=2):   # (the knob comes back behind an exception too)
                if ds.knn_filter_allowed(g, metric, d, k):
                    fname = g.knn_plan(False, metric, ds.N, ds.NQ, d, k)[0]
                    census[(metric, fname)] += 1
                    ids, dd = g.exact_knn(v["base"], v["queries"], k, metric, want_dist=True)
                    bad += _rows_differ(ids, dd, want_ids, want_dist, fname)
            if bad:
                failures.append(((metric, d, ds.trace_scan(d, name)), bad))
    names = {k[1] for k in census}
    for metric in (0, 1):
        assert {"knn_scan_kernel<%d, 8, 2, false>" % metric, "knn_scan_kernel<%d, 16, 2, false>" % metric,
                "knn_scan_kernel<%d, 32, 1, false>" % metric} <= names, names
    assert "knn_scan_wide_kernel<0, 16, false>" in names and "knn_scan_wide_kernel<1, 8, false>" in names, names
    assert any(n.startswith("knn_filter_kernel") for n in names), names
    _report("exact scan", census, failures)


# ---- 7. the device builder either side of its d <= 128 guard ---------------------------------------------------------------------------
def test_gd_pruning_either_side_of_its_length_guard(g):
    """gbnns_build_graph_gd_device against gbnns_build_graph_gd at d = 1 .. 8 and 124 .. 132 on full-mantissa rows, 40-NN lists from
    exact_knn, M = 12: equal graphs; the device decides up to d = 128 (the node's vector fits pi_s[132]) and everything is the host's above."""
    n = 1024
    census, failures = collections.Counter(), []
    for d in ds.GD_DIMS:
        x = np.ascontiguousarray(ds.vectors(d)["base"][:n])
        knn = g.exact_knn(x, x, 40, self_offset=0)
        koff, knbr = datagen.dense_to_csr(knn)
        bad = []
        for rev in (True, False):
            w_off, w_nbr = g.build_graph_gd(koff, knbr, x, 12, reverse=rev, threads=8)
            off, nbr, on_host = g.build_graph_gd_device(koff, knbr, x, 12, reverse=rev, threads=8)
            census[(d, rev)] = on_host
            if not (np.array_equal(off, w_off) and np.array_equal(nbr, w_nbr)):
                bad.append("reverse %s: the graphs differ" % rev)
            if (on_host != n) if d > ds.GD_DEVICE_MAX_DIM else (on_host >= n // 2):
                bad.append("reverse %s: %d of %d nodes on the host" % (rev, on_host, n))
        if bad:
            failures.append((d, bad))
    _report("GD pruning (nodes finished on the host)", census, failures)
