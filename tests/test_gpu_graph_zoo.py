"""Topology as an axis, on the device (run with -m gpu on an MI355X): the census of tests/walk_instances.py, the feature instances (tags,
bridge, half rows, byte rows, byte walk, byte queries, top-k) and the general kernel's several entry points on the graphs of
tests/graph_zoo.py -- rows without neighbours, full rows, repeated ids, self loops, components smaller than the beam, hops that find
nothing fresh, paths that find exactly one id a hop, small components whose rows repeat an id.  tests/test_graph_zoo_cpu.py proves on the CPU that the graphs hold all that and that
the oracle is a valid expectation on them (the compiled reference agrees byte for byte).  Every output is compared with the CPU oracle's,
every launched kernel with its planned name; nothing takes a tolerance.
"""
import time

import numpy as np
import pytest

import bridge_util as bru
import golden_util as gu
import graph_zoo as gz
import half_rows_util as hu
import tag_util as tg
import topk_util as tu
import walk_instances as wi
from gbnns_dim_red_amd import bridge_graph, cut_graph

pytestmark = pytest.mark.gpu

NONE = gz.NONE
WANT = ("hops", "dist_calc", "cand", "cand_dist", "edges")
OUTPUTS = ("ids",) + WANT


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _launched(p):
    return p["walk_kernel"].split(" (")[0]


def _against_walk(r, w, want=None):
    """Names of the outputs of r that differ from the oracle walk w: candidate ids in pop order, distance bit patterns, hops, dist_calc, the
    padding from column count on (0xFFFFFFFF / +inf) and -- want given -- the answers."""
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append("candidate ids (%d rows)" % int((r["cand"] != w["ids"]).any(axis=1).sum()))
    if not np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])):
        bad.append("distance bits (%d differ)" % int((gu.bits(r["cand_dist"]) != gu.bits(w["dists"])).sum()))
    if not np.array_equal(r["hops"], w["hops"]):
        bad.append("hops (%d differ)" % int((r["hops"] != w["hops"]).sum()))
    if not np.array_equal(r["dist_calc"], w["dist_calc"]):
        bad.append("dist_calc (%d differ)" % int((r["dist_calc"] != w["dist_calc"]).sum()))
    past = np.arange(r["cand"].shape[1])[None, :] >= np.asarray(w["count"])[:, None]
    if not ((r["cand"][past] == NONE).all() and np.isposinf(r["cand_dist"][past]).all() and (r["cand"][~past] != NONE).all()):
        bad.append("padding past count")
    if want is not None and not np.array_equal(r["ids"], want):
        bad.append("answers (%d differ)" % int((r["ids"] != want).sum()))
    return bad


def _short_edges(r, w, deg, ef, hops_bound=None):
    """out_edges against graph_zoo.short_list_edges: where the list never fills, the kept degrees of the rows it returns."""
    exp, mask = gz.short_list_edges(deg, w, ef, hops_bound)
    if np.array_equal(r["edges"][mask], exp[mask]):
        return []
    return ["edges (%d of %d short lists differ from the kept degrees of their rows)" % (int((r["edges"][mask] != exp[mask]).sum()), int(mask.sum()))]


def _same_bytes(a, b, names=OUTPUTS):
    return [n for n in names if np.asarray(a[n]).tobytes() != np.asarray(b[n]).tobytes()]


# ---- A. the census on every topology -------------------------------------------------------------------------------------------------------
def _census_search(g, ix, v, ent, case, hash_capacity):
    """test_gpu_walk_instances._search with the zoo's entry ids and the edge counter."""
    for name, val in case.knobs.items():
        ix.knob(name, val)
    kw = dict(aux=True, llf=True, hops_bound=50) if case.aux else {}
    ix.profile_read(reset=True)
    r = ix.search(v["queries"], case.ef, mode=g.MODE_LOWQ, queries_low=v["q_low"], entry_ids=ent, want=WANT, flags=case.flags,
                  hash_capacity=hash_capacity, **kw)
    return r, ix.profile_read(reset=True)


@pytest.mark.parametrize("topology", gz.TOPOLOGIES)
@pytest.mark.parametrize("metric,dim", wi.SETS, ids=["m%d_d%d" % s for s in wi.SETS])
def test_every_walk_instance_on_every_topology(g, orc, metric, dim, topology):
    """Every census case of the set with the graph replaced by the zoo's (same vectors, knobs, flags, hash_capacity; the zoo's entry ids;
    a case with an auxiliary graph uses the one that repeats ids of the main rows): candidate ids in pop order, distance bits, hops,
    dist_calc and the padding past count equal the oracle walk, the answers getRealNearest over it, walk_kernel the planned name.
    hash_capacity 128: at least the queries whose walk outgrows 128 ids are handed over, the planned retry instance runs where there are
    any and finishes at least half of them, every output equals the hash_capacity 0 run.  out_edges equals degree x hops where
    graph_zoo.expected_edges covers the query, the kept degrees of the returned rows where the list never fills (graph_zoo.short_list_edges;
    on knots that tells raw slots from kept ones), and is byte-identical across the cases of one (graph, auxiliary graph, beam)."""
    t0 = time.time()
    cases = [c for c in wi.CASES if (c.metric, c.dim) == (metric, dim)]
    failures, ran, searches, edges_of = [], 0, 0, {}
    for key in sorted({c.graph_key for c in cases}):
        group = [c for c in cases if c.graph_key == key]
        n, cap = key[2], wi.ELL_STRIDE[key[3]]
        v = wi.vectors(metric, dim, n)
        off, nbr, ent = gz.case_graph(group[0], topology)
        ix = g.Index(v["base"], off, nbr, db_low=v["db_low"], metric=metric)
        if any(c.aux for c in group):
            ix.set_aux_graph(*gz.zoo_aux(topology, n, cap, gz.seed_of(group[0])))
        ix.profile_enable(True)
        for c in group:
            w, want = gz.oracle_walk(orc, c, topology)
            r, p = _census_search(g, ix, v, ent, c, c.hash_capacity)
            ran, searches = ran + 1, searches + 1
            bad = _against_walk(r, w, want)
            if _launched(p) != c.first:
                bad.append("first pass launched %s" % _launched(p))
            if c.hash_capacity:
                over = gz.over(orc, c, topology)
                handed, general = int(p["retry_queries"]), int(p["retry_general_queries"])
                if handed < over:
                    bad.append("%d queries outgrow the visited set, %d handed over" % (over, handed))
                if over and p["retry_kernel"] != c.retry:
                    bad.append("retry pass launched '%s'" % p["retry_kernel"])
                if 2 * (handed - general) < over:
                    bad.append("retry pass finished %d of %d handed over (%d outgrow the set)" % (handed - general, handed, over))
                r0, _ = _census_search(g, ix, v, ent, c, 0)
                searches += 1
                bad += ["%s differs from hash_capacity 0" % name for name in _same_bytes(r, r0)]
            elif p["retry_queries"] < p["retry_general_queries"]:
                bad.append("counts: %d handed over, %d to the general kernel" % (p["retry_queries"], p["retry_general_queries"]))
            exp, mask = gz.expected_edges(topology, n, cap, gz.seed_of(c), ent, w["hops"], aux=bool(c.aux))
            if not np.array_equal(r["edges"][mask], exp[mask]):
                bad.append("edges (%d of %d differ from degree x hops)" % (int((r["edges"][mask] != exp[mask]).sum()), int(mask.sum())))
            if not c.aux:
                bad += _short_edges(r, w, gz.kept_degrees(topology, n, cap, gz.seed_of(c)), c.ef)
            first = edges_of.setdefault(key + (c.aux, c.ef), (tuple(c), r["edges"]))
            if first[1].tobytes() != r["edges"].tobytes():
                bad.append("edges differ from case %s in %d queries" % (first[0], int((first[1] != r["edges"]).sum())))
            if bad:
                failures.append((tuple(c), bad))
        ix.close()
    print("zoo census", topology, (metric, dim), "cases", ran, "searches", searches, "failures", len(failures), "%.2f s" % (time.time() - t0))
    print(*failures, sep="\n")
    assert ran == len(cases)
    assert not failures, failures


# ---- B. the feature instances ----------------------------------------------------------------------------------------------------------------
B_KEY, B_N, B_DLOW, B_BEAMS = (0, 32), 3000, 32, (8, 64, 100, 200)


def _tag_expected(orc, build, off, nbr, v, T, Q, ent, ef):
    """tag_util.expected / bridge_util.expected over the DE-DUPLICATED rows (build: cut_graph / bridge_graph), plus the expanded rows'
    answer check data: dict(ids, dists, count, hops, dist_calc, want)."""
    c = dict(off=off, nbr=nbr, db_low=v["db_low"], q_low=v["q_low"], queries=v["queries"], base=v["base"], T=T, Q=Q, ent=ent)
    return (tg.expected if build is cut_graph else bru.expected)(orc, c, ef, 0)


def _topk_bad(orc, w, base, queries, k_values, what, search):
    """gbnns_search_topk at every k of k_values over the walk w: rows equal tu.expected_topk on the oracle's scalar distances, columns
    past count hold 0xFFFFFFFF / +inf, column 0 equals out_ids."""
    bad = []
    dist = tu.list_distances(orc, base, queries, w["ids"], w["count"], 0)
    for k in k_values:
        rk = search(k)
        want_ids, want_dist = tu.expected_topk(dist, w["ids"], w["count"], k)
        if not np.array_equal(rk["top_ids"], want_ids):
            bad.append("%s top-%d ids (%d rows)" % (what, k, int((rk["top_ids"] != want_ids).any(axis=1).sum())))
        if not np.array_equal(gu.bits(rk["top_dist"]), gu.bits(want_dist)):
            bad.append("%s top-%d distance bits" % (what, k))
        past = np.arange(k)[None, :] >= np.minimum(w["count"], k)[:, None]
        if not ((rk["top_ids"][past] == NONE).all() and np.isposinf(rk["top_dist"][past]).all()):
            bad.append("%s top-%d padding" % (what, k))
        if not np.array_equal(rk["top_ids"][:, 0], rk["ids"]):
            bad.append("%s top-%d column 0 is not out_ids" % (what, k))
        bad += ["%s top-%d: %s" % (what, k, b) for b in _against_walk(rk, w)]
    return bad


@pytest.mark.parametrize("topology", gz.TOPOLOGIES)
def test_feature_instances_on_every_topology(g, orc, topology):
    """cap 32 and 64, L2, walked rows of 32 floats, beams 8 / 64 / 100 / 200: the tagged and the bridged first pass (three query words in
    one batch, two queries entering at a row their word does not allow; expected: the oracle on cut_graph / bridge_graph of the
    de-duplicated rows), half rows (the oracle on float32(float16(db_low))), a byte handle's fused first pass, the byte-row PLAIN walk and
    the integer byte-query walk (the oracle on the widened bytes), gbnns_search_topk with k = 5 and k = ef on the float and the byte
    handle.  Every output byte, the launched name, the bad-entry rows, the top-k padding; a bridged call with every row allowed equals the
    untagged call, edges included."""
    t0 = time.time()
    v = wi.vectors(0, B_DLOW, B_N)
    bv = gz.byte_vectors(B_N)
    T, Q = tg.row_tags(B_N), tg.query_tags(gz.NQ)
    failures, searches = [], 0
    for cap in (32, 64):
        off, nbr = gz.zoo(topology, B_N, cap, B_KEY)
        doff, dnbr = gz.zoo_dedup(topology, B_N, cap, B_KEY)
        ent = gz.entries(topology, B_N, cap, B_KEY)
        tent = gz.tagged_entries(ent, T, Q)
        ok = tg.entry_ok(T, Q, tent)
        assert not ok[list(gz.DISALLOWED)].any() and ok.sum() == gz.NQ - len(gz.DISALLOWED)
        R = hu.rounded(v["db_low"])
        deg = gz.kept_degrees(topology, B_N, cap, B_KEY)
        ix = g.Index(v["base"], off, nbr, db_low=v["db_low"], metric=0)
        ix.enable_half_rows()
        ix.profile_enable(True)
        bx = g.Index(bv["base"], off, nbr, db_low=v["db_low"], metric=0)
        assert bx.is_bytes
        bx.profile_enable(True)
        for h in (ix, bx):
            for name, val in (("coop", 0), ("late_rows", 0), ("spec_min_nq", 0), ("spec_any_form", 0), ("spec_tail", 0)):
                h.knob(name, val)
        low = dict(mode=g.MODE_LOWQ, queries_low=v["q_low"], want=WANT)
        for ef in B_BEAMS:
            def note(what, bad):
                if bad:
                    failures.append((topology, cap, ef, what, bad))

            def run(h, queries, planned, **kw):
                h.profile_read(reset=True)
                r = h.search(queries, ef, **kw)
                p = h.profile_read(reset=True)
                return r, ([] if planned is None or _launched(p) == planned else ["launched %s, planned %s" % (_launched(p), planned)])

            # tagged and bridged first pass
            ix.set_tags(T)
            for what, build, flags, planned in (("tagged", cut_graph, 0, tg.tag_kernel(0, B_DLOW, ef, cap == 32)),
                                                ("bridged", bridge_graph, g.FLAG_TAG_BRIDGE, bru.bridge_kernel(0, B_DLOW, ef))):
                w = _tag_expected(orc, build, doff, dnbr, v, T, Q, tent, ef)
                r, bad = run(ix, v["queries"], planned, entry_ids=tent, query_tags=Q, flags=flags, **low)
                searches += 1
                bad += _against_walk(r, w, w["want"])
                rows = list(gz.DISALLOWED)
                if not ((r["ids"][rows] == NONE).all() and (r["cand"][rows] == NONE).all() and np.isposinf(r["cand_dist"][rows]).all()
                        and (r["hops"][rows] == 0).all() and (r["dist_calc"][rows] == 0).all() and (r["edges"][rows] == 0).all()):
                    bad.append("bad-entry rows")
                note(what, bad)
            ix.set_tags(np.full(B_N, tg.ALL, np.uint32))
            plain, _ = run(ix, v["queries"], None, entry_ids=ent, **low)
            allowed, _ = run(ix, v["queries"], None, entry_ids=ent, query_tags=np.full(gz.NQ, tg.ALL, np.uint32), flags=g.FLAG_TAG_BRIDGE, **low)
            searches += 2
            note("bridged with every row allowed against the untagged call", _same_bytes(allowed, plain))
            # the untagged float handle and its top-k rows
            w = orc.walk(v["q_low"], v["db_low"], off, nbr, ef, entries=ent, threads=8)
            note("untagged", _against_walk(plain, w, orc.rerank(v["queries"], w["ids"], w["count"], v["base"], threads=8)) + _short_edges(plain, w, deg, ef))
            note("top-k", _topk_bad(orc, w, v["base"], v["queries"], (5, ef), "float handle",
                                    lambda k: ix.search(v["queries"], ef, entry_ids=ent, top_k=k, **low)))
            # half rows
            wh = orc.walk(v["q_low"], R, off, nbr, ef, entries=ent, threads=8)
            r, bad = run(ix, v["queries"], hu.half_kernel(0, B_DLOW, ef, cap == 32), entry_ids=ent, flags=g.FLAG_HALF_ROWS, **low)
            note("half rows", bad + _against_walk(r, wh, orc.rerank(v["queries"], wh["ids"], wh["count"], v["base"], threads=8)) + _short_edges(r, wh, deg, ef))
            # the byte handle: fused first pass, top-k, byte-row PLAIN walk, integer byte-query walk
            r, bad = run(bx, bv["queries"], g.byte_plan(0, B_DLOW, B_N, cap, ef)[0], entry_ids=ent, **low)
            note("byte handle", bad + _against_walk(r, w, orc.rerank(bv["queries"], w["ids"], w["count"], bv["wide"], threads=8)) + _short_edges(r, w, deg, ef))
            note("top-k", _topk_bad(orc, w, bv["wide"], bv["queries"], (5, ef), "byte handle",
                                    lambda k: bx.search(bv["queries"], ef, entry_ids=ent, top_k=k, **low)))
            plain_kw = dict(mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=WANT, flags=g.FLAG_BYTE_WALK)
            wb = orc.walk(bv["queries"], bv["wide"], off, nbr, ef, k=ef, entries=ent, threads=8)
            r, bad = run(bx, bv["queries"], g.byte_walk_plan(0, 128, B_N, cap, ef), **plain_kw)
            note("byte walk", bad + _against_walk(r, wb, np.where(wb["count"] > 0, wb["ids"][:, 0], NONE).astype(np.uint32)) + _short_edges(r, wb, deg, ef))
            bx.knob("byte_query_int", 7)
            wq = orc.walk(bv["queries_u8_wide"], bv["wide"], off, nbr, ef, k=ef, entries=ent, threads=8)
            r, bad = run(bx, bv["queries_u8"], g.byte_query_plan(0, 128, B_N, cap, ef), **plain_kw)
            note("byte queries", bad + _against_walk(r, wq, np.where(wq["count"] > 0, wq["ids"][:, 0], NONE).astype(np.uint32)) + _short_edges(r, wq, deg, ef))
            searches += 8   # half rows, byte handle, byte walk, byte queries, four top-k calls
        ix.close()
        bx.close()
    print("zoo features", topology, "searches", searches, "failures", len(failures), "%.2f s" % (time.time() - t0))
    print(*failures, sep="\n")
    assert not failures, failures


# ---- C. entry points and the general kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", ("ragged", "islands", "star", "knots"))
def test_two_entry_points_on_the_general_kernel(g, orc, topology):
    """[e, e], [e, e's first neighbour] and [a dead end, e] at cap 32 and 96, beams 1 / 8 / 64 / 200: alone, with the auxiliary graph that
    repeats ids of the main rows under AUX_GRAPH | LLF (hops_bound 50) and under AUX_GRAPH alone with hops_bound 3; MODE_LOWQ and MODE_PLAIN
    (k = ef), and once more with every hop reading both rows (no LLF, hops_bound 50).  The profile names walk_general_kernel.  The
    single-entry searches run with GBNNS_FLAG_WIDE_INDEX as well; their out_edges on short lists are the kept degrees of the returned rows,
    the auxiliary rows' included where every hop reads them."""
    t0 = time.time()
    v = wi.vectors(0, 32, B_N)
    failures, searches = [], 0
    for cap in (32, 96):
        off, nbr = gz.zoo(topology, B_N, cap, B_KEY)
        aux = gz.zoo_aux(topology, B_N, cap, B_KEY)
        ix = g.Index(v["base"], off, nbr, db_low=v["db_low"], metric=0)
        ix.set_aux_graph(*aux)
        ix.profile_enable(True)
        single = gz.entries(topology, B_N, cap, B_KEY)
        for ef in (1, 8, 64, 200):
            for kind in gz.ENTRY_KINDS + ("wide",):
                ent = single if kind == "wide" else gz.two_entries(topology, B_N, cap, B_KEY, kind)
                flags = g.FLAG_WIDE_INDEX if kind == "wide" else 0
                for use_aux, llf, hb in gz.ENTRY_RUNS:
                    okw = dict(aux=aux, llf=llf, hops_bound=hb) if use_aux else {}
                    skw = dict(aux=True, llf=llf, hops_bound=hb) if use_aux else {}
                    for mode in ("lowq", "plain"):
                        ix.profile_read(reset=True)
                        if mode == "lowq":
                            w = orc.walk(v["q_low"], v["db_low"], off, nbr, ef, entries=ent, threads=8, **okw)
                            want = orc.rerank(v["queries"], w["ids"], w["count"], v["base"], threads=8)
                            r = ix.search(v["queries"], ef, mode=g.MODE_LOWQ, queries_low=v["q_low"], entry_ids=ent, want=WANT, flags=flags, **skw)
                        else:
                            w = orc.walk(v["queries"], v["base"], off, nbr, ef, k=ef, entries=ent, threads=8, **okw)
                            want = np.where(w["count"] > 0, w["ids"][:, 0], NONE).astype(np.uint32)
                            r = ix.search(v["queries"], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=WANT, flags=flags, **skw)
                        p = ix.profile_read(reset=True)
                        searches += 1
                        bad = _against_walk(r, w, want)
                        if kind != "wide" and _launched(p) != "walk_general_kernel":
                            bad.append("launched %s" % _launched(p))
                        if kind == "wide" and not (use_aux and llf):   # one entry point: a short list's edges are its rows' kept degrees
                            bad += _short_edges(r, w, gz.kept_degrees(topology, B_N, cap, B_KEY, aux=use_aux), ef, hb if use_aux else None)
                        if bad:
                            failures.append((topology, cap, ef, kind, use_aux, llf, hb, mode, bad))
        ix.close()
    print("zoo entry points", topology, "searches", searches, "failures", len(failures), "%.2f s" % (time.time() - t0))
    print(*failures, sep="\n")
    assert not failures, failures
