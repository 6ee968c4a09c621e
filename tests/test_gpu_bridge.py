"""gbnns_search_tagged with GBNNS_FLAG_TAG_BRIDGE on an MI355X (run with -m gpu).  The contract: a disallowed neighbour is looked through --
the allowed entries of its own row take its place, one level deep -- and a bridged tagged search of query i is the reference's search on that
graph G''(i).  Every expected value below is the CPU oracle's on gbnns_dim_red_amd.bridge_graph's CSR, one oracle call per distinct value of
Q -- candidate ids in pop order, the bit patterns of their distances, count, hops, dist_calc, answers -- and nothing takes a tolerance.
n = 2 048 rows and 96 queries throughout.
"""
import numpy as np
import pytest

import bridge_util as bu
import datagen
import golden_util as gu
import locality_order_util as lo
import tag_util as tg
import topk_util as tu

pytestmark = pytest.mark.gpu

WANT = ("hops", "dist_calc", "cand", "cand_dist")


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


_EXPECTED = {}


def _expected(orc, key, c, ef, metric, **kw):
    k = (key, ef, tuple(sorted((a, repr(b) if not isinstance(b, np.ndarray) else b.tobytes()) for a, b in kw.items() if a != "aux")), "aux" in kw)
    if k not in _EXPECTED:
        _EXPECTED[k] = bu.expected(orc, c, ef, metric, **kw)
    return _EXPECTED[k]


def _against(r, w, answers=True):
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append("candidate ids (%d rows)" % tg.rows_that_differ(r["cand"], w["ids"]))
    if not np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])):
        bad.append("distance bits (%d differ)" % int((gu.bits(r["cand_dist"]) != gu.bits(w["dists"])).sum()))
    if not np.array_equal((r["cand"] != tg.NONE).sum(axis=1), w["count"]):
        bad.append("count")
    if not np.array_equal(r["hops"], w["hops"]):
        bad.append("hops (%d differ)" % int((r["hops"] != w["hops"]).sum()))
    if not np.array_equal(r["dist_calc"], w["dist_calc"]):
        bad.append("dist_calc (%d differ)" % int((r["dist_calc"] != w["dist_calc"]).sum()))
    if answers and not np.array_equal(r["ids"], w["want"]):
        bad.append("answers (%d differ)" % int((r["ids"] != w["want"]).sum()))
    return bad


def _bridged(g, ix, c, ef, flags=0, **kw):
    """One profiled bridged LOWQ search -> (results, name of the first-pass kernel, profile)."""
    ix.profile_read(reset=True)
    kw.setdefault("entry_ids", c["ent"])
    kw.setdefault("query_tags", c["Q"])
    kw.setdefault("want", WANT)
    r = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], flags=flags | g.FLAG_TAG_BRIDGE, **kw)
    p = ix.profile_read(reset=True)
    return r, p["walk_kernel"].split(" (")[0], p


def _index(g, c, metric, profile=True, **kw):
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric, **kw)
    ix.set_tags(c["T"])
    if profile:
        ix.profile_enable(True)
    return ix


def _instances(g, orc, key, c, metric, dlow, beams=tg.BEAMS, flags=0, general=False):
    """Every beam on one index -> the list of failures."""
    ix = _index(g, c, metric)
    failures = []
    for ef in beams:
        w = _expected(orc, key, c, ef, metric)
        r, launched, p = _bridged(g, ix, c, ef, flags=flags)
        bad = _against(r, w)
        planned = "walk_general_kernel" if general else bu.bridge_kernel(metric, dlow, ef)
        if launched != planned:
            bad.append("launched %s, expected %s" % (launched, planned))
        if p["retry_kernel"]:
            bad.append("a retry pass ran: %s" % p["retry_kernel"])
        # the instance, not the fall-back, is what was compared
        if planned != "walk_general_kernel" and p["general_queries"] * 8 > len(c["Q"]):
            bad.append("%d queries went to the general kernel" % p["general_queries"])
        print("bridged", key, ef, launched, "general_queries", p["general_queries"])
        # once more with the batch walked in locality order (locality_order_util.in_order): same kernel, a valid order, the same bytes
        (ro, lo_launched, po), in_order = lo.in_order(ix, c["q_low"], lambda: _bridged(g, ix, c, ef, flags=flags))
        in_order += lo.same_bytes(ro, r, ("ids",) + WANT)
        if (lo_launched, po["retry_kernel"]) != (launched, p["retry_kernel"]):
            in_order.append("launched %s / '%s'" % (lo_launched, po["retry_kernel"]))
        bad += ["in order: " + b for b in in_order]
        if bad:
            failures.append((key, ef, bad))
    ix.close()
    return failures


# ---- 1. every bridge instance and the general kernel, by name and bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("metric,d,dlow", tg.SHAPES, ids=["m%d_d%d_low%d" % s for s in tg.SHAPES])
def test_bridged_walk_on_the_contest_indexes(g, orc, metric, d, dlow):
    """One-pass adjacency rows, three values of Q (about 1/2, 1/8 and all rows) in one batch: the one- and two-register bridge instances
    (ef 8, 64; 100), the general kernel's bridged instance at ef 200 and over 576-byte rows."""
    c = tg.contest(metric, d, dlow)
    failures = _instances(g, orc, ("contest", metric, d, dlow), c, metric, dlow)
    assert not failures, failures


@pytest.mark.parametrize("metric,dlow", tg.TWO_PASS_SHAPES, ids=["m%d_low%d" % s for s in tg.TWO_PASS_SHAPES])
def test_bridged_walk_on_two_pass_adjacency_rows(g, orc, metric, dlow):
    """Adjacency rows of 33 .. 48 slots: a looked-through row takes two passes of the pair form, a bridged row many refills of the staging area."""
    c = tg.two_pass(metric, dlow)
    failures = _instances(g, orc, ("two_pass", metric, dlow), c, metric, dlow)
    assert not failures, failures


# ---- 2. the flag matters --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d,dlow", tg.SHAPES, ids=["m%d_d%d_low%d" % s for s in tg.SHAPES])
def test_the_flag_matters(g, orc, metric, d, dlow):
    """ef 8: for at least 60 of the 64 restricted queries the walk on G'' differs from the walk on the cut graph in answer or hop count, the
    flagged call returns the former and the unflagged call the latter."""
    c = tg.contest(metric, d, dlow)
    w = _expected(orc, ("contest", metric, d, dlow), c, 8, metric)
    cut = tg.expected(orc, c, 8, metric)
    sel = (c["Q"] & 0xFF) != 0xFF
    assert sel.sum() == 64 and bu.queries_that_differ(w, cut, sel) >= 60, bu.queries_that_differ(w, cut, sel)
    ix = _index(g, c, metric)
    r, _, _ = _bridged(g, ix, c, 8)
    assert not _against(r, w), _against(r, w)
    plain = ix.search(c["queries"], 8, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], query_tags=c["Q"], want=WANT)
    assert not _against(plain, cut), _against(plain, cut)
    ix.close()


# ---- 3. modes, top-k, buffers, flags ---------------------------------------------------------------------------------------------------------
def test_net_and_plain_modes(g, orc):
    metric, d, dlow, ef = 0, 128, 32, 64
    c = tg.contest(metric, d, dlow)
    key = ("contest", metric, d, dlow)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"], metric=metric)
    ix.set_tags(c["T"])
    kw = dict(entry_ids=c["ent"], query_tags=c["Q"], flags=g.FLAG_TAG_BRIDGE)
    r = ix.search(c["queries"], ef, mode=g.MODE_NET, want=WANT + ("q_low",), **kw)
    q_low = orc.project(c["net"], c["queries"], threads=4)
    assert np.array_equal(gu.bits(r["q_low"]), gu.bits(q_low))
    assert not _against(r, _expected(orc, key, c, ef, metric, q_low=q_low))
    # PLAIN: the walk runs in the original space, whose rows (128 floats) have no bridge instance -- the general kernel
    r = ix.search(c["queries"], ef, mode=g.MODE_PLAIN, k=ef, want=WANT, **kw)
    w = _expected(orc, key + ("plain",), c, ef, metric, q_low=c["queries"], db=c["base"], rerank=False)
    assert not _against(r, w, answers=False), _against(r, w, answers=False)
    ix.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_topk_and_bad_entries(g, orc, where):
    """top_k = 3 from HOST and DEVICE buffers; Q == 0, an entry row the query may not see and an entry id >= n give the bad-entry row, their
    neighbours in the batch the oracle's rows -- on a bridge instance and on the general kernel."""
    import torch
    metric, d, dlow = 0, 128, 32
    c = tg.contest(metric, d, dlow)
    Q, ent = c["Q"].copy(), c["ent"].copy()
    Q[[3, 40]] = 0
    banned = np.flatnonzero((c["T"] & 0x01) == 0)
    ent[[10, 55]] = banned[[5, 300]]            # queries 10 and 55 have Q == 0x01
    ent[[20, 77]] = [tg.N, 0xFFFFFFF0]
    bad_rows = np.array([3, 40, 10, 55, 20, 77])
    assert not tg.entry_ok(c["T"], Q, ent)[bad_rows].any() and tg.entry_ok(c["T"], Q, ent).sum() == len(Q) - 6
    ix = _index(g, c, metric, profile=False)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    memo = {}
    for ef, flags in ((64, 0), (64, g.FLAG_WIDE_INDEX)):
        w = _expected(orc, ("contest", metric, d, dlow), c, ef, metric, Q=Q, ent=ent)
        flags |= g.FLAG_TAG_BRIDGE
        if where == "host":
            r = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=ent, query_tags=Q, want=WANT + ("edges",), flags=flags,
                          top_k=3)
        else:
            r = ix.search(t(c["queries"]), ef, mode=g.MODE_LOWQ, queries_low=t(c["q_low"]), entry_ids=t(ent.view(np.int32)),
                          query_tags=t(Q.view(np.int32)), want=WANT + ("edges",), flags=flags, top_k=3)
            torch.cuda.synchronize()
            r = {k: v.cpu().numpy() for k, v in r.items()}
            for name in ("ids", "cand", "top_ids"):
                r[name] = r[name].view(np.uint32)
        assert not _against(r, w), (ef, flags, _against(r, w))
        assert (r["edges"][bad_rows] == 0).all() and (r["top_ids"][bad_rows] == tg.NONE).all() and np.isinf(r["top_dist"][bad_rows]).all()
        assert (r["cand"][bad_rows] == tg.NONE).all() and (r["ids"][bad_rows] == tg.NONE).all()
        count = (r["cand"] != tg.NONE).sum(axis=1)
        dist = tu.list_distances(orc, c["base"], c["queries"], r["cand"], count, metric, memo)
        want_ids, want_dist = tu.expected_topk(dist, r["cand"], count, 3)
        assert np.array_equal(r["top_ids"], want_ids) and np.array_equal(gu.bits(r["top_dist"]), gu.bits(want_dist))
    ix.close()


def test_unfused_rerank_and_all_allowed_identity(g, orc):
    """GBNNS_FLAG_NO_FUSED_RERANK changes nothing; with every row allowed (T and Q all ones) every output of a bridged call equals the untagged
    search's bit for bit, edges included -- on a bridge instance (ef 8, 64, 100) and on the general kernel (ef 200)."""
    metric, d, dlow = 0, 128, 32
    c = tg.contest(metric, d, dlow)
    ix = _index(g, c, metric)
    r, _, _ = _bridged(g, ix, c, 64, flags=g.FLAG_NO_FUSED_RERANK)
    assert not _against(r, _expected(orc, ("contest", metric, d, dlow), c, 64, metric))
    ix.set_tags(np.full(tg.N, tg.ALL, np.uint32))
    q_all = np.full(len(c["Q"]), tg.ALL, np.uint32)
    for ef in (8, 64, 100, 200):
        kw = dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=WANT + ("edges",), top_k=5)
        plain = ix.search(c["queries"], ef, **kw)
        bridged = ix.search(c["queries"], ef, query_tags=q_all, flags=g.FLAG_TAG_BRIDGE, **kw)
        assert set(plain) == set(bridged)
        for name in plain:
            assert bridged[name].tobytes() == plain[name].tobytes(), (ef, name)
    ix.close()


def test_bridged_batches_in_flight(g, orc):
    """Three bridged batches with GBNNS_FLAG_DEFER_JOIN (depth 3) and different Q arrays on torch tensors, twice round: every call's outputs
    equal the synchronous HOST result of its batch, which equals the oracle on G''."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    metric, d, dlow, ef = 0, 128, 32, 64
    c = tg.contest(metric, d, dlow)
    rng = tu.rng_of(9900)
    pools = [np.arange(grp * tu.PER, (grp + 1) * tu.PER) for grp in c["qg"]]
    batches = []
    for b in range(3):
        Q = np.roll(c["Q"], b)
        batches.append((Q, tg.allowed_entries(rng, c["T"], Q, pools)))
    ix = g.Index(t(c["base"]), c["off"], c["nbr"], db_low=t(c["db_low"]), metric=metric)
    ix.set_tags(c["T"])
    kw = dict(mode=g.MODE_LOWQ, want=WANT)
    host = [ix.search(c["queries"], ef, queries_low=c["q_low"], entry_ids=ent, query_tags=Q, flags=g.FLAG_TAG_BRIDGE, **kw) for Q, ent in batches]
    assert len({h["cand"].tobytes() for h in host}) == 3   # the batches are distinct
    for (Q, ent), h in zip(batches, host):
        assert not _against(h, bu.expected(orc, c, ef, metric, Q=Q, ent=ent))
    q, ql = t(c["queries"]), t(c["q_low"])
    dev_in = [(t(Q.view(np.int32)), t(ent.view(np.int32))) for Q, ent in batches]
    outs = []
    for call in range(6):
        Q, ent = dev_in[call % 3]
        outs.append(ix.search(q, ef, queries_low=ql, entry_ids=ent, query_tags=Q, out={}, flags=g.FLAG_DEFER_JOIN | g.FLAG_TAG_BRIDGE, defer_depth=3, **kw))
    ix.join()
    torch.cuda.synchronize()
    for call, r in enumerate(outs):
        h = host[call % 3]
        for name in ("ids",) + WANT:
            assert r[name].cpu().numpy().tobytes() == h[name].tobytes(), (call, name)
    ix.close()


# ---- 4. the general kernel's domain ---------------------------------------------------------------------------------------------------------
def test_general_kernel_domain(g, orc):
    metric, d, dlow, ef = 0, 128, 32, 64
    c = tg.contest(metric, d, dlow)
    key = ("contest", metric, d, dlow)
    ix = _index(g, c, metric)
    failures = []

    def check(what, r, launched, w):
        bad = _against(r, w)
        if launched != "walk_general_kernel":
            bad.append("launched %s" % launched)
        if bad:
            failures.append((what, bad))

    r, launched, _ = _bridged(g, ix, c, ef, flags=g.FLAG_WIDE_INDEX)
    check("wide index", r, launched, _expected(orc, key, c, ef, metric))
    rng = tu.rng_of(9901)
    pools = [np.arange(grp * tu.PER, (grp + 1) * tu.PER) for grp in c["qg"]]
    ent2 = np.stack([c["ent"], tg.allowed_entries(rng, c["T"], c["Q"], pools)], axis=1).astype(np.uint32)
    r, launched, _ = _bridged(g, ix, c, ef, entry_ids=ent2)
    check("two entry points", r, launched, _expected(orc, key, c, ef, metric, ent=ent2))
    # the auxiliary graph, bridged through itself
    aux = datagen.contest_graph(tu.rng_of(9902), tu.GROUPS, tu.PER, 0, 6)
    ix.set_aux_graph(*aux)
    for llf in (False, True):
        r, launched, _ = _bridged(g, ix, c, ef, aux=True, llf=llf, hops_bound=50)
        check("auxiliary graph llf %d" % llf, r, launched, _expected(orc, key, c, ef, metric, aux=aux, llf=llf, hops_bound=50))
    ix.close()
    assert not failures, failures


# ---- 5. hand-built graphs ----------------------------------------------------------------------------------------------------------------------
def test_parity_graph_walks_through_the_odd_rows(g, orc):
    """(a), (d): only even rows are allowed, every neighbour of an even row is odd and its row holds even ids, u among them.  The cut walk
    returns the entry alone; the bridged walk is the oracle's on G'' and makes more than one hop."""
    c = bu.parity()
    key = ("parity",)
    assert (_expected(orc, key, c, 8, 0)["hops"] > 1).all()
    failures = _instances(g, orc, key, c, 0, 32, beams=(8, 100)) + _instances(g, orc, key, c, 0, 32, beams=(64,), flags=g.FLAG_WIDE_INDEX, general=True)
    assert not failures, failures


def test_twin_rows_are_claimed_and_counted_once(g, orc):
    """(b): two adjacent disallowed neighbours with identical rows -- every looked-through id twice inside one chunk of the pair form and of
    the general kernel.  dist_calc, the candidates and their order are the sequential ones."""
    c = bu.twins()
    key = ("twins",)
    failures = _instances(g, orc, key, c, 0, 32, beams=(8, 64, 100)) + _instances(g, orc, key, c, 0, 32, beams=(8, 64), flags=g.FLAG_WIDE_INDEX, general=True)
    assert not failures, failures


@pytest.mark.parametrize("slots", [40, 72])
def test_a_disallowed_chunk_is_not_the_end_of_a_looked_through_row(g, orc, slots):
    """(c): tag_util.odd_first -- every row is 32 / 64 disallowed slots followed by 8 allowed ones, for u and for every row looked through."""
    c = tg.odd_first(slots)
    key = ("odd_first", slots)
    assert (_expected(orc, key, c, 8, 0)["count"] == 8).all()
    failures = _instances(g, orc, key, c, 0, 32, beams=(8, 100)) + _instances(g, orc, key, c, 0, 32, beams=(8,), flags=g.FLAG_WIDE_INDEX, general=True)
    assert not failures, failures


# ---- 6. hand-over -----------------------------------------------------------------------------------------------------------------------------
def test_hand_over_goes_to_the_bridged_general_kernel(g, orc):
    """A visited set of 128 entries whose probe sequences give up at once: the bridge instance hands queries over, there is no retry pass,
    the general kernel's bridged instance finishes them -- the outputs are still the oracle's."""
    metric, d, dlow, ef = 0, 128, 32, 64
    c = tg.contest(metric, d, dlow)
    ix = _index(g, c, metric)
    ix.knob("vs_disp", 1)
    w = _expected(orc, ("contest", metric, d, dlow), c, ef, metric)
    r, launched, p = _bridged(g, ix, c, ef, hash_capacity=128)
    assert launched == bu.bridge_kernel(metric, dlow, ef), launched
    assert not _against(r, w), _against(r, w)
    assert p["general_queries"] > 0 and p["retry_kernel"] == "", p
    print("bridged hand-over general_queries", p["general_queries"])
    ix.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(g):
    metric, d, dlow, ef = 0, 128, 32, 64
    c = tg.contest(metric, d, dlow)
    ix = _index(g, c, metric, profile=False)
    kw = dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"])
    for top_k in (0, 3):   # gbnns_search_ex / gbnns_search_topk: the flag has no meaning there
        with pytest.raises(g.GbnnsError) as e:
            ix.search(c["queries"], ef, flags=g.FLAG_TAG_BRIDGE, top_k=top_k, **kw)
        assert e.value.code == 1, (top_k, e.value)
    ix.enable_half_rows()
    with pytest.raises(g.GbnnsError) as e:
        ix.search(c["queries"], ef, flags=g.FLAG_TAG_BRIDGE | g.FLAG_HALF_ROWS, query_tags=c["Q"], **kw)
    assert e.value.code == 5, e.value
    ix.search(c["queries"], ef, flags=g.FLAG_TAG_BRIDGE, query_tags=c["Q"], **kw)   # the handle still serves
    ix.close()
