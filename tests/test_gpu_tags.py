"""gbnns_search_tagged on an MI355X (run with -m gpu).  The contract: row j is allowed for query i when (T[j] & Q[i]) != 0, and a tagged
search of query i is the reference's search on the graph whose adjacency rows keep the allowed neighbours only.  Every expected value
below is the CPU oracle's on gbnns_dim_red_amd.cut_graph's CSR, one oracle call per distinct value of Q -- candidate ids in pop order,
the bit patterns of their distances, hops, dist_calc, answers -- and nothing takes a tolerance.  tests/test_tags_cpu.py proves that on
each fixture the walk on G' differs from the walk on the full graph; the instance tests assert it again.
"""
import numpy as np
import pytest

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
        _EXPECTED[k] = tg.expected(orc, c, ef, metric, **kw)
    return _EXPECTED[k]


def _against(r, w):
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append("candidate ids (%d rows)" % tg.rows_that_differ(r["cand"], w["ids"]))
    if not np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])):
        bad.append("distance bits (%d differ)" % int((gu.bits(r["cand_dist"]) != gu.bits(w["dists"])).sum()))
    if not np.array_equal(r["hops"], w["hops"]):
        bad.append("hops")
    if not np.array_equal(r["dist_calc"], w["dist_calc"]):
        bad.append("dist_calc")
    if not np.array_equal(r["ids"], w["want"]):
        bad.append("answers (%d differ)" % int((r["ids"] != w["want"]).sum()))
    return bad


def _tagged(g, ix, c, ef, flags=0, **kw):
    """One profiled tagged LOWQ search -> (results, name of the first-pass kernel, profile)."""
    ix.profile_read(reset=True)
    kw.setdefault("entry_ids", c["ent"])
    kw.setdefault("query_tags", c["Q"])
    r = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], want=WANT, flags=flags, **kw)
    p = ix.profile_read(reset=True)
    return r, p["walk_kernel"].split(" (")[0], p


def _index(g, c, metric, profile=True, **kw):
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric, **kw)
    ix.set_tags(c["T"])
    if profile:
        ix.profile_enable(True)
    return ix


def _instances(g, orc, key, c, metric, dlow, one_pass, beams=tg.BEAMS, vacuity=True):
    """Every beam (and both row-request orders of the 576-byte instance) on one index -> the list of failures.  Each case runs a second time
    in locality order (locality_order_util.in_order): same kernel, a valid order read back, every output equal byte for byte."""
    ix = _index(g, c, metric)
    failures = []
    for ef in beams:
        w = _expected(orc, key, c, ef, metric)
        if vacuity:
            differ, of = tg.restricted_queries_that_differ(w, tg.untagged(orc, c, ef, metric), c["Q"])
            assert 4 * differ >= of > 0, ("the case is vacuous", key, ef, differ, of)
        for late in ((0, 1) if (dlow == 144 and ef > 128) else (0,)):
            ix.knob("late_rows", late)
            r, launched, p = _tagged(g, ix, c, ef)
            bad = _against(r, w)
            planned = tg.tag_kernel(metric, dlow, ef, one_pass, late=bool(late))
            if launched != planned:
                bad.append("launched %s, expected %s" % (launched, planned))
            if p["retry_kernel"]:
                bad.append("a retry pass ran: %s" % p["retry_kernel"])
            # the instance, not the fall-back, is what was compared (a shape without a tag instance runs whole on the general kernel)
            if planned != "walk_general_kernel" and p["general_queries"] * 8 > len(c["Q"]):
                bad.append("%d queries went to the general kernel" % p["general_queries"])
            print("tagged", key, ef, late, launched, "general_queries", p["general_queries"])
            # once more with the batch walked in locality order: work item b walks query order[b], under that query's own word, from its entry
            (ro, lo_launched, po), in_order = lo.in_order(ix, c["q_low"], lambda: _tagged(g, ix, c, ef))
            in_order += lo.same_bytes(ro, r, ("ids",) + WANT)
            if (lo_launched, po["retry_kernel"]) != (launched, p["retry_kernel"]):
                in_order.append("launched %s / '%s'" % (lo_launched, po["retry_kernel"]))
            bad += ["in order: " + b for b in in_order]
            if bad:
                failures.append((key, ef, late, bad))
    ix.close()
    return failures


# ---- 1. every tag instance, by name and bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d,dlow", tg.SHAPES, ids=["m%d_d%d_low%d" % s for s in tg.SHAPES])
def test_tag_instances_on_the_contest_indexes(g, orc, metric, d, dlow):
    """One-pass adjacency rows: the one-register list (ef 8, 64), the two-register list (100) and the two-list kernel (200) of every walked
    width, three values of Q (about 1/2, 1/8 and all rows) in one batch; 576-byte rows have a tag instance at ef 200 only, in both orders
    of the row requests -- below it the general kernel takes the batch."""
    c = tg.contest(metric, d, dlow)
    failures = _instances(g, orc, ("contest", metric, d, dlow), c, metric, dlow, True)
    assert not failures, failures


@pytest.mark.parametrize("metric,dlow", tg.TWO_PASS_SHAPES, ids=["m%d_low%d" % s for s in tg.TWO_PASS_SHAPES])
def test_tag_instances_on_two_pass_adjacency_rows(g, orc, metric, dlow):
    """Adjacency rows of 33 .. 48 slots: the instances with the pass loop."""
    c = tg.two_pass(metric, dlow)
    failures = _instances(g, orc, ("two_pass", metric, dlow), c, metric, dlow, False)
    assert not failures, failures


# ---- 2. a chunk that is all disallowed is not the end of the row --------------------------------------------------------------
@pytest.mark.parametrize("slots", [40, 72])
def test_a_disallowed_chunk_is_not_the_end_of_the_row(g, orc, slots):
    """Rows whose first 32 / 64 neighbours are odd ids and whose last 8 are even, T allows the even rows: the preloaded first chunk (and,
    72 slots, the second one) is all disallowed.  Beams 8 / 100 / 200: the one- and two-register lists and the two-list kernel in their
    pass-loop forms; 576-byte rows at ef 200 in both orders of the row requests and, below it, the general kernel."""
    c = tg.odd_first(slots)
    failures = _instances(g, orc, ("odd_first", slots, 32), c, 0, 32, False, beams=(8, 100, 200), vacuity=False)
    failures += _instances(g, orc, ("odd_first", slots, 144), tg.odd_first(slots, 144), 0, 144, False, beams=(8, 200), vacuity=False)
    assert not failures, failures
    for ef in (8, 200):   # (what a kernel that broke on the empty chunk would return: the entry alone)
        assert (_expected(orc, ("odd_first", slots, 32), c, ef, 0)["count"] == ef).all()


# ---- 3. identity ----------------------------------------------------------------------------------------------------------------
def test_all_allowed_equals_the_untagged_search(g):
    metric, d, dlow = 0, 128, 32
    c = tg.contest(metric, d, dlow)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"], metric=metric)
    ix.set_tags(np.full(tg.N, tg.ALL, np.uint32))
    q_all = np.full(len(c["Q"]), tg.ALL, np.uint32)
    want = WANT + ("edges",)
    runs = []
    for ef in (8, 64, 200):
        runs.append(("NET ef %d" % ef, dict(ef=ef, entry_ids=c["ent"], want=want + ("q_low",), top_k=5)))
        runs.append(("LOWQ unfused ef %d" % ef, dict(ef=ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=want,
                                                    flags=g.FLAG_NO_FUSED_RERANK)))
        for k in (1, 5):
            runs.append(("PLAIN k %d ef %d" % (k, ef), dict(ef=ef, mode=g.MODE_PLAIN, k=k, entry_ids=c["ent"], want=want)))
    for what, kw in runs:
        ef = kw.pop("ef")
        plain = ix.search(c["queries"], ef, **kw)
        tagged = ix.search(c["queries"], ef, query_tags=q_all, **kw)
        assert set(plain) == set(tagged)
        for name in plain:
            assert tagged[name].tobytes() == plain[name].tobytes(), (what, name)
    ix.close()


# ---- 4. bad entries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_bad_entries_get_the_empty_row(g, orc, where):
    """Q == 0, an entry row the query may not see, an entry id >= n: each gets the bad-entry row and its neighbours in the batch are the
    oracle's -- from a tag instance (ef 64, 200), from the general kernel (GBNNS_FLAG_WIDE_INDEX) and in the top-k rows."""
    import torch
    metric, d, dlow = 0, 128, 32
    c = tg.contest(metric, d, dlow)
    Q, ent = c["Q"].copy(), c["ent"].copy()
    Q[[3, 40]] = 0
    banned = np.flatnonzero((c["T"] & 0x01) == 0)
    ent[[10, 55]] = banned[[5, 300]]            # queries 10 and 55 have Q == 0x01
    assert (Q[[10, 55]] == 0x01).all()
    ent[[20, 77]] = [tg.N, 0xFFFFFFF0]
    bad_rows = np.array([3, 40, 10, 55, 20, 77])
    assert not tg.entry_ok(c["T"], Q, ent)[bad_rows].any() and tg.entry_ok(c["T"], Q, ent).sum() == len(Q) - 6
    ix = _index(g, c, metric, profile=False)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for ef, flags in ((64, 0), (200, 0), (64, g.FLAG_WIDE_INDEX)):
        w = _expected(orc, ("contest", metric, d, dlow), c, ef, metric, Q=Q, ent=ent)
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
    ix.close()


# ---- 5. hand-over -----------------------------------------------------------------------------------------------------------------
def test_hand_over_goes_straight_to_the_general_kernel(g, orc):
    """A visited set of 128 entries whose probe sequences give up at once: the tag instance hands queries over, there is no retry pass,
    the tagged general kernel finishes them -- the outputs are still the oracle's."""
    metric, d, dlow = 0, 128, 32
    c = tg.contest(metric, d, dlow)
    ix = _index(g, c, metric)
    ix.knob("vs_disp", 1)
    for ef in (64, 200):
        w = _expected(orc, ("contest", metric, d, dlow), c, ef, metric)
        r, launched, p = _tagged(g, ix, c, ef, hash_capacity=128)
        assert launched == tg.tag_kernel(metric, dlow, ef, True), launched
        assert not _against(r, w), (ef, _against(r, w))
        assert p["general_queries"] > 0 and p["retry_kernel"] == "", p
        print("tagged hand-over ef", ef, "general_queries", p["general_queries"])
    ix.close()


# ---- 6. the general kernel's domain ------------------------------------------------------------------------------------------------
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

    r, launched, _ = _tagged(g, ix, c, ef, flags=g.FLAG_WIDE_INDEX)
    check("wide index", r, launched, _expected(orc, key, c, ef, metric))
    # two entry points per query, both rows the query may see, inside its component
    rng = tu.rng_of(9500)
    pools = [np.arange(grp * tu.PER, (grp + 1) * tu.PER) for grp in c["qg"]]
    ent2 = np.stack([c["ent"], tg.allowed_entries(rng, c["T"], c["Q"], pools)], axis=1).astype(np.uint32)
    r, launched, _ = _tagged(g, ix, c, ef, entry_ids=ent2)
    check("two entry points", r, launched, _expected(orc, key, c, ef, metric, ent=ent2))
    ent_bad = ent2.copy()
    ent_bad[4, 1] = np.flatnonzero((c["T"] & c["Q"][4]) == 0)[0]   # one of the two is not allowed: the bad-entry row
    r, launched, _ = _tagged(g, ix, c, ef, entry_ids=ent_bad)
    w = _expected(orc, key, c, ef, metric, ent=ent_bad)
    assert w["count"][4] == 0
    check("two entry points, one not allowed", r, launched, w)
    # the auxiliary graph, cut the same way
    aux = datagen.contest_graph(tu.rng_of(9501), tu.GROUPS, tu.PER, 0, 6)
    ix.set_aux_graph(*aux)
    for llf in (False, True):
        for hb in (3, 50):
            r, launched, _ = _tagged(g, ix, c, ef, aux=True, llf=llf, hops_bound=hb)
            check("auxiliary graph llf %d hops_bound %d" % (llf, hb), r, launched, _expected(orc, key, c, ef, metric, aux=aux, llf=llf, hops_bound=hb))
    ix.close()
    assert not failures, failures


# ---- 7. top-k -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ef", [64, 200])
def test_topk_of_a_tagged_search(g, orc, ef):
    metric, d, dlow = 0, 128, 32
    c = tg.contest(metric, d, dlow)
    ix = _index(g, c, metric, profile=False)
    w = _expected(orc, ("contest", metric, d, dlow), c, ef, metric)
    memo = {}
    for k in (1, 10, ef):
        r = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], query_tags=c["Q"], want=WANT, top_k=k)
        assert not _against(r, w), (k, _against(r, w))
        count = (r["cand"] != tg.NONE).sum(axis=1)
        dist = tu.list_distances(orc, c["base"], c["queries"], r["cand"], count, metric, memo)
        want_ids, want_dist = tu.expected_topk(dist, r["cand"], count, k)
        assert np.array_equal(r["top_ids"], want_ids) and np.array_equal(gu.bits(r["top_dist"]), gu.bits(want_dist)), k
        assert np.array_equal(r["top_ids"][:, 0], r["ids"])
        for name in ("cand", "top_ids"):
            ids = r[name]
            seen = ids != tg.NONE
            assert ((c["T"][np.where(seen, ids, 0)] & c["Q"][:, None]) != 0)[seen].all(), (k, name)
    ix.close()


# ---- 8. tag updates -------------------------------------------------------------------------------------------------------------------
def test_tag_updates(g, orc):
    metric, d, dlow, ef = 0, 128, 32, 64
    c = tg.contest(metric, d, dlow)
    kw = dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=WANT)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric)
    before = ix.search(c["queries"], ef, **kw)
    with pytest.raises(g.GbnnsError) as e:   # no table yet
        ix.search(c["queries"], ef, query_tags=c["Q"], **kw)
    assert e.value.code == 1
    # rows [512, 1536) get their tags, the others keep the initial all-ones word
    T = np.full(tg.N, tg.ALL, np.uint32)
    T[512:1536] = c["T"][512:1536]
    ix.set_tags(c["T"][512:1536], first=512)
    r = ix.search(c["queries"], ef, query_tags=c["Q"], **kw)
    w = tg.expected(orc, c, ef, metric, T=T)
    assert not _against(r, w), _against(r, w)
    assert tg.rows_that_differ(w["ids"], _expected(orc, ("contest", metric, d, dlow), c, ef, metric)["ids"]) > 0
    # ... then the rest, from a device buffer
    import torch
    ix.set_tags(torch.from_numpy(c["T"][:512].view(np.int32).copy()).to("cuda:0"))
    ix.set_tags(c["T"][1536:], first=1536)
    r = ix.search(c["queries"], ef, query_tags=c["Q"], **kw)
    assert not _against(r, _expected(orc, ("contest", metric, d, dlow), c, ef, metric))
    after = ix.search(c["queries"], ef, **kw)   # an untagged search does not see the table
    for name in before:
        assert after[name].tobytes() == before[name].tobytes(), name
    ix.clear_tags()
    with pytest.raises(g.GbnnsError) as e:
        ix.search(c["queries"], ef, query_tags=c["Q"], **kw)
    assert e.value.code == 1
    ix.set_tags(np.zeros(0, np.uint32))         # an empty range creates the table: all ones
    r = ix.search(c["queries"], ef, query_tags=np.full(len(c["Q"]), 1, np.uint32), **kw)
    for name in before:
        assert r[name].tobytes() == before[name].tobytes(), name
    ix.close()


# ---- 9. batches in flight ---------------------------------------------------------------------------------------------------------------
def test_tagged_batches_in_flight(g, orc):
    """Three tagged batches with GBNNS_FLAG_DEFER_JOIN (depth 3) and different Q arrays on torch tensors, twice round: after join and
    synchronise every call's outputs equal the synchronous HOST result of its batch, which equals the oracle on the cut graphs."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    metric, d, dlow, ef = 0, 128, 32, 64
    c = tg.contest(metric, d, dlow)
    rng = tu.rng_of(9600)
    pools = [np.arange(grp * tu.PER, (grp + 1) * tu.PER) for grp in c["qg"]]
    batches = []
    for b in range(3):
        Q = np.roll(c["Q"], b)
        batches.append((Q, tg.allowed_entries(rng, c["T"], Q, pools)))
    ix = g.Index(t(c["base"]), c["off"], c["nbr"], db_low=t(c["db_low"]), metric=metric)
    ix.set_tags(c["T"])
    kw = dict(mode=g.MODE_LOWQ, want=WANT)
    host = [ix.search(c["queries"], ef, queries_low=c["q_low"], entry_ids=ent, query_tags=Q, **kw) for Q, ent in batches]
    assert len({h["cand"].tobytes() for h in host}) == 3   # the batches are distinct
    for (Q, ent), h in zip(batches, host):
        assert not _against(h, tg.expected(orc, c, ef, metric, Q=Q, ent=ent))
    q, ql = t(c["queries"]), t(c["q_low"])
    dev_in = [(t(Q.view(np.int32)), t(ent.view(np.int32))) for Q, ent in batches]
    outs = []
    for call in range(6):
        Q, ent = dev_in[call % 3]
        outs.append(ix.search(q, ef, queries_low=ql, entry_ids=ent, query_tags=Q, out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3, **kw))
    ix.join()
    torch.cuda.synchronize()
    for call, r in enumerate(outs):
        h = host[call % 3]
        for name in ("ids",) + WANT:
            assert r[name].cpu().numpy().tobytes() == h[name].tobytes(), (call, name)
    ix.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(g):
    metric, d, dlow, ef = 0, 128, 32, 64
    c = tg.contest(metric, d, dlow)
    kw = dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], query_tags=c["Q"])
    ix = _index(g, c, metric, profile=False)
    ix.enable_half_rows()
    for flags in (g.FLAG_HALF_ROWS, g.FLAG_MFMA_PROJECTION):
        with pytest.raises(g.GbnnsError) as e:
            ix.search(c["queries"], ef, flags=flags, **kw)
        assert e.value.code == 5, (flags, e.value)
    with pytest.raises(g.GbnnsError) as e:
        ix.search(c["queries"], ef, top_k=ef + 1, **kw)
    assert e.value.code == 1
    with pytest.raises(g.GbnnsError) as e:   # PLAIN: k == 0 only
        ix.search(c["queries"], ef, mode=g.MODE_PLAIN, entry_ids=c["ent"], query_tags=c["Q"], top_k=1)
    assert e.value.code == 1
    for first, count in ((tg.N - 3, 4), (tg.N + 1, 0), (0, tg.N + 1)):
        with pytest.raises(g.GbnnsError) as e:
            ix.set_tags(np.ones(count, np.uint32), first=first)
        assert e.value.code == 1, (first, count)
    ix.set_tags(np.ones(3, np.uint32), first=tg.N - 3)   # the last rows: inside
    ix.set_tags(c["T"][tg.N - 3:], first=tg.N - 3)
    ix.search(c["queries"], ef, **kw)                     # the handle still serves
    ix.close()


# ---- 11. the knob the timing tool uses ---------------------------------------------------------------------------------------------------
def test_knob_hot_puts_untagged_calls_on_the_generic_family(g):
    """Knob "hot" = 0: an untagged search takes the generic instance the tag instances are built from, with the same outputs."""
    for (metric, d, dlow), ef, generic in (((0, 128, 32), 64, "walk_reg_kernel<0, 8, true, false, 1, true, false>"),
                                           ((0, 96, 48), 40, "walk_reg_kernel<0, 12, true, false, 1, true, false>"),
                                           ((0, 128, 32), 200, "walk_reg_big_kernel<0, 8, true, false, false, true, false>")):
        c = tg.contest(metric, d, dlow)
        ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric)
        ix.profile_enable(True)
        ix.knob("coop", 0)
        kw = dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=WANT + ("edges",))
        runs = {}
        for hot in (1, 0, 1):
            ix.knob("hot", hot)
            assert ix.knob_get("hot") == hot
            ix.profile_read(reset=True)
            r = ix.search(c["queries"], ef, **kw)
            runs.setdefault(hot, []).append((r, ix.profile_read(reset=True)["walk_kernel"].split(" (")[0]))
        assert runs[0][0][1] == generic, runs[0][0][1]
        assert runs[1][0][1] == runs[1][1][1] != generic
        for name in runs[0][0][0]:
            assert runs[0][0][0][name].tobytes() == runs[1][0][0][name].tobytes() == runs[1][1][0][name].tobytes(), name
        ix.close()
