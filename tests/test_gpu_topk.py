"""The k-answer re-rank on an MI355X (run with -m gpu): gbnns_rerank_topk on candidate lists and gbnns_search_topk behind every walk
kernel family, ids and distance bits against rows computed on the CPU with the oracle's scalar distances (tests/topk_util.py).
Nothing takes a tolerance.  tests/test_topk_cpu.py proves that the contest lists used here are decided by the order of the float32
roundings and by the pop-index tie rule.
"""
import numpy as np
import pytest

import datagen
import golden_util as gu
import locality_order_util as lo
import oracle as orc_mod
import topk_util as tu

pytestmark = pytest.mark.gpu

NONE = tu.NONE


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _same_rows(got_ids, got_dist, want_ids, want_dist, key):
    bad = np.flatnonzero((got_ids != want_ids).any(axis=1))
    assert bad.size == 0, (key, "ids", bad.size, [(int(i), got_ids[i][:6].tolist(), want_ids[i][:6].tolist()) for i in bad[:4]])
    if got_dist is not None:
        bad = np.flatnonzero((gu.bits(got_dist) != gu.bits(want_dist)).any(axis=1))
        assert bad.size == 0, (key, "distance bits", bad.size, bad[:8].tolist())


# ---- 1. stand-alone, on the equal-distance contests ------------------------------------------------------------------
TOPK_KS = (1, 10, 32, 33, 64, 65, 200)


@pytest.mark.parametrize("d,metric", tu.RERANK_SHAPES, ids=["d%d_m%d" % s for s in tu.RERANK_SHAPES])
def test_rerank_topk_contest_stand_alone(g, orc, d, metric):
    """gbnns_rerank_topk on candidates that are equidistant in real arithmetic: which ids make the row, and in which order, is decided
    by the reference's summation order and, among equal float32 distances, by pop position.  Every distance form of the re-rank
    (topk_util.RERANK_SHAPES), counts 0 .. 200 around the 32- and 64-candidate passes, k around the same marks: rows shorter than
    k end in 0xFFFFFFFF / +inf.  k = 1 is getRealNearest; column 0 is gbnns_rerank's answer at every k."""
    base, q, cand, count = tu.rerank_contest(d, metric)
    off, nbr = datagen.contest_graph(tu.rng_of(1), tu.GROUPS, tu.PER, 1, 2)
    dist = tu.list_distances(orc, base, q, cand, count, metric)
    some = count > 0
    nearest = np.full(len(count), NONE, np.uint32)
    nearest[some] = orc.rerank(q[some], cand[some], count[some], base, metric=metric, threads=8)
    full = count == cand.shape[1]
    ix = g.Index(base, off, nbr, metric=metric)
    best = ix.rerank(q, cand, count)
    assert np.array_equal(best, nearest), (d, metric, "gbnns_rerank")
    for k in TOPK_KS:
        want_ids, want_dist = tu.expected_topk(dist, cand, count, k)
        ids, dd = ix.rerank_topk(q, cand, k, count)
        _same_rows(ids, dd, want_ids, want_dist, (d, metric, k))
        assert np.array_equal(ids[:, 0], best), (d, metric, k, "column 0 against gbnns_rerank")
        if k == 1:
            assert np.array_equal(ids[:, 0], nearest), (d, metric, "k = 1 against getRealNearest")
        # full lists without a count array (count = stride), and without the distances
        ids, dd = ix.rerank_topk(q[full], cand[full], k)
        _same_rows(ids, dd, want_ids[full], want_dist[full], (d, metric, k, "count = stride"))
        ids, dd = ix.rerank_topk(q, cand, k, count, want_dist=False)
        assert dd is None
        _same_rows(ids, None, want_ids, None, (d, metric, k, "no out_dist"))
    ix.close()


# ---- 2. stand-alone, distinct distances: the sort ---------------------------------------------------------------------
SORT_SHAPES = [(128, 0), (128, 1), (300, 0), (300, 1), (45, 0), (45, 1)]


@pytest.mark.parametrize("d,metric", SORT_SHAPES, ids=["d%d_m%d" % s for s in SORT_SHAPES])
def test_rerank_topk_sorts_distinct_distances(g, orc, d, metric):
    """Full-mantissa vectors: the 200 distances of a list are nearly all distinct, so the row is a sort.  The candidate rows are drawn
    with replacement: every one has an id twice, which is reported once per occurrence -- adjacent, in pop order."""
    rng = tu.rng_of(7100 + 2 * d + metric)
    base = datagen.full_mantissa(rng, 2048, d)
    q = datagen.full_mantissa(rng, 64, d)
    cand = rng.integers(0, 2048, size=(64, 200)).astype(np.uint32)
    count = np.full(64, 200, np.int32)
    assert all(len(np.unique(row)) < 200 for row in cand)
    dist = tu.list_distances(orc, base, q, cand, count, metric)
    assert np.median([len(np.unique(row)) for row in dist]) >= 150
    off, nbr = datagen.random_graph(rng, 2048, 1, 2)
    ix = g.Index(base, off, nbr, metric=metric)
    for k in (10, 200):
        want_ids, want_dist = tu.expected_topk(dist, cand, count, k)
        ids, dd = ix.rerank_topk(q, cand, k, count)
        _same_rows(ids, dd, want_ids, want_dist, (d, metric, k))
    # (k = 200) an id that occurs twice sits in neighbouring columns
    for i, row in enumerate(ids):
        for v in np.unique(row):
            at = np.flatnonzero(row == v)
            assert len(at) == (cand[i] == v).sum() and at[-1] - at[0] == len(at) - 1, (d, metric, i, int(v), at.tolist())
    ix.close()


# ---- 3. a long list: more than 16 keys per lane, a last partial pass -------------------------------------------------
def test_rerank_topk_long_lists(g, orc):
    d, metric, stride = 128, 0, 1100
    rng = tu.rng_of(7300)
    base = datagen.full_mantissa(rng, 2048, d)
    q = datagen.full_mantissa(rng, 16, d)
    cand = rng.integers(0, 2048, size=(16, stride)).astype(np.uint32)
    count = np.array([(1024, 1025, 1100)[i % 3] for i in range(16)], np.int32)
    dist = tu.list_distances(orc, base, q, cand, count, metric)
    off, nbr = datagen.random_graph(rng, 2048, 1, 2)
    ix = g.Index(base, off, nbr, metric=metric)
    want_ids, want_dist = tu.expected_topk(dist, cand, count, stride)
    ids, dd = ix.rerank_topk(q, cand, stride, count)
    _same_rows(ids, dd, want_ids, want_dist, ("long", stride))
    assert np.array_equal(ids[:, 0], ix.rerank(q, cand, count))
    ix.close()


# ---- 4. through the search: every walk kernel family leaves its candidates to the top-k kernel ---------------------
def _hosts(g):
    """(ef, knobs, flags, hash_capacity): the fused walk_hot (ef 8, 64), walk_hot2 (100), walk_hot_big and the two-wavefront walk (200),
    the bitmap first pass, the re-rank in its own launch, a visited set too small (hand-over to the retry and general kernels), the
    LDS-list kernel (1 100); on the wider walked rows and the dot metric the generic instances of the same beams."""
    return [(8, {}, 0, 0), (64, {}, 0, 0), (100, {}, 0, 0), (200, {"coop": 0}, 0, 0), (200, {"coop": 1}, 0, 0),
            (200, {"coop": 0}, g.FLAG_BITMAP_PASS, 0), (64, {}, g.FLAG_NO_FUSED_RERANK, 0), (64, {}, 0, 128), (1100, {}, 0, 0)]


def _expected_from_walk(orc, c, w, metric, k, memo):
    dist = tu.list_distances(orc, c["base"], c["queries"], w["ids"], w["count"], metric, memo)
    return tu.expected_topk(dist, w["ids"], w["count"], k)


SEARCH_SHAPES = [(0, 128, 32), (0, 960, 64), (0, 300, 32), (1, 200, 32)]


@pytest.mark.parametrize("metric,d,dlow", SEARCH_SHAPES, ids=["m%d_d%d_low%d" % s for s in SEARCH_SHAPES])
def test_search_topk_on_a_contest_index(g, orc, metric, d, dlow):
    """gbnns_search_topk (MODE_LOWQ) on a contest index: the rows equal the contract applied to the oracle's walk; ids, hops and
    dist_calc are those of the call without top_k; column 0 is the answer."""
    c = tu.contest_index_data(metric, d, dlow)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric)
    ix.profile_enable(True)
    walks, memo = {}, {}
    for ef, knobs, flags, cap in _hosts(g):
        if ef not in walks:
            walks[ef] = orc.walk(c["q_low"], c["db_low"], c["off"], c["nbr"], ef, entries=c["ent"], metric=metric, threads=8)
        w = walks[ef]
        ix.knob("coop", knobs.get("coop", -1))
        kw = dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=("hops", "dist_calc", "cand"), flags=flags,
                  hash_capacity=cap)
        plain = ix.search(c["queries"], ef, **kw)
        assert np.array_equal(plain["cand"], w["ids"]), (metric, d, dlow, ef, flags, cap)
        for k in sorted({1, min(10, ef), ef}):
            ix.profile_read(reset=True)
            r = ix.search(c["queries"], ef, top_k=k, **kw)
            p = ix.profile_read(reset=True)
            key = (metric, d, dlow, ef, tuple(knobs.items()), flags, cap, k, p["walk_kernel"])
            print("search_topk", key)
            want_ids, want_dist = _expected_from_walk(orc, c, w, metric, k, memo)
            _same_rows(r["top_ids"], r["top_dist"], want_ids, want_dist, key)
            for name in ("ids", "hops", "dist_calc", "cand"):
                assert np.array_equal(r[name], plain[name]), (key, name)
            assert np.array_equal(r["top_ids"][:, 0], r["ids"]), key
            # the same call with the batch walked in locality order: the top-k kernel behind it reads the candidate rows of the queries' own slots
            ro, in_order = lo.in_order(ix, c["q_low"], lambda: ix.search(c["queries"], ef, top_k=k, **kw))
            in_order += lo.same_bytes(ro, r, ("ids", "hops", "dist_calc", "cand", "top_ids", "top_dist"))
            in_order += lo.same_kernels(ix.profile_read(reset=True), p, cap != 0)
            assert not in_order, (key, in_order)
    ix.close()


def test_search_topk_bad_entry_id_on_device_buffers(g, orc):
    """DEVICE buffers are not validated: a query whose entry id is >= n gets an empty candidate list, hence a row of 0xFFFFFFFF / +inf;
    the other rows are those of the HOST call."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = tu.contest_index_data(0, 128, 32)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"])
    for ef, k in ((64, 10), (200, 200)):
        host = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], top_k=k)
        ent = c["ent"].astype(np.int64)
        ent[5] = len(c["base"]) + 3
        r = ix.search(t(c["queries"]), ef, mode=g.MODE_LOWQ, queries_low=t(c["q_low"]), entry_ids=t(ent.astype(np.uint32).view(np.int32)),
                      top_k=k)
        torch.cuda.synchronize()
        ids, dd = r["top_ids"].cpu().numpy().view(np.uint32), r["top_dist"].cpu().numpy()
        assert (ids[5] == NONE).all() and np.isposinf(dd[5]).all(), (ef, k, ids[5][:4], dd[5][:4])
        assert r["ids"].cpu().numpy().view(np.uint32)[5] == NONE
        keep = np.arange(len(ent)) != 5
        _same_rows(ids[keep], dd[keep], host["top_ids"][keep], host["top_dist"][keep], (ef, k, "device against host"))
    ix.close()


# ---- 5. MODE_NET, and PLAIN refused ------------------------------------------------------------------------------------
def test_search_topk_net_mode_and_plain_refused(g, orc):
    metric, d, dlow, ef, k = 0, 128, 32, 64, 10
    c = tu.contest_index_data(metric, d, dlow)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"], metric=metric)
    s = orc.search_batch(orc_mod.MODE_NET, c["queries"], c["base"], c["off"], c["nbr"], ef, db_low=c["db_low"], net=c["net"],
                         entries=c["ent"], metric=metric, threads=8)
    w = orc.walk(orc.project(c["net"], c["queries"]), c["db_low"], c["off"], c["nbr"], ef, entries=c["ent"], metric=metric, threads=8)
    r = ix.search(c["queries"], ef, entry_ids=c["ent"], want=("hops", "dist_calc", "cand"), top_k=k)
    assert np.array_equal(r["cand"], w["ids"])
    assert np.array_equal(r["ids"], s["ids"]) and np.array_equal(r["hops"], s["hops"])
    want_ids, want_dist = _expected_from_walk(orc, c, w, metric, k, {})
    _same_rows(r["top_ids"], r["top_dist"], want_ids, want_dist, ("net", ef, k))
    assert np.array_equal(r["top_ids"][:, 0], s["ids"])
    with pytest.raises(g.GbnnsError):
        ix.search(c["queries"], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=c["ent"], top_k=k)
    with pytest.raises(g.GbnnsError):
        ix.search(c["queries"], ef, entry_ids=c["ent"], top_k=ef + 1)
    ix.close()


# ---- 6. device buffers, batches in flight ----------------------------------------------------------------------------
def test_search_topk_device_buffers_in_flight(g, orc):
    """GBNNS_FLAG_DEFER_JOIN with depth 3 on torch tensors: four distinct 96-query batches rotate over 12 calls; after join and
    synchronise every call's top_ids / top_dist (and ids) equal the synchronous HOST result of its batch."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    metric, d, dlow, ef, k = 0, 128, 32, 64, 10
    c = tu.contest_index_data(metric, d, dlow)
    rng = tu.rng_of(7600)
    batches = []
    for _ in range(4):
        q_low = datagen.full_mantissa(rng, len(c["qg"]), dlow)
        ent = (c["qg"] * tu.PER + rng.integers(0, tu.PER, size=len(c["qg"]))).astype(np.uint32)
        batches.append((q_low, ent))
    ix = g.Index(t(c["base"]), c["off"], c["nbr"], db_low=t(c["db_low"]), metric=metric)
    host = [ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=ql, entry_ids=ent, top_k=k) for ql, ent in batches]
    assert len({h["top_ids"].tobytes() for h in host}) == 4   # the batches are distinct
    q = t(c["queries"])
    dev_in = [(t(ql), t(ent.view(np.int32))) for ql, ent in batches]
    outs = []
    for call in range(12):
        ql, ent = dev_in[call % 4]
        outs.append(ix.search(q, ef, mode=g.MODE_LOWQ, queries_low=ql, entry_ids=ent, out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3,
                              top_k=k))
    ix.join()
    torch.cuda.synchronize()
    for call, r in enumerate(outs):
        h = host[call % 4]
        assert np.array_equal(r["ids"].cpu().numpy().view(np.uint32), h["ids"]), call
        _same_rows(r["top_ids"].cpu().numpy().view(np.uint32), r["top_dist"].cpu().numpy(), h["top_ids"], h["top_dist"], ("in flight", call))
    ix.close()
