"""The half-base handle (Index(db=<float16>), gbnns_index_create_half_base) on an MI355X (run with -m gpu).  The contract: every call returns
what the same call returns on the handle over db.astype(float32), bit for bit.  Every expected value below is the unchanged CPU oracle's on
the widened table -- candidate ids in pop order, the bit patterns of distances, hops, dist_calc, answers, the exact top-k distances -- and
nothing takes a tolerance.  tests/test_half_base_cpu.py proves that on every fixture the order of the roundings is visible and that
bit-equal pairs exist, so a kernel that added in another order, flushed a subnormal, lost the sign of a zero or broke a tie the other way
cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

import bridge_util as bg
import datagen
import golden_util as gu
import half_base_util as hb
import half_rows_util as hu
import oracle as orc_mod
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


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _index(g, c, metric=0, table="base", **kw):
    ix = g.Index(c[table], c["off"], c["nbr"], db_low=c["db_low"], metric=metric, **kw)
    assert ix.is_half_base == (table == "base") and not ix.is_bytes
    ix.profile_enable(True)
    ix.knob("coop", 0)   # (at 96 queries the auto rule takes the two-wavefront walk at ef 200)
    return ix


def _search(g, ix, c, ef, **kw):
    """One profiled LOWQ search -> (results, name of the first-pass kernel, profile)."""
    ix.profile_read(reset=True)
    kw.setdefault("entry_ids", c["ent"])
    kw.setdefault("queries_low", c["q_low"])
    kw.setdefault("mode", g.MODE_LOWQ)
    r = ix.search(c["queries"], ef, want=WANT, **kw)
    p = ix.profile_read(reset=True)
    return r, p["walk_kernel"].split(" (")[0], p


_WALKS = {}


def _oracle(orc, key, c, ef, metric, db_low=None, **kw):
    """(walk over the low-dimensional table, answers re-ranked on the WIDENED half table), once per fixture, beam and call form."""
    k = (key, ef, metric)
    if k not in _WALKS:
        w = orc.walk(c["q_low"], c["db_low"] if db_low is None else db_low, c["off"], c["nbr"], ef, entries=kw.pop("entries", c["ent"]), metric=metric,
                     threads=8, **kw)
        _WALKS[k] = (w, orc.rerank(c["queries"], w["ids"], w["count"], c["wide"], metric=metric, threads=8))
    return _WALKS[k]


def _against(r, w, want):
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append("candidate ids (%d rows)" % hb.rows_that_differ(r["cand"], w["ids"]))
    if not np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])):
        bad.append("distance bits (%d differ)" % int((gu.bits(r["cand_dist"]) != gu.bits(w["dists"])).sum()))
    if not np.array_equal(r["hops"], w["hops"]):
        bad.append("hops")
    if not np.array_equal(r["dist_calc"], w["dist_calc"]):
        bad.append("dist_calc")
    if not np.array_equal(r["ids"], want):
        bad.append("answers (%d differ)" % int((r["ids"] != want).sum()))
    return bad


def _same_bytes(a, b, names=("ids",) + WANT):
    return [n for n in names if np.asarray(a[n]).tobytes() != np.asarray(b[n]).tobytes()]


def _topk_against(orc, c, w, r, k, metric):
    dist = tu.list_distances(orc, c["wide"], c["queries"], w["ids"], w["count"], metric)
    ids, dd = tu.expected_topk(dist, w["ids"], w["count"], k)
    bad = []
    if not np.array_equal(r["top_ids"], ids):
        bad.append("top-%d ids (%d rows)" % (k, hb.rows_that_differ(r["top_ids"], ids)))
    if not np.array_equal(gu.bits(r["top_dist"]), gu.bits(dd)):
        bad.append("top-%d distance bits" % k)
    return bad


# ---- 1. the stand-alone kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,metric", hb.RERANK_SHAPES, ids=["d%d_m%d" % s for s in hb.RERANK_SHAPES])
def test_standalone_half_rerank(g, orc, d, metric):
    """gbnns_rerank and gbnns_rerank_topk (k = 1, 10, 200) over lists of 0 .. 200 candidates, every shape of hb.RERANK_SHAPES (the comment
    there says which loop of which form each enters).  One list holds the table's last row; on DEVICE buffers one holds an id >= n, which is
    read as row 0 and reported as given.  A DEVICE table -- borrowed at d % 8 == 0 and a 16-byte aligned address, re-laid otherwise, which a
    view that starts 8 bytes into its allocation is at every d -- gives the host table's bytes."""
    import torch
    c = hb.rerank_contest(d, metric)
    rng = tu.rng_of(10850 + d)
    off, nbr = datagen.random_graph(rng, hb.N, 2, 30)
    db_low = datagen.full_mantissa(rng, hb.N, 32)
    q, cand, count = c["queries"], c["cand"], c["count"]
    memo = {}
    dist = tu.list_distances(orc, c["wide"], q, cand, count, metric, memo)
    ix = g.Index(c["base"], off, nbr, db_low=db_low, metric=metric)
    assert ix.is_half_base and not ix.is_bytes
    print("half rows d %d metric %d:" % (d, metric), g.half_base_plan(metric, d))
    failures = []
    best = ix.rerank(q, cand, count)
    some = count > 0   # (the oracle's getRealNearest reads the first id of a list: empty lists are the ranked distances' to decide)
    if not np.array_equal(best[some], orc.rerank(q[some], cand[some], count[some], c["wide"], metric=metric, threads=8)):
        failures.append("rerank ids")
    if not np.array_equal(best, tu.expected_topk(dist, cand, count, 1)[0][:, 0]):
        failures.append("rerank ids against the ranked distances")
    got = {}
    for k in (1, 10, 200):
        ids, dd = ix.rerank_topk(q, cand, k, count)
        want_ids, want_dd = tu.expected_topk(dist, cand, count, k)
        got[k] = (ids, dd)
        if not np.array_equal(ids, want_ids):
            failures.append("top-%d ids (%d rows)" % (k, hb.rows_that_differ(ids, want_ids)))
        if not np.array_equal(gu.bits(dd), gu.bits(want_dd)):
            failures.append("top-%d distance bits (%d differ)" % (k, int((gu.bits(dd) != gu.bits(want_dd)).sum())))
    # DEVICE buffers, an id outside the table in every list that has a fourth candidate: read as row 0, reported as given
    cand_out = cand.copy()
    has4 = count > 3
    cand_out[has4, 3] = hb.N + 5
    cand_row0 = cand_out.copy()
    cand_row0[has4, 3] = 0
    dist0 = tu.list_distances(orc, c["wide"], q, cand_row0, count, metric, memo)
    want_ids, want_dd = tu.expected_topk(dist0, cand_out, count, 10)
    lib = g.load_library()
    dq, dc, dn = _t(q), _t(cand_out.view(np.int32)), _t(count)
    dev_base = _t(c["base"])
    flat = torch.zeros(hb.N * d + 4, dtype=torch.float16, device=dev_base.device)
    shifted = flat[4:].view(hb.N, d)   # starts 8 bytes into its allocation: never borrowed
    shifted.copy_(dev_base)
    assert dev_base.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 8
    for table in ("host", "device", "device, misaligned"):
        ixd = ix if table == "host" else g.Index(dev_base if table == "device" else shifted, off, nbr, db_low=_t(db_low), metric=metric)
        assert ixd.is_half_base
        out1 = torch.empty(len(q), dtype=torch.int32, device=dq.device)
        outk = torch.empty((len(q), 10), dtype=torch.int32, device=dq.device)
        outd = torch.empty((len(q), 10), dtype=torch.float32, device=dq.device)
        s = torch.cuda.current_stream().cuda_stream
        assert lib.gbnns_rerank(ixd._h, dq.data_ptr(), len(q), dc.data_ptr(), cand.shape[1], dn.data_ptr(), out1.data_ptr(), 1, s) == 0
        assert lib.gbnns_rerank_topk(ixd._h, dq.data_ptr(), len(q), dc.data_ptr(), cand.shape[1], dn.data_ptr(), 10, outk.data_ptr(), outd.data_ptr(), 1, s) == 0
        torch.cuda.synchronize()
        if not np.array_equal(outk.cpu().numpy().view(np.uint32), want_ids) or not np.array_equal(gu.bits(outd.cpu().numpy()), gu.bits(want_dd)):
            failures.append("%s table, id >= n: top-10" % table)
        if not np.array_equal(out1.cpu().numpy().view(np.uint32), want_ids[:, 0]):
            failures.append("%s table, id >= n: rerank" % table)
        if table != "host":
            ids, dd = ixd.rerank_topk(q, cand, 10, count)
            if ids.tobytes() != got[10][0].tobytes() or dd.tobytes() != got[10][1].tobytes():
                failures.append("%s table differs from the host table" % table)
            ixd.close()
    ix.close()
    assert not failures, failures


# ---- 2. widening is exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_widening_is_exact(g, orc, metric):
    """One-hot rows, one per mark (the smallest and the largest subnormal, the smallest normal, +-65 504, -0) and place -- all eight places
    of both lanes' chunks at d = 32 --, against a zero query and a query of ones: rerank_topk's distances are the oracle's bits on the
    widened table.  Under the zero query a flushed subnormal shows as distance 0, a mis-signed widening as another bit pattern."""
    table = hb.one_hot_table()
    n, d = table.shape
    w = hb.wide(table)
    rng = tu.rng_of(10870)
    off, nbr = datagen.random_graph(rng, n, 2, 8)
    db_low = datagen.full_mantissa(rng, n, 32)
    q = np.ascontiguousarray(np.stack([np.zeros(d, np.float32), np.ones(d, np.float32)]))
    cand = np.ascontiguousarray(np.stack([rng.permutation(n), rng.permutation(n)]).astype(np.uint32))
    count = np.full(2, n, np.int32)
    dist = tu.list_distances(orc, w, q, cand, count, metric)
    if metric == 0:   # the fixture's own point: every subnormal row is visible under the zero query
        sub = np.isin(cand[0], np.arange(0, 2 * hb.ONE_HOT_D))
        assert (dist[0][sub] > 0).all()
    ix = g.Index(table, off, nbr, db_low=db_low, metric=metric)
    ids, dd = ix.rerank_topk(q, cand, n, count)
    want_ids, want_dd = tu.expected_topk(dist, cand, count, n)
    assert np.array_equal(gu.bits(dd), gu.bits(want_dd)), int((gu.bits(dd) != gu.bits(want_dd)).sum())
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(ix.rerank(q, cand, count), want_ids[:, 0])
    ix.close()


# ---- 3. searches ---------------------------------------------------------------------------------------------------------------------
def _pair_check(g, what, failures, h, f, c, ef, w, want, **kw):
    """The half-base handle against the oracle, and against the float handle's call with FLAG_NO_FUSED_RERANK: the same first-pass kernel,
    the same bytes."""
    rh, kh, _ = _search(g, h, c, ef, **kw)
    fkw = dict(kw, flags=kw.get("flags", 0) | g.FLAG_NO_FUSED_RERANK)
    rf, kf, _ = _search(g, f, c, ef, **fkw)
    bad = _against(rh, w, want)
    if kh != kf:
        bad.append("first pass %s, a float handle's unfused %s" % (kh, kf))
    if _same_bytes(rh, rf):
        bad.append("differs from the float handle in %s" % _same_bytes(rh, rf))
    print("half base:", what, "ef", ef, kh)
    if bad:
        failures.append((what, ef, bad))


@pytest.mark.parametrize("metric,d,dlow", hb.INDEX_SHAPES, ids=["m%d_d%d_l%d" % s for s in hb.INDEX_SHAPES])
def test_lowq_every_beam(g, orc, metric, d, dlow):
    c = hb.index_data(metric, d, dlow)
    h, f = _index(g, c, metric), _index(g, c, metric, table="wide")
    failures = []
    for ef in hb.BEAMS:
        w, want = _oracle(orc, ("lowq", d), c, ef, metric)
        _pair_check(g, "LOWQ", failures, h, f, c, ef, w, want)
        # ... and its ten best
        r = h.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=WANT, top_k=min(10, ef))
        bad = _against(r, w, want) + _topk_against(orc, c, w, r, min(10, ef), metric)
        if bad:
            failures.append(("top_k", ef, bad))
    h.close()
    f.close()
    assert not failures, failures


@pytest.mark.parametrize("ef", hb.BEAMS)
@pytest.mark.parametrize("metric,d,dlow", hb.INDEX_SHAPES, ids=["m%d_d%d_l%d" % s for s in hb.INDEX_SHAPES])
def test_call_forms(g, orc, metric, d, dlow, ef):
    """Both indexes at every beam: three entry points, the auxiliary graph, FLAG_HALF_ROWS after enable_half_rows(), tagged (every row, half
    the rows) and bridged calls -- each against the oracle and against the float handle's unfused call."""
    c = hb.index_data(metric, d, dlow)
    h, f = _index(g, c, metric), _index(g, c, metric, table="wide")
    failures = []
    ent3 = np.stack([c["ent"], (c["ent"] // hb.PER) * hb.PER + (c["ent"] % hb.PER + 101) % hb.PER,
                     (c["ent"] // hb.PER) * hb.PER + (c["ent"] % hb.PER + 57) % hb.PER], axis=1).astype(np.uint32)
    w, want = _oracle(orc, ("ent3", d), c, ef, metric, entries=ent3)
    _pair_check(g, "three entry points", failures, h, f, c, ef, w, want, entry_ids=ent3)
    aux = datagen.contest_graph(tu.rng_of(10901), hb.GROUPS, hb.PER, 0, 6)
    for ix in (h, f):
        ix.set_aux_graph(*aux)
    w, want = _oracle(orc, ("aux", d), c, ef, metric, aux=aux, llf=True, hops_bound=50)
    _pair_check(g, "auxiliary graph", failures, h, f, c, ef, w, want, aux=True, llf=True, hops_bound=50)
    for ix in (h, f):
        ix.enable_half_rows()
    w, want = _oracle(orc, ("half rows", d), c, ef, metric, db_low=hu.rounded(c["db_low"]))
    _pair_check(g, "half walked rows", failures, h, f, c, ef, w, want, flags=g.FLAG_HALF_ROWS)
    T = tg.row_tags()
    rng = tu.rng_of(10950)
    pools = [np.arange(q * hb.PER, (q + 1) * hb.PER) for q in c["qg"]]
    cw = dict(c, base=c["wide"])
    for ix in (h, f):
        ix.set_tags(T)
    for what, qv, flags, exp in (("every row allowed", tg.ALL, 0, tg.expected), ("half the rows allowed", 0x0F, 0, tg.expected),
                                 ("bridged", 0x0F, g.FLAG_TAG_BRIDGE, bg.expected)):
        Q = np.full(len(c["qg"]), qv, np.uint32)
        ent = tg.allowed_entries(rng, T, Q, pools)
        e = exp(orc, cw, ef, metric, T=T, Q=Q, ent=ent)
        _pair_check(g, "tagged, " + what, failures, h, f, c, ef, dict(ids=e["ids"], dists=e["dists"], hops=e["hops"], dist_calc=e["dist_calc"]), e["want"],
                    entry_ids=ent, query_tags=Q, flags=flags)
        if qv == 0x0F and not flags:   # the census of the same words
            allowed, first = h.tag_census(Q)
            fa, ff = f.tag_census(Q)
            assert allowed.tobytes() == fa.tobytes() and first.tobytes() == ff.tobytes()
    h.close()
    f.close()
    assert not failures, failures


@pytest.mark.parametrize("ef", hb.BEAMS)
def test_net_mode_and_topk(g, orc, ef):
    metric, d, dlow = hb.INDEX_SHAPES[0]
    c = hb.index_data(metric, d, dlow)
    k = min(10, ef)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    assert ix.is_half_base
    s = orc.search_batch(orc_mod.MODE_NET, c["queries"], c["wide"], c["off"], c["nbr"], ef, db_low=c["db_low"], net=c["net"], entries=c["ent"], threads=8)
    w = orc.walk(orc.project(c["net"], c["queries"]), c["db_low"], c["off"], c["nbr"], ef, entries=c["ent"], threads=8)
    r = ix.search(c["queries"], ef, entry_ids=c["ent"], want=WANT + ("q_low",), top_k=k)
    assert np.array_equal(r["ids"], s["ids"]) and np.array_equal(r["hops"], s["hops"]) and np.array_equal(r["dist_calc"] + ef, s["dist_calc"])
    assert np.array_equal(r["cand"], w["ids"]) and np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"]))
    assert np.array_equal(gu.bits(ix.project(c["queries"])), gu.bits(orc.project(c["net"], c["queries"])))
    assert not _topk_against(orc, c, w, r, k, metric)
    assert np.array_equal(r["top_ids"][:, 0], s["ids"])
    ix.close()


def test_batches_in_flight_on_device_buffers(g, orc):
    """GBNNS_FLAG_DEFER_JOIN with depth 3 on torch tensors, the half table a borrowed torch.float16 tensor: three distinct batches rotate over
    nine calls; after join and synchronise every call's outputs equal the synchronous HOST result of its batch, which equals the oracle."""
    import torch
    metric, d, dlow = hb.INDEX_SHAPES[0]
    c = hb.index_data(metric, d, dlow)
    ef = 64
    rng = tu.rng_of(10960)
    batches = []
    for _ in range(3):
        q_low = datagen.full_mantissa(rng, len(c["qg"]), dlow)
        ent = (c["qg"] * hb.PER + rng.integers(0, hb.PER, size=len(c["qg"]))).astype(np.uint32)
        batches.append((q_low, ent))
    ix = g.Index(_t(c["base"]), c["off"], c["nbr"], db_low=_t(c["db_low"]))
    assert ix.is_half_base
    host = [ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=ql, entry_ids=ent, want=WANT) for ql, ent in batches]
    assert len({h["cand"].tobytes() for h in host}) == 3
    for (ql, ent), h in zip(batches, host):
        w = orc.walk(ql, c["db_low"], c["off"], c["nbr"], ef, entries=ent, threads=8)
        assert not _against(h, w, orc.rerank(c["queries"], w["ids"], w["count"], c["wide"], threads=8))
    q = _t(c["queries"])
    dev_in = [(_t(ql), _t(ent.view(np.int32))) for ql, ent in batches]
    outs = []
    for call in range(9):
        ql, ent = dev_in[call % 3]
        outs.append(ix.search(q, ef, mode=g.MODE_LOWQ, queries_low=ql, entry_ids=ent, out={}, want=WANT, flags=g.FLAG_DEFER_JOIN, defer_depth=3))
    ix.join()
    torch.cuda.synchronize()
    for call, r in enumerate(outs):
        h = host[call % 3]
        for name in ("ids",) + WANT:
            assert r[name].cpu().numpy().tobytes() == h[name].tobytes(), (call, name)
    ix.close()


# ---- 4. a half-base handle is the float handle ------------------------------------------------------------------------------------
def test_half_base_handle_equals_float_handle(g):
    """The same calls on Index(base) and Index(wide(base)) in one process -- the float handle's default (fused) route included: every output
    byte."""
    metric, d, dlow = hb.INDEX_SHAPES[0]
    c = hb.index_data(metric, d, dlow)
    h = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    f = g.Index(c["wide"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    assert h.is_half_base and not f.is_half_base
    for ef in (64, 100, 200):
        for kw in (dict(), dict(top_k=10), dict(mode=g.MODE_LOWQ, queries_low=c["q_low"]), dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], top_k=10)):
            rh = h.search(c["queries"], ef, entry_ids=c["ent"], want=WANT, **kw)
            rf = f.search(c["queries"], ef, entry_ids=c["ent"], want=WANT, **kw)
            names = ("ids",) + WANT + (("top_ids", "top_dist") if "top_k" in kw else ())
            assert not _same_bytes(rh, rf, names), (ef, sorted(kw), _same_bytes(rh, rf, names))
    h.close()
    f.close()
    # rerank / rerank_topk: the contest lists against the float handle over the same rows (any graph will do), every form
    for dd, mm in ((96, 0), (300, 0), (960, 0), (128, 1)):
        rc = hb.rerank_contest(dd, mm)
        h = g.Index(rc["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=mm)
        f = g.Index(rc["wide"], c["off"], c["nbr"], db_low=c["db_low"], metric=mm)
        for k in (1, 10, 200):
            ih, dh = h.rerank_topk(rc["queries"], rc["cand"], k, rc["count"])
            i_f, df = f.rerank_topk(rc["queries"], rc["cand"], k, rc["count"])
            assert ih.tobytes() == i_f.tobytes() and dh.tobytes() == df.tobytes(), (dd, mm, k)
        assert h.rerank(rc["queries"], rc["cand"], rc["count"]).tobytes() == f.rerank(rc["queries"], rc["cand"], rc["count"]).tobytes()
        h.close()
        f.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(g):
    metric, d, dlow = hb.INDEX_SHAPES[0]
    c = hb.index_data(metric, d, dlow)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"])
    lib = g.load_library()

    def refused(code, call, *words):
        with pytest.raises(g.GbnnsError) as e:
            call()
        assert e.value.code == code, (code, str(e.value))
        for wd in ("half-base",) + words:
            assert wd in str(e.value), str(e.value)

    refused(5, lambda: ix.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"]), "GBNNS_MODE_PLAIN")
    refused(5, lambda: ix.exact_knn(c["queries"], 10), "gbnns_index_exact_knn")
    Q = np.full(len(c["queries"]), 0x0F, np.uint32)
    ix.set_tags(tg.row_tags())
    refused(5, lambda: ix.exact_knn(c["queries"], 10, query_tags=Q, gather=True), "gbnns_index_exact_knn_gather")
    refused(5, lambda: ix.search_auto(c["queries"], 64, 10, Q, scan_below=0, mode=g.MODE_LOWQ, queries_low=c["q_low"]), "gbnns_search_tagged_auto")
    refused(1, lambda: ix.search(c["queries"], 64, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], flags=g.FLAG_BYTE_WALK),
            "GBNNS_FLAG_BYTE_WALK")
    # gbnns_search_byte_queries: the binding refuses uint8 queries before the library sees them (TypeError), the library refuses them too
    with pytest.raises(TypeError):
        ix.search(c["queries"].astype(np.uint8), 64, mode=g.MODE_LOWQ, queries_low=c["q_low"])
    with pytest.raises(TypeError):
        ix.search(c["queries"].astype(np.float16), 64, mode=g.MODE_LOWQ, queries_low=c["q_low"])
    qb = np.zeros((4, d), np.uint8)
    ql = np.ascontiguousarray(c["q_low"][:4])
    out = np.empty(4, np.uint32)
    a = g.binding._SearchArgs(struct_size=C.sizeof(g.binding._SearchArgs), mode=g.MODE_LOWQ, ef=8, k=8, mem_kind=g.binding.MEM_HOST, n_q=4,
                              queries=None, queries_low=ql.ctypes.data, out_ids=out.ctypes.data)
    assert lib.gbnns_search_byte_queries(ix._h, C.byref(a), qb.ctypes.data, None, 0, None, None) == 1
    assert b"half-base" in lib.gbnns_last_error()
    ix.close()
    # a half-base handle needs db_low
    with pytest.raises(g.GbnnsError) as e:
        g.Index(c["base"], c["off"], c["nbr"])
    assert e.value.code == 1
    f = g.Index(c["wide"], c["off"], c["nbr"], db_low=c["db_low"])
    assert f.is_half_base is False
    f.close()
