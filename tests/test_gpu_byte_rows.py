"""The byte handle (Index(db=<uint8>), gbnns_index_create_bytes) on an MI355X (run with -m gpu).  The contract: every call returns what the
same call returns on the handle over db.astype(float32), bit for bit.  Every expected value below is the unchanged CPU oracle's on the
widened table -- candidate ids in pop order, the bit patterns of distances, hops, dist_calc, answers, the exact top-k distances -- and
nothing takes a tolerance.  tests/test_byte_rows_cpu.py proves that on every fixture the order of the roundings is visible and that
bit-equal pairs exist, so a kernel that added in another order, sign-extended a byte or broke a tie the other way cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

import bridge_util as bg
import byte_rows_util as bu
import datagen
import golden_util as gu
import half_rows_util as hu
import locality_order_util as lo
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
    assert ix.is_bytes == (table == "base")
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
    """(walk over the low-dimensional table, answers re-ranked on the WIDENED byte table), once per fixture and beam."""
    k = (key, ef, tuple(sorted(kw)))
    if k not in _WALKS:
        w = orc.walk(c["q_low"], c["db_low"] if db_low is None else db_low, c["off"], c["nbr"], ef, entries=kw.pop("entries", c["ent"]), metric=metric,
                     threads=8, **kw)
        _WALKS[k] = (w, orc.rerank(c["queries"], w["ids"], w["count"], c["wide"], metric=metric, threads=8))
    return _WALKS[k]


def _against(r, w, want):
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append("candidate ids (%d rows)" % bu.rows_that_differ(r["cand"], w["ids"]))
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


# ---- 1. the stand-alone kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,metric", bu.RERANK_SHAPES, ids=["d%d_m%d" % s for s in bu.RERANK_SHAPES])
def test_standalone_byte_rerank(g, orc, d, metric):
    """gbnns_rerank and gbnns_rerank_topk (k = 1, 10, 200) over lists of 0 .. 200 candidates: the chunk-pair form (d = 128: eight chunks,
    48: three, 16: one), a lane per row with the d % 4 tail ignored (100, 45), the negative dot with and without its masked tail.  One list
    holds the table's last row; on DEVICE buffers one holds an id >= n, which is read as row 0 and reported as given.  A DEVICE table (borrowed at
    d % 16 == 0, re-laid otherwise) gives the same bytes."""
    import torch
    c = bu.rerank_contest(d, metric)
    rng = tu.rng_of(9850 + d)
    off, nbr = datagen.random_graph(rng, bu.N, 2, 30)
    db_low = datagen.full_mantissa(rng, bu.N, 32)
    q, cand, count = c["queries"], c["cand"], c["count"]
    dist = tu.list_distances(orc, c["wide"], q, cand, count, metric)
    ix = g.Index(c["base"], off, nbr, db_low=db_low, metric=metric)
    assert ix.is_bytes
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
            failures.append("top-%d ids (%d rows)" % (k, bu.rows_that_differ(ids, want_ids)))
        if not np.array_equal(gu.bits(dd), gu.bits(want_dd)):
            failures.append("top-%d distance bits (%d differ)" % (k, int((gu.bits(dd) != gu.bits(want_dd)).sum())))
    # DEVICE buffers, an id outside the table in every list that has a fourth candidate: read as row 0, reported as given
    cand_out = cand.copy()
    has4 = count > 3
    cand_out[has4, 3] = bu.N + 5
    cand_row0 = cand_out.copy()
    cand_row0[has4, 3] = 0
    dist0 = tu.list_distances(orc, c["wide"], q, cand_row0, count, metric)
    want_ids, want_dd = tu.expected_topk(dist0, cand_out, count, 10)
    lib = g.load_library()
    dq, dc, dn = _t(q), _t(cand_out.view(np.int32)), _t(count)
    for table in ("host", "device"):
        ixd = ix if table == "host" else g.Index(_t(c["base"]), off, nbr, db_low=_t(db_low), metric=metric)
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
        if table == "device":
            ids, dd = ixd.rerank_topk(q, cand, 10, count)
            if ids.tobytes() != got[10][0].tobytes() or dd.tobytes() != got[10][1].tobytes():
                failures.append("device table differs from the host table")
            ixd.close()
    ix.close()
    assert not failures, failures


# ---- 2. the fused instances ----------------------------------------------------------------------------------------------------
def test_fused_instances(g, orc):
    """LOWQ on the contest index, L2, d 128, d_low 32: walk_hot_bytes_kernel (ef 8, 64) and walk_hot2_bytes_kernel (100) re-rank their own
    query; ef 200 runs walk_hot_big_kernel and the stand-alone byte kernel.  The launched kernel is byte_plan's."""
    c = bu.index_data(0, 128, 32)
    ix = _index(g, c)
    failures = []
    for ef in bu.BEAMS:
        w, want = _oracle(orc, "contest", c, ef, 0)
        r, launched, p = _search(g, ix, c, ef)
        bad = _against(r, w, want)
        planned, fused = g.byte_plan(0, 32, bu.N, 32, ef)
        if launched != planned:
            bad.append("launched %s, planned %s" % (launched, planned))
        if fused != (ef <= 128):
            bad.append("fused %s" % fused)
        print("byte rows", ef, launched, "fused" if fused else "stand-alone re-rank")
        # the same case in locality order: the fused byte re-rank reads the staged query of the MAPPED work item
        (ro, _, po), in_order = lo.in_order(ix, c["q_low"], lambda: _search(g, ix, c, ef))
        in_order += lo.same_bytes(ro, r, ("ids",) + WANT) + lo.same_kernels(po, p, False)
        bad += ["in order: " + b for b in in_order]
        if bad:
            failures.append((ef, bad))
    ix.close()
    assert not failures, failures


def test_fused_net_mode_and_topk(g, orc):
    c = bu.index_data(0, 128, 32)
    ef, k = 64, 10
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    ix.profile_enable(True)
    s = orc.search_batch(orc_mod.MODE_NET, c["queries"], c["wide"], c["off"], c["nbr"], ef, db_low=c["db_low"], net=c["net"], entries=c["ent"], threads=8)
    w = orc.walk(orc.project(c["net"], c["queries"]), c["db_low"], c["off"], c["nbr"], ef, entries=c["ent"], threads=8)
    r = ix.search(c["queries"], ef, entry_ids=c["ent"], want=WANT + ("q_low",), top_k=k)
    p = ix.profile_read(reset=True)
    assert p["walk_kernel"].split(" (")[0] == "walk_hot_bytes_kernel", p["walk_kernel"]
    assert np.array_equal(r["ids"], s["ids"]) and np.array_equal(r["hops"], s["hops"]) and np.array_equal(r["dist_calc"] + ef, s["dist_calc"])
    assert np.array_equal(r["cand"], w["ids"]) and np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"]))
    assert np.array_equal(gu.bits(ix.project(c["queries"])), gu.bits(orc.project(c["net"], c["queries"])))
    dist = tu.list_distances(orc, c["wide"], c["queries"], w["ids"], w["count"], 0)
    want_ids, want_dist = tu.expected_topk(dist, w["ids"], w["count"], k)
    assert np.array_equal(r["top_ids"], want_ids) and np.array_equal(gu.bits(r["top_dist"]), gu.bits(want_dist))
    assert np.array_equal(r["top_ids"][:, 0], s["ids"])
    # LOWQ with top_k, through the fused kernel too
    w2, want2 = _oracle(orc, "contest", c, ef, 0)
    r2 = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=WANT, top_k=k)
    assert not _against(r2, w2, want2)
    d2 = tu.list_distances(orc, c["wide"], c["queries"], w2["ids"], w2["count"], 0)
    ids2, dist2 = tu.expected_topk(d2, w2["ids"], w2["count"], k)
    assert np.array_equal(r2["top_ids"], ids2) and np.array_equal(gu.bits(r2["top_dist"]), gu.bits(dist2))
    ix.close()


def test_fused_integer_queries(g, orc):
    """The real SIFT case: integer queries, every sum exact, every row of a group at the same distance -- the pop index alone decides."""
    c = bu.index_data(0, 128, 32, integer=True)
    ix = _index(g, c)
    for ef in (64, 100):
        w, want = _oracle(orc, "integer", c, ef, 0)
        r, launched, _ = _search(g, ix, c, ef)
        assert launched == ("walk_hot_bytes_kernel" if ef <= 64 else "walk_hot2_bytes_kernel"), launched
        assert not _against(r, w, want), (ef, _against(r, w, want))
        # (all candidates tie: getRealNearest keeps the first popped)
        assert np.array_equal(r["ids"], w["ids"][:, 0])
    ix.close()


# ---- 3. hand-overs ---------------------------------------------------------------------------------------------------------------
def test_hand_overs_go_to_the_general_byte_kernel(g, orc):
    c = bu.index_data(0, 128, 32)
    ix = _index(g, c)
    for ef in (64, 100):
        w, want = _oracle(orc, "contest", c, ef, 0)
        r, launched, p = _search(g, ix, c, ef, hash_capacity=128)
        assert launched == ("walk_hot_bytes_kernel" if ef <= 64 else "walk_hot2_bytes_kernel"), launched
        assert p["general_queries"] > 0 and p["retry_kernel"] == "", p
        assert not _against(r, w, want), (ef, _against(r, w, want))
    ix.close()


# ---- 4. the unfused domain -------------------------------------------------------------------------------------------------------
def _both(g, c, metric=0, half=False):
    b, f = _index(g, c, metric), _index(g, c, metric, table="wide")
    if half:
        b.enable_half_rows()
        f.enable_half_rows()
    return b, f


def _pair_check(g, what, failures, b, f, c, ef, w, want, **kw):
    rb, kb, _ = _search(g, b, c, ef, **kw)
    rf, kf, _ = _search(g, f, c, ef, **kw)
    bad = _against(rb, w, want)
    if kb != kf:
        bad.append("first pass %s, a float handle's %s" % (kb, kf))
    if _same_bytes(rb, rf):
        bad.append("differs from the float handle in %s" % _same_bytes(rb, rf))
    print("byte rows, unfused:", what, kb)
    if bad:
        failures.append((what, bad))


def test_unfused_domain_runs_the_float_handles_kernel(g, orc):
    failures = []
    c = bu.index_data(0, 128, 32)
    b, f = _both(g, c, half=True)
    w, want = _oracle(orc, "contest", c, 64, 0)
    _pair_check(g, "no fused re-rank", failures, b, f, c, 64, w, want, flags=g.FLAG_NO_FUSED_RERANK)
    R = hu.rounded(c["db_low"])
    wr, wantr = _oracle(orc, "contest_R", c, 64, 0, db_low=R)
    _pair_check(g, "half rows", failures, b, f, c, 64, wr, wantr, flags=g.FLAG_HALF_ROWS)
    ent2 = np.stack([c["ent"], (c["ent"] // bu.PER) * bu.PER + (c["ent"] % bu.PER + 101) % bu.PER], axis=1).astype(np.uint32)
    w2, want2 = _oracle(orc, "contest_ent2", c, 64, 0, entries=ent2)
    _pair_check(g, "two entry points", failures, b, f, c, 64, w2, want2, entry_ids=ent2)
    # tagged calls: every row allowed; half the rows allowed (the oracle on cut_graph); bridged (on bridge_graph)
    T = tg.row_tags()
    rng = tu.rng_of(9950)
    pools = [np.arange(q * bu.PER, (q + 1) * bu.PER) for q in c["qg"]]
    cw = dict(c, base=c["wide"])
    for ix in (b, f):
        ix.set_tags(T)
    for what, qv, flags, exp in (("every row allowed", tg.ALL, 0, tg.expected), ("half the rows allowed", 0x0F, 0, tg.expected),
                                 ("bridged", 0x0F, g.FLAG_TAG_BRIDGE, bg.expected)):
        Q = np.full(len(c["qg"]), qv, np.uint32)
        ent = tg.allowed_entries(rng, T, Q, pools)
        e = exp(orc, cw, 64, 0, T=T, Q=Q, ent=ent)
        _pair_check(g, "tagged, " + what, failures, b, f, c, 64, dict(ids=e["ids"], dists=e["dists"], hops=e["hops"], dist_calc=e["dist_calc"]), e["want"],
                    entry_ids=ent, query_tags=Q, flags=flags)
    b.close()
    f.close()
    for what, metric, dlow in (("d_low 48", 0, 48), ("negative dot", 1, 32)):
        c = bu.index_data(metric, 128, dlow)
        b, f = _both(g, c, metric)
        for ef in (64, 100):
            w, want = _oracle(orc, what, c, ef, metric)
            _pair_check(g, "%s ef %d" % (what, ef), failures, b, f, c, ef, w, want)
        b.close()
        f.close()
    assert not failures, failures


def test_batches_in_flight_on_device_buffers(g, orc):
    """GBNNS_FLAG_DEFER_JOIN with depth 3 on torch tensors, the byte table a borrowed torch.uint8 tensor: three distinct batches rotate over
    nine calls; after join and synchronise every call's outputs equal the synchronous HOST result of its batch, which equals the oracle.
    (No kernel name here: profiling serialises a handle's calls, so a profiled call is never in flight.)"""
    import torch
    c = bu.index_data(0, 128, 32)
    ef = 64
    rng = tu.rng_of(9960)
    batches = []
    for _ in range(3):
        q_low = datagen.full_mantissa(rng, len(c["qg"]), 32)
        ent = (c["qg"] * bu.PER + rng.integers(0, bu.PER, size=len(c["qg"]))).astype(np.uint32)
        batches.append((q_low, ent))
    ix = g.Index(_t(c["base"]), c["off"], c["nbr"], db_low=_t(c["db_low"]))
    assert ix.is_bytes
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


# ---- 5. a byte handle is the float handle ----------------------------------------------------------------------------------------
def test_byte_handle_equals_float_handle(g):
    c = bu.index_data(0, 128, 32)
    rc = bu.rerank_contest(128, 0)
    b = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    f = g.Index(c["wide"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    assert b.is_bytes and not f.is_bytes
    for ef in (64, 100, 200):
        for kw in (dict(), dict(top_k=10), dict(mode=g.MODE_LOWQ, queries_low=c["q_low"]), dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], top_k=10)):
            rb = b.search(c["queries"], ef, entry_ids=c["ent"], want=WANT, **kw)
            rf = f.search(c["queries"], ef, entry_ids=c["ent"], want=WANT, **kw)
            names = ("ids",) + WANT + (("top_ids", "top_dist") if "top_k" in kw else ())
            assert not _same_bytes(rb, rf, names), (ef, sorted(kw), _same_bytes(rb, rf, names))
    b.close()
    f.close()
    # rerank_topk: the contest lists against the float handle over the same rows (any graph will do)
    b = g.Index(rc["base"], c["off"], c["nbr"], db_low=c["db_low"])
    f = g.Index(rc["wide"], c["off"], c["nbr"], db_low=c["db_low"])
    for k in (1, 10, 200):
        ib, db_ = b.rerank_topk(rc["queries"], rc["cand"], k, rc["count"])
        i_f, df = f.rerank_topk(rc["queries"], rc["cand"], k, rc["count"])
        assert ib.tobytes() == i_f.tobytes() and db_.tobytes() == df.tobytes(), k
    assert b.rerank(rc["queries"], rc["cand"], rc["count"]).tobytes() == f.rerank(rc["queries"], rc["cand"], rc["count"]).tobytes()
    b.close()
    f.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(g):
    c = bu.index_data(0, 128, 32)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"])
    with pytest.raises(g.GbnnsError) as e:
        ix.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"])
    assert e.value.code == 5   # GBNNS_ERR_UNSUPPORTED
    ix.close()
    with pytest.raises(g.GbnnsError) as e:
        g.Index(c["base"], c["off"], c["nbr"])
    assert e.value.code == 1   # GBNNS_ERR_INVALID: a byte handle needs db_low
    f = g.Index(c["wide"], c["off"], c["nbr"], db_low=c["db_low"])
    assert f.is_bytes is False
    f.close()
