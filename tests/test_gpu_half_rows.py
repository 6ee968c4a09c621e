"""GBNNS_FLAG_HALF_ROWS on an MI355X (run with -m gpu).  The contract: a flagged search is the reference's search on the table
R = float32(float16(db_low)).  Every expected value below is the CPU oracle's on NumPy's R -- candidate ids in pop order, the bit
patterns of their distances, hops, dist_calc, answers -- and nothing takes a tolerance.  tests/test_half_rows_cpu.py proves that on
each fixture the walk over R differs from the walk over db_low, so a kernel that gathered the wrong table cannot pass.
"""
import numpy as np
import pytest

import datagen
import golden_util as gu
import half_rows_util as hu
import locality_order_util as lo
import oracle as orc_mod
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


_WALKS = {}


def _oracle(orc, key, c, ef, metric, table="R", **kw):
    """(walk over c[table], re-ranked answers), computed once per fixture and beam."""
    k = (key, table, ef, tuple(sorted(kw)))
    if k not in _WALKS:
        w = orc.walk(c["q_low"], c[table], c["off"], c["nbr"], ef, entries=kw.pop("entries", c["ent"]), metric=metric, threads=8, **kw)
        _WALKS[k] = (w, orc.rerank(c["queries"], w["ids"], w["count"], c["base"], metric=metric, threads=8))
    return _WALKS[k]


def _against(r, w, want):
    bad = []
    if not np.array_equal(r["cand"], w["ids"]):
        bad.append("candidate ids (%d rows)" % hu.rows_that_differ(r["cand"], w["ids"]))
    if not np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])):
        bad.append("distance bits (%d differ)" % int((gu.bits(r["cand_dist"]) != gu.bits(w["dists"])).sum()))
    if not np.array_equal(r["hops"], w["hops"]):
        bad.append("hops")
    if not np.array_equal(r["dist_calc"], w["dist_calc"]):
        bad.append("dist_calc")
    if not np.array_equal(r["ids"], want):
        bad.append("answers (%d differ)" % int((r["ids"] != want).sum()))
    return bad


def _flagged(g, ix, c, ef, flags=0, **kw):
    """One profiled flagged LOWQ search -> (results, name of the first-pass kernel, profile)."""
    ix.profile_read(reset=True)
    kw.setdefault("entry_ids", c["ent"])
    r = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], want=WANT, flags=flags | g.FLAG_HALF_ROWS, **kw)
    p = ix.profile_read(reset=True)
    return r, p["walk_kernel"].split(" (")[0], p


def _index(g, c, metric, **kw):
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric, **kw)
    ix.enable_half_rows()
    ix.profile_enable(True)
    ix.knob("coop", 0)   # (at 96 queries the auto rule takes the two-wavefront walk at ef 200)
    return ix


# ---- 1. every half instance, by name and bit-exact -------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d,dlow", hu.SHAPES, ids=["m%d_d%d_low%d" % s for s in hu.SHAPES])
def test_half_instances_on_the_contest_indexes(g, orc, metric, d, dlow):
    """One-pass adjacency rows: the one-register list (ef 8, 64), the two-register list (100) and the two-list kernel (200) of every
    walked width; 576-byte rows take the float32 instance on R up to ef 128, and at ef 200 both orders of the row requests."""
    c = hu.contest(metric, d, dlow)
    ix = _index(g, c, metric)
    failures = []
    for ef in hu.BEAMS:
        w, want = _oracle(orc, ("contest", metric, d, dlow), c, ef, metric)
        for late in ((0, 1) if (dlow == 144 and ef > 128) else (0,)):
            ix.knob("late_rows", late)
            r, launched, p = _flagged(g, ix, c, ef)
            bad = _against(r, w, want)
            planned = hu.half_kernel(metric, dlow, ef, True, late=bool(late))
            if launched != planned:
                bad.append("launched %s, expected %s" % (launched, planned))
            print("half rows", (metric, d, dlow, ef, late), launched)
            (ro, _, po), in_order = lo.in_order(ix, c["q_low"], lambda: _flagged(g, ix, c, ef))   # the same case in locality order
            in_order += lo.same_bytes(ro, r, ("ids",) + WANT) + lo.same_kernels(po, p, False)
            bad += ["in order: " + b for b in in_order]
            if bad:
                failures.append(((metric, d, dlow, ef, late), bad))
    ix.close()
    assert not failures, failures


@pytest.mark.parametrize("metric,dlow", hu.TWO_PASS_SHAPES, ids=["m%d_low%d" % s for s in hu.TWO_PASS_SHAPES])
def test_half_instances_on_two_pass_adjacency_rows(g, orc, metric, dlow):
    """Adjacency rows of 33 .. 48 slots: the instances with the pass loop."""
    c = hu.two_pass(metric, dlow)
    ix = _index(g, c, metric)
    failures = []
    for ef in hu.BEAMS:
        w, want = _oracle(orc, ("two_pass", metric, dlow), c, ef, metric)
        for late in ((0, 1) if (dlow == 144 and ef > 128) else (0,)):
            ix.knob("late_rows", late)
            r, launched, p = _flagged(g, ix, c, ef)
            bad = _against(r, w, want)
            planned = hu.half_kernel(metric, dlow, ef, False, late=bool(late))
            if launched != planned:
                bad.append("launched %s, expected %s" % (launched, planned))
            print("half rows, two passes", (metric, dlow, ef, late), launched)
            (ro, _, po), in_order = lo.in_order(ix, c["q_low"], lambda: _flagged(g, ix, c, ef))   # the same case in locality order
            in_order += lo.same_bytes(ro, r, ("ids",) + WANT) + lo.same_kernels(po, p, False)
            bad += ["in order: " + b for b in in_order]
            if bad:
                failures.append(((metric, dlow, ef, late), bad))
    ix.close()
    assert not failures, failures


# ---- 2. everything outside the domain walks R too ---------------------------------------------------------------------------
def test_everything_outside_the_domain_walks_r(g, orc):
    metric, d, dlow = 0, 128, 32
    c = hu.contest(metric, d, dlow)
    ix = _index(g, c, metric)
    key = ("contest", metric, d, dlow)
    failures = []

    def check(what, ef, r, launched, w, want, expect_prefix):
        bad = _against(r, w, want)
        if not launched.startswith(expect_prefix):
            bad.append("launched %s, expected %s..." % (launched, expect_prefix))
        print("half rows, outside the domain:", what, launched)
        if bad:
            failures.append((what, bad))

    # a visited set too small: the half first pass hands over to the float32 retry and general passes
    w, want = _oracle(orc, key, c, 64, metric)
    r, launched, p = _flagged(g, ix, c, 64, hash_capacity=128)
    check("hash_capacity 128", 64, r, launched, w, want, "walk_reg_half_kernel<0, 8, 1, true>")
    assert p["retry_queries"] > 0, p
    assert p["retry_kernel"].startswith("walk_reg_kernel<0, 8, true, true, 1,"), p["retry_kernel"]
    w, want = _oracle(orc, key, c, 200, metric)
    r, launched, _ = _flagged(g, ix, c, 200, flags=g.FLAG_BITMAP_PASS)
    check("bitmap pass", 200, r, launched, w, want, "walk_bitmap_big_kernel<0, 8,")
    ix.knob("coop", 1)
    r, launched, _ = _flagged(g, ix, c, 200)
    check("two-wavefront walk", 200, r, launched, w, want, "walk_coop_kernel<8,")
    ix.knob("coop", 0)
    for ef in (64, 200):
        w, want = _oracle(orc, key, c, ef, metric)
        r, launched, _ = _flagged(g, ix, c, ef, flags=g.FLAG_WIDE_INDEX)
        check("wide index ef %d" % ef, ef, r, launched, w, want, "walk_reg_kernel<0, 8, false," if ef == 64 else "walk_reg_big_kernel<0, 8, false,")
    w, want = _oracle(orc, key, c, 1100, metric)
    r, launched, _ = _flagged(g, ix, c, 1100)
    check("LDS list", 1100, r, launched, w, want, "walk_fast_kernel<0, 8,")
    w, want = _oracle(orc, key, c, 64, metric)
    r, launched, _ = _flagged(g, ix, c, 64, flags=g.FLAG_NO_FUSED_RERANK)
    check("re-rank in its own launch", 64, r, launched, w, want, "walk_reg_half_kernel<0, 8, 1, true>")
    # two entry points per query (the second one another row of the query's component): the general kernel takes the batch
    ent2 = np.stack([c["ent"], (c["ent"] // tu.PER) * tu.PER + (c["ent"] % tu.PER + 101) % tu.PER], axis=1).astype(np.uint32)
    w, want = _oracle(orc, key + ("ent2",), c, 64, metric, entries=ent2)
    r, launched, _ = _flagged(g, ix, c, 64, entry_ids=ent2)
    check("two entry points", 64, r, launched, w, want, "walk_general_kernel")
    # the auxiliary graph: the float32 hop with the auxiliary rows
    aux = datagen.contest_graph(tu.rng_of(8801), tu.GROUPS, tu.PER, 0, 6)
    ix.set_aux_graph(*aux)
    w = orc.walk(c["q_low"], c["R"], c["off"], c["nbr"], 64, entries=c["ent"], metric=metric, threads=8, aux=aux, llf=True, hops_bound=50)
    want = orc.rerank(c["queries"], w["ids"], w["count"], c["base"], metric=metric, threads=8)
    r, launched, _ = _flagged(g, ix, c, 64, aux=True, llf=True, hops_bound=50)
    check("auxiliary graph", 64, r, launched, w, want, "walk_reg_kernel<0, 8, true, false, 1, false, true>")
    ix.close()
    assert not failures, failures


# ---- 3. an exactly representable table --------------------------------------------------------------------------------------
def test_exactly_representable_table_gives_identical_bytes(g, orc):
    """db_low = multiples of 1 / 256: R == db_low, so flagged and unflagged searches return the same bytes in every output -- the
    equal-distance ties such data holds (tests/test_half_rows_cpu.py counts the lists that have some) included -- while the flagged one
    gathers 2-byte rows."""
    c = hu.clustered_index()
    ix = _index(g, c, 0)
    for ef in hu.BEAMS:
        w, want = _oracle(orc, ("clustered", 32), c, ef, 0, table="db_low")
        r, launched, _ = _flagged(g, ix, c, ef)
        plain = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=WANT)
        assert launched == hu.half_kernel(0, 32, ef, True), (ef, launched)
        for name in ("ids",) + WANT:
            assert r[name].tobytes() == plain[name].tobytes(), (ef, name)
        assert not _against(r, w, want), (ef, _against(r, w, want))
    ix.close()


# ---- 4. binary16 subnormals survive -----------------------------------------------------------------------------------------
def test_binary16_subnormals_survive(g, orc):
    """One component's rows are small multiples of 2^-24; the queries that enter it must get the oracle's rows on R -- which differ,
    for every one of them, from its rows on R with those values flushed to zero (tests/test_half_rows_cpu.py)."""
    c = hu.subnormal_index()
    ix = _index(g, c, 0)
    sub = c["sub_queries"]
    for ef in (8, 64, 200):
        w, want = _oracle(orc, ("subnormal",), c, ef, 0)
        r, launched, _ = _flagged(g, ix, c, ef)
        assert launched == hu.half_kernel(0, 32, ef, True), (ef, launched)
        assert not _against(r, w, want), (ef, _against(r, w, want))
        if ef <= 64:
            f, _ = _oracle(orc, ("subnormal",), c, ef, 0, table="R_flushed")
            assert hu.rows_that_differ(r["cand"][sub], f["ids"][sub]) == len(sub), ef
    assert np.array_equal(gu.bits(ix.low_rows()), gu.bits(c["R"]))
    ix.close()


# ---- 5. NET mode and top-k --------------------------------------------------------------------------------------------------
def test_net_mode_and_topk(g, orc):
    metric, d, dlow, ef, k = 0, 128, 32, 64, 10
    c = hu.contest(metric, d, dlow)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"], metric=metric)
    ix.enable_half_rows()
    s = orc.search_batch(orc_mod.MODE_NET, c["queries"], c["base"], c["off"], c["nbr"], ef, db_low=c["R"], net=c["net"], entries=c["ent"],
                         metric=metric, threads=8)
    w = orc.walk(orc.project(c["net"], c["queries"]), c["R"], c["off"], c["nbr"], ef, entries=c["ent"], metric=metric, threads=8)
    r = ix.search(c["queries"], ef, entry_ids=c["ent"], want=WANT + ("q_low",), flags=g.FLAG_HALF_ROWS, top_k=k)
    plain = ix.search(c["queries"], ef, entry_ids=c["ent"], want=WANT + ("q_low",))
    assert np.array_equal(r["ids"], s["ids"]) and np.array_equal(r["hops"], s["hops"]) and np.array_equal(r["dist_calc"] + ef, s["dist_calc"])
    assert np.array_equal(r["cand"], w["ids"]) and np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"]))
    assert r["q_low"].tobytes() == plain["q_low"].tobytes(), "the query is never rounded"
    assert hu.rows_that_differ(r["cand"], plain["cand"]) >= 24
    dist = tu.list_distances(orc, c["base"], c["queries"], w["ids"], w["count"], metric)
    want_ids, want_dist = tu.expected_topk(dist, w["ids"], w["count"], k)
    assert np.array_equal(r["top_ids"], want_ids) and np.array_equal(gu.bits(r["top_dist"]), gu.bits(want_dist))
    assert np.array_equal(r["top_ids"][:, 0], s["ids"])
    ix.close()


# ---- 6. low_rows: the device conversion is gbnns_round_to_half ---------------------------------------------------------------
@pytest.mark.parametrize("dlow", [32, 30], ids=["low32", "low30_padded"])
def test_low_rows_equals_the_round_trip(g, dlow):
    """A table that holds the edge list (ties to even both ways, the subnormal range and the tie below it, both zeros, the largest finite
    value and its upper neighbours) beside full-mantissa rows, HOST-created and DEVICE-borrowed: low_rows() equals NumPy's round trip
    and gbnns_round_to_half's widened output, bit for bit.  d_low = 30: the handle's rows are padded to 32 floats (a DEVICE table of such
    rows is copied by gbnns_index_create, not borrowed), the 2-byte rows to 32 halves."""
    import torch
    dev = torch.device("cuda:0")
    rng = tu.rng_of(8960 + dlow)
    n = 512
    db_low = datagen.full_mantissa(rng, n, dlow)
    edge_in, _ = hu.edge_values()
    flat = db_low.reshape(-1)
    flat[rng.permutation(flat.size)[:len(edge_in) * 8]] = np.tile(edge_in, 8)
    base = datagen.full_mantissa(rng, n, 40)
    off, nbr = datagen.random_graph(rng, n, 2, 30)
    want = hu.rounded(db_low)
    _, wide = g.round_to_half(db_low)
    assert np.array_equal(gu.bits(wide), gu.bits(want))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for make in (lambda: g.Index(base, off, nbr, db_low=db_low), lambda: g.Index(t(base), off, nbr, db_low=t(db_low))):
        ix = make()
        with pytest.raises(g.GbnnsError):
            ix.low_rows()
        ix.enable_half_rows()
        assert np.array_equal(gu.bits(ix.low_rows()), gu.bits(want))
        got = ix.low_rows(device=True)
        torch.cuda.synchronize()
        assert np.array_equal(gu.bits(got.cpu().numpy()), gu.bits(want))
        ix.close()


# ---- 7. protocol ------------------------------------------------------------------------------------------------------------
def test_protocol(g, orc):
    metric, d, dlow, ef = 0, 128, 32, 64
    c = hu.contest(metric, d, dlow)
    kw = dict(mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"], want=WANT)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric)
    before = ix.search(c["queries"], ef, **kw)
    with pytest.raises(g.GbnnsError) as e:
        ix.search(c["queries"], ef, flags=g.FLAG_HALF_ROWS, **kw)
    assert e.value.code == 1
    ix.enable_half_rows()
    ix.enable_half_rows()   # idempotent
    with pytest.raises(g.GbnnsError) as e:
        ix.search(c["queries"], ef, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"], flags=g.FLAG_HALF_ROWS)
    assert e.value.code == 1
    w, want = _oracle(orc, ("contest", metric, d, dlow), c, ef, metric)
    r = ix.search(c["queries"], ef, flags=g.FLAG_HALF_ROWS, **kw)
    assert not _against(r, w, want)
    after = ix.search(c["queries"], ef, **kw)
    for name in ("ids",) + WANT:
        assert after[name].tobytes() == before[name].tobytes(), name
    ix.close()
    # a table that leaves the binary16 range: refused, the handle keeps serving unflagged searches
    big = c["db_low"].copy()
    big[777, 5] = 70000.0
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=big, metric=metric)
    with pytest.raises(g.GbnnsError) as e:
        ix.enable_half_rows()
    assert e.value.code == 5 and "777" in str(e.value)
    with pytest.raises(g.GbnnsError):
        ix.search(c["queries"], ef, flags=g.FLAG_HALF_ROWS, **kw)
    wb = orc.walk(c["q_low"], big, c["off"], c["nbr"], ef, entries=c["ent"], metric=metric, threads=8)
    assert np.array_equal(ix.search(c["queries"], ef, **kw)["cand"], wb["ids"])
    ix.close()
    # an index without db_low
    ix = g.Index(c["base"], c["off"], c["nbr"], metric=metric)
    with pytest.raises(g.GbnnsError) as e:
        ix.enable_half_rows()
    assert e.value.code == 1
    ix.close()


# ---- 8. device buffers, batches in flight -----------------------------------------------------------------------------------
def test_half_rows_device_buffers_in_flight(g, orc):
    """GBNNS_FLAG_DEFER_JOIN | GBNNS_FLAG_HALF_ROWS with depth 3 on torch tensors: four distinct 96-query batches rotate over 12 calls;
    after join and synchronise every call's outputs equal the synchronous HOST result of its batch, which equals the oracle on R."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    metric, d, dlow, ef = 0, 128, 32, 64
    c = hu.contest(metric, d, dlow)
    rng = tu.rng_of(8970)
    batches = []
    for _ in range(4):
        q_low = datagen.full_mantissa(rng, len(c["qg"]), dlow)
        ent = (c["qg"] * tu.PER + rng.integers(0, tu.PER, size=len(c["qg"]))).astype(np.uint32)
        batches.append((q_low, ent))
    ix = g.Index(t(c["base"]), c["off"], c["nbr"], db_low=t(c["db_low"]), metric=metric)
    ix.enable_half_rows()
    host = [ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=ql, entry_ids=ent, want=WANT, flags=g.FLAG_HALF_ROWS) for ql, ent in batches]
    assert len({h["cand"].tobytes() for h in host}) == 4   # the batches are distinct
    for (ql, ent), h in zip(batches, host):
        w = orc.walk(ql, c["R"], c["off"], c["nbr"], ef, entries=ent, metric=metric, threads=8)
        assert not _against(h, w, orc.rerank(c["queries"], w["ids"], w["count"], c["base"], metric=metric, threads=8))
    q = t(c["queries"])
    dev_in = [(t(ql), t(ent.view(np.int32))) for ql, ent in batches]
    outs = []
    for call in range(12):
        ql, ent = dev_in[call % 4]
        outs.append(ix.search(q, ef, mode=g.MODE_LOWQ, queries_low=ql, entry_ids=ent, out={}, want=WANT, flags=g.FLAG_DEFER_JOIN | g.FLAG_HALF_ROWS,
                              defer_depth=3))
    ix.join()
    torch.cuda.synchronize()
    for call, r in enumerate(outs):
        h = host[call % 4]
        for name in ("ids",) + WANT:
            assert r[name].cpu().numpy().tobytes() == h[name].tobytes(), (call, name)
    ix.close()
