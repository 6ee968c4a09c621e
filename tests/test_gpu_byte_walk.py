"""The byte-row PLAIN walk (MODE_PLAIN with FLAG_BYTE_WALK on a byte handle) on an MI355X (run with -m gpu).  The contract: every output
equals, bit for bit, what the same call without the flag returns on the handle over db.astype(float32).  Every expected value below is the
unchanged CPU oracle's walk over the widened table in the original space -- candidate ids in pop order, the bit patterns of distances, hops,
dist_calc, the k-th best as the answer -- and every case is additionally compared byte for byte (edges included) with the float handle in the
same process.  Nothing takes a tolerance.  tests/test_byte_walk_cpu.py proves that on every fixture the order of the roundings is visible,
that bit-equal pairs exist and that the hand-over case does hand over, so a kernel that added in another order, sign-extended a byte, read
its partner's chunk or broke a tie the other way cannot pass.
"""
import numpy as np
import pytest

import byte_rows_util as bu
import byte_walk_util as bw
import datagen
import topk_util as tu

pytestmark = pytest.mark.gpu

WANT = bw.WANT


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


def _stride(off):
    return max(16, (int(np.diff(off.astype(np.int64)).max()) + 15) // 16 * 16)


def _pair(g, base, off, nbr, db_low, metric=0, profile=True):
    """(byte handle, float handle over the widened table), profile on, the two-wavefront walk off."""
    b = g.Index(base, off, nbr, db_low=db_low, metric=metric)
    f = g.Index(bu.wide(base), off, nbr, db_low=db_low, metric=metric)
    assert b.is_bytes and not f.is_bytes
    for ix in (b, f):
        ix.profile_enable(profile)
        ix.knob("coop", 0)
    return b, f


def _plain(g, ix, queries, ef, k, ent, flags=0, **kw):
    """One profiled PLAIN search -> (results, name of the first-pass kernel, profile)."""
    ix.profile_read(reset=True)
    r = ix.search(queries, ef, mode=g.MODE_PLAIN, k=k, entry_ids=ent, want=WANT, flags=flags, **kw)
    p = ix.profile_read(reset=True)
    return r, p["walk_kernel"].split(" (")[0], p


def _check(g, what, failures, b, f, queries, ef, k, ent, w, planned=None, **kw):
    """The flagged call on the byte handle against the oracle and against the unflagged call on the float handle."""
    flags, float_flags = kw.pop("flags", 0), kw.pop("float_flags", 0)
    rb, kb, pb = _plain(g, b, queries, ef, k, ent, flags=g.FLAG_BYTE_WALK | flags, **kw)
    rf = _plain(g, f, queries, ef, k, ent, flags=float_flags, **kw)[0] if f is not None else None
    bad = bw.against(rb, w)
    if rf is not None and bw.same_bytes(rb, rf):
        bad.append("differs from the float handle in %s" % bw.same_bytes(rb, rf))
    if planned is not None and kb != planned:
        bad.append("launched %s, planned %s" % (kb, planned))
    print("byte walk:", what, "ef", ef, "k", k, kb, "general_queries", pb["general_queries"])
    if bad:
        failures.append((what, ef, k, bad))
    return rb, pb


# ---- 1. the fast instances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["random_one_pass", "random_two_pass", "contest", "contest_integer"])
def test_fast_instances(g, orc, fixture):
    """L2, d = 128, compact index, one entry point: walk_reg_bytes_kernel<1 | 2, ONE_CHUNK> and walk_reg_big_bytes_kernel<ONE_PASS> at ef 8,
    64, 100, 200 with k = ef, the launched kernel the one byte_walk_plan names; k = 1 and 5 at ef 64: the answer is the k-th best."""
    if fixture.startswith("random"):
        c = bw.random_bytes(128)
        off, nbr = c["graphs"][1 if fixture == "random_one_pass" else 2]
        ent = c["ent"]
    else:
        c = bw.contest(0, 128, fixture == "contest_integer")
        off, nbr, ent = c["off"], c["nbr"], c["ent"]
    stride = _stride(off)
    assert (stride <= 32) == (fixture != "random_two_pass")
    b, f = _pair(g, c["base"], off, nbr, c["db_low"])
    failures = []
    for ef, k in [(ef, ef) for ef in bw.BEAMS] + [(64, 1), (64, 5)]:
        w = bw.expected(orc, fixture, c["queries"], c["wide"], off, nbr, ef, k, ent)
        planned = g.byte_walk_plan(0, 128, bw.N, stride, ef)
        assert "bytes_kernel" in planned, planned
        rb, _ = _check(g, fixture, failures, b, f, c["queries"], ef, k, ent, w, planned=planned)
        if k < ef and not np.array_equal(rb["ids"], bw.expected(orc, fixture, c["queries"], c["wide"], off, nbr, ef, ef, ent)["ids"][:, ef - k]):
            failures.append((fixture, ef, k, "the answer is not the k-th best of the full list"))
    b.close()
    f.close()
    assert not failures, failures


# ---- 2. hand-overs -----------------------------------------------------------------------------------------------------------------
def test_hand_overs_go_straight_to_the_general_instance(g, orc):
    """A visited set of 128 entries: at least three quarters of the batch is handed over, there is no retry pass, every output is still
    the oracle's."""
    c = bw.random_bytes(128)
    failures = []
    for graph in (1, 2):
        off, nbr = c["graphs"][graph]
        b, f = _pair(g, c["base"], off, nbr, c["db_low"])
        for ef in (64, 200):
            w = bw.expected(orc, "random_one_pass" if graph == 1 else "random_two_pass", c["queries"], c["wide"], off, nbr, ef, ef, c["ent"])
            _, p = _check(g, "hand-over, graph %d" % graph, failures, b, f, c["queries"], ef, ef, c["ent"], w,
                          planned=g.byte_walk_plan(0, 128, bw.N, _stride(off), ef), hash_capacity=128)
            if p["general_queries"] * 4 < 3 * bw.NQ or p["retry_kernel"] != "":
                failures.append((graph, ef, "general_queries %d, retry_kernel %r" % (p["general_queries"], p["retry_kernel"])))
        b.close()
        f.close()
    assert not failures, failures


# ---- 3. the general kernel's byte-walk instance ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,metric,d", [("d48", 0, 48), ("d100", 0, 100), ("dot_d45", 1, 45), ("dot_d128", 1, 128)])
def test_general_instance_other_shapes(g, orc, what, metric, d):
    """Three chunks, 112-byte rows with the d % 4 tail ignored, the negative dot with and without its masked tail: the contest fixture, and for
    L2 the random bytes of that dimension on both graphs."""
    failures = []
    cases = [("contest", bw.contest(metric, d))]
    if metric == 0:
        r = bw.random_bytes(d)
        cases += [("random graph %d" % gr, dict(r, off=r["graphs"][gr][0], nbr=r["graphs"][gr][1])) for gr in (1, 2)]
    for name, c in cases:
        b, f = _pair(g, c["base"], c["off"], c["nbr"], c["db_low"], metric)
        for ef in (8, 64, 200):
            w = bw.expected(orc, (what, name), c["queries"], c["wide"], c["off"], c["nbr"], ef, ef, c["ent"], metric=metric)
            planned = g.byte_walk_plan(metric, d, bw.N, _stride(c["off"]), ef)
            assert planned == "walk_general_kernel"
            _check(g, "%s %s" % (what, name), failures, b, f, c["queries"], ef, ef, c["ent"], w, planned=planned)
        b.close()
        f.close()
    assert not failures, failures


def test_general_instance_on_d128(g, orc):
    """What takes a d = 128 L2 call out of the fast instances' domain: three entry points per query, the auxiliary graph with and without
    llf and hops_bound, FLAG_WIDE_INDEX, a beam above 1 024."""
    c = bw.random_bytes(128)
    off, nbr = c["graphs"][1]
    rng = tu.rng_of(7790)
    b, f = _pair(g, c["base"], off, nbr, c["db_low"])
    failures = []
    ent3 = np.ascontiguousarray(np.stack([c["ent"], rng.integers(0, bw.N, size=bw.NQ), rng.integers(0, bw.N, size=bw.NQ)], axis=1).astype(np.uint32))
    w = bw.expected(orc, "ent3", c["queries"], c["wide"], off, nbr, 64, 64, ent3)
    _check(g, "three entry points", failures, b, f, c["queries"], 64, 64, ent3, w, planned="walk_general_kernel")
    aux = datagen.random_graph(rng, bw.N, 0, 20)
    for ix in (b, f):
        ix.set_aux_graph(aux[0], aux[1])
    for llf, hb in ((False, 50), (True, 50), (True, 3)):
        w = bw.expected(orc, "aux", c["queries"], c["wide"], off, nbr, 64, 64, c["ent"], aux=aux, llf=llf, hops_bound=hb)
        _check(g, "auxiliary graph llf %s hops_bound %d" % (llf, hb), failures, b, f, c["queries"], 64, 64, c["ent"], w, planned="walk_general_kernel",
               aux=True, llf=llf, hops_bound=hb)
    for ix in (b, f):
        ix.set_aux_graph(None, None)
    w = bw.expected(orc, "random_one_pass", c["queries"], c["wide"], off, nbr, 64, 64, c["ent"])
    _check(g, "wide index", failures, b, f, c["queries"], 64, 64, c["ent"], w, planned="walk_general_kernel", flags=g.FLAG_WIDE_INDEX,
           float_flags=g.FLAG_WIDE_INDEX)
    # (FLAG_BITMAP_PASS is ignored by a flagged call: the fast instance, the same outputs)
    _check(g, "bitmap pass flag", failures, b, None, c["queries"], 64, 64, c["ent"], w, planned=g.byte_walk_plan(0, 128, bw.N, _stride(off), 64),
           flags=g.FLAG_BITMAP_PASS)
    w = bw.expected(orc, "random_one_pass", c["queries"], c["wide"], off, nbr, 1100, 1100, c["ent"])
    _check(g, "ef 1 100", failures, b, f, c["queries"], 1100, 1100, c["ent"], w, planned="walk_general_kernel")
    b.close()
    f.close()
    assert not failures, failures


# ---- 4. buffers and flight ---------------------------------------------------------------------------------------------------------
def test_device_buffers_and_batches_in_flight(g, orc):
    """DEVICE tensors in and out (the byte table a borrowed torch.uint8 tensor); three FLAG_DEFER_JOIN batches in flight with rotating
    buffers give byte-identical outputs to the synchronous HOST call of their batch, which is the oracle's; FLAG_SERIAL too; an entry id >= n
    in a DEVICE buffer gives the bad-entry row."""
    import torch
    c = bw.random_bytes(128)
    off, nbr = c["graphs"][1]
    ef = 64
    rng = tu.rng_of(7791)
    ix = g.Index(_t(c["base"]), off, nbr, db_low=_t(c["db_low"]))
    assert ix.is_bytes
    ix.knob("coop", 0)
    batches = [(np.ascontiguousarray(c["queries"][rng.permutation(bw.NQ)]), rng.integers(0, bw.N, size=bw.NQ).astype(np.uint32)) for _ in range(3)]
    host = []
    for i, (q, ent) in enumerate(batches):
        h = ix.search(q, ef, mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=WANT, flags=g.FLAG_BYTE_WALK)
        assert not bw.against(h, bw.expected(orc, ("flight", i), q, c["wide"], off, nbr, ef, ef, ent)), i
        s = ix.search(q, ef, mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=WANT, flags=g.FLAG_BYTE_WALK | g.FLAG_SERIAL)
        assert not bw.same_bytes(h, s), i
        host.append(h)
    assert len({h["cand"].tobytes() for h in host}) == 3
    dev_in = [(_t(q), _t(ent.view(np.int32))) for q, ent in batches]
    outs = [ix.search(dev_in[call % 3][0], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=dev_in[call % 3][1], out={}, want=WANT,
                      flags=g.FLAG_BYTE_WALK | g.FLAG_DEFER_JOIN, defer_depth=3) for call in range(9)]
    ix.join()
    torch.cuda.synchronize()
    for call, r in enumerate(outs):
        for name in ("ids",) + WANT:
            assert r[name].cpu().numpy().tobytes() == host[call % 3][name].tobytes(), (call, name)
    # a bad entry id in a DEVICE buffer: data, not an error -- the all-0xFFFFFFFF row for that query, the others untouched
    q, ent = batches[0]
    bad = ent.copy()
    bad[5] = bw.N
    bad[17] = 0xFFFFFFF0
    for ef2 in (64, 200):
        want = bw.expected(orc, ("flight", 0), q, c["wide"], off, nbr, ef2, ef2, ent)
        r = ix.search(_t(q), ef2, mode=g.MODE_PLAIN, k=ef2, entry_ids=_t(bad.view(np.int32)), want=WANT, flags=g.FLAG_BYTE_WALK)
        torch.cuda.synchronize()
        r = {n: v.cpu().numpy() for n, v in r.items()}
        ok = np.ones(bw.NQ, bool)
        ok[[5, 17]] = False
        assert np.array_equal(r["cand"].view(np.uint32)[ok], want["ids"][ok]) and np.array_equal(r["ids"].view(np.uint32)[ok], want["want"][ok])
        for i in (5, 17):
            assert (r["cand"].view(np.uint32)[i] == bw.NONE).all() and r["ids"].view(np.uint32)[i] == bw.NONE
            assert r["hops"][i] == 0 and r["dist_calc"][i] == 0 and r["edges"][i] == 0 and np.isinf(r["cand_dist"][i]).all()
    ix.close()


# ---- 5. tagged -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [(0, 128), (1, 45)])
def test_tagged_and_bridged(g, orc, metric, d):
    """query_tags with half the rows allowed, cut and bridged: the oracle on cut_graph's / bridge_graph's CSR over the widened table; with
    every tag set: the untagged flagged call, counters and edges included."""
    import tag_util as tg
    c = bw.contest(metric, d)
    T = tg.row_tags()
    rng = tu.rng_of(7792 + d)
    pools = [np.arange(q * bu.PER, (q + 1) * bu.PER) for q in c["qg"]]
    b, f = _pair(g, c["base"], c["off"], c["nbr"], c["db_low"], metric)
    for ix in (b, f):
        ix.set_tags(T)
    failures = []
    ef = 64
    Q = np.full(bw.NQ, 0x0F, np.uint32)
    ent = tg.allowed_entries(rng, T, Q, pools)
    allowed = (T & 0x0F) != 0
    assert 0.3 < allowed.mean() < 0.7
    for what, graph_of, flags in (("cut", g.cut_graph, 0), ("bridged", g.bridge_graph, g.FLAG_TAG_BRIDGE)):
        off2, nbr2 = graph_of(c["off"], c["nbr"], allowed)
        w = bw.expected(orc, ("tagged", what, metric, d), c["queries"], c["wide"], off2, nbr2, ef, ef, ent, metric=metric)
        assert g.byte_walk_plan(metric, d, bw.N, _stride(c["off"]), ef, tagged=True) == "walk_general_kernel"
        _check(g, "tagged, " + what, failures, b, f, c["queries"], ef, ef, ent, w, planned="walk_general_kernel", query_tags=Q, flags=flags,
               float_flags=flags)
    every = np.full(bw.NQ, tg.ALL, np.uint32)
    w = bw.expected(orc, ("untagged", metric, d), c["queries"], c["wide"], c["off"], c["nbr"], ef, ef, c["ent"], metric=metric)
    plain, _, _ = _plain(g, b, c["queries"], ef, ef, c["ent"], flags=g.FLAG_BYTE_WALK)
    for flags in (0, g.FLAG_TAG_BRIDGE):
        rb, _ = _check(g, "every tag set", failures, b, f, c["queries"], ef, ef, c["ent"], w, query_tags=every, flags=flags, float_flags=flags)
        if bw.same_bytes(rb, plain):
            failures.append(("every tag set", flags, "differs from the untagged flagged call in %s" % bw.same_bytes(rb, plain)))
    b.close()
    f.close()
    assert not failures, failures


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(g):
    c = bw.contest(0, 128)
    b = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    f = g.Index(c["wide"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])

    def code(ix, **kw):
        with pytest.raises(g.GbnnsError) as e:
            ix.search(c["queries"], 64, entry_ids=c["ent"], **kw)
        return e.value.code

    assert code(f, mode=g.MODE_PLAIN, k=1, flags=g.FLAG_BYTE_WALK) == 1                          # the flag on a float handle
    assert code(b, mode=g.MODE_LOWQ, queries_low=c["q_low"], flags=g.FLAG_BYTE_WALK) == 1        # ... with LOWQ
    assert code(b, mode=g.MODE_NET, flags=g.FLAG_BYTE_WALK) == 1                                 # ... with NET
    with pytest.raises(g.GbnnsError) as e:
        b.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"])
    assert e.value.code == 5 and "GBNNS_FLAG_BYTE_WALK" in str(e.value)                          # PLAIN without the flag: still unsupported
    assert code(b, mode=g.MODE_PLAIN, k=64, flags=g.FLAG_BYTE_WALK, top_k=5) == 1                # top_k with PLAIN: still invalid
    assert code(f, mode=g.MODE_PLAIN, k=64, top_k=5) == 1
    assert code(b, mode=g.MODE_PLAIN, k=1, flags=g.FLAG_BYTE_WALK | g.FLAG_HALF_ROWS) == 1       # half rows with PLAIN: still invalid
    # ... and the handles still serve
    r = b.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"], flags=g.FLAG_BYTE_WALK)
    assert np.array_equal(r["ids"], f.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"])["ids"])
    b.close()
    f.close()
