"""The half-row PLAIN walk (MODE_PLAIN with FLAG_HALF_WALK on a half-base handle) on an MI355X (run with -m gpu).  The contract: every output
equals, bit for bit, what the same call without the flag returns on the handle over db.astype(float32).  Every expected value below is the
unchanged CPU oracle's walk over the widened table in the original space -- candidate ids in pop order, the bit patterns of distances, hops,
dist_calc, the k-th best as the answer -- and every case is additionally compared byte for byte (edges included) with the float handle in the
same process.  Nothing takes a tolerance.  tests/test_half_walk_cpu.py proves that on every fixture the order of the roundings is visible,
that bit-equal pairs exist and that the hand-over cases do hand over, so a kernel that added in another order, read its partner's chunk,
read past a row's padding or broke a tie the other way cannot pass.
"""
import numpy as np
import pytest

import datagen
import half_base_util as hb
import half_walk_util as hw
import topk_util as tu

pytestmark = pytest.mark.gpu

WANT = hw.WANT


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


def _pair(g, base, off, nbr, db_low, metric=0, net=None):
    """(half-base handle, float handle over the widened table), profile on, the two-wavefront walk off."""
    h = g.Index(base, off, nbr, db_low=db_low, metric=metric, net=net)
    f = g.Index(hb.wide(base), off, nbr, db_low=db_low, metric=metric, net=net)
    assert h.is_half_base and not f.is_half_base
    for ix in (h, f):
        ix.profile_enable(True)
        ix.knob("coop", 0)
    h.knob("half_walk_fast", 2)   # every fast instance, as half_walk_plan reports: also those of a class the default leaves to the general instance
    return h, f


def _plain(g, ix, queries, ef, k, ent, flags=0, **kw):
    """One profiled PLAIN search -> (results, name of the first-pass kernel, profile)."""
    ix.profile_read(reset=True)
    r = ix.search(queries, ef, mode=g.MODE_PLAIN, k=k, entry_ids=ent, want=WANT, flags=flags, **kw)
    p = ix.profile_read(reset=True)
    return r, p["walk_kernel"].split(" (")[0], p


def _check(g, what, failures, h, f, queries, ef, k, ent, w, planned=None, **kw):
    """The flagged call on the half-base handle against the oracle and against the unflagged call on the float handle."""
    flags, float_flags = kw.pop("flags", 0), kw.pop("float_flags", 0)
    rh, kh, ph = _plain(g, h, queries, ef, k, ent, flags=g.FLAG_HALF_WALK | flags, **kw)
    rf = _plain(g, f, queries, ef, k, ent, flags=float_flags, **kw)[0] if f is not None else None
    bad = hw.against(rh, w)
    if rf is not None and hw.same_bytes(rh, rf):
        bad.append("differs from the float handle in %s" % hw.same_bytes(rh, rf))
    if planned is not None and kh != planned:
        bad.append("launched %s, planned %s" % (kh, planned))
    print("half walk:", what, "ef", ef, "k", k, kh, "general_queries", ph["general_queries"])
    if bad:
        failures.append((what, ef, k, bad))
    return rh, ph


def _cases(d, kinds):
    """(name, fixture with off / nbr / ent) of dimension d: "contest" and / or the random halves over both graphs."""
    out = []
    if "contest" in kinds:
        out.append(("contest", hw.contest(0, d)))
    if "random" in kinds:
        r = hw.random_halves(d)
        out += [("random graph %d" % gr, dict(r, off=r["graphs"][gr][0], nbr=r["graphs"][gr][1])) for gr in (1, 2)]
    return out


# ---- 1. the fast instances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,kinds,marker", [(96, ("contest", "random"), "hwalk_kernel<24"), (128, ("contest",), "hwalk_kernel<0"),
                                            (960, ("contest",), "hwalk_kernel<0"), (300, ("random",), "hwalk_kernel<0"),
                                            (404, ("random",), "hwalk_kernel<0")], ids=lambda v: str(v) if isinstance(v, int) else None)
def test_fast_instances(g, orc, d, kinds, marker):
    """L2, compact index, one entry point.  d = 96: the 24-step pair form -- one list register over one- and two-pass adjacency rows, two over
    one-pass rows, the two-list kernel without and with the pass loop (ef 100 over the two-pass graph has no 24-step instance: the general
    instance, as planned).  d = 128 and 960 (even chunk counts, the eight- and four-loads loops), 300 (38 chunks: a lane's odd share of
    19, the last chunk half padding) and 404 (51 chunks: the lone even-lane chunk, half padded): the run-time-length instances.  ef 8, 64, 100,
    200 with k = ef, the launched kernel the one half_walk_plan names; k = 1 and 5 at ef 64: the answer is the k-th best."""
    failures = []
    for name, c in _cases(d, kinds):
        off, nbr, ent = c["off"], c["nbr"], c["ent"]
        stride = _stride(off)
        h, f = _pair(g, c["base"], off, nbr, c["db_low"])
        for ef, k in [(ef, ef) for ef in hw.BEAMS] + [(64, 1), (64, 5)]:
            w = hw.expected(orc, ("hw fast", d, name), c["queries"], c["wide"], off, nbr, ef, k, ent)
            planned = g.half_walk_plan(0, d, hw.N, stride, ef)
            if not (d == 96 and stride > 32 and 64 < ef <= 128):
                assert marker in planned, planned
            rh, _ = _check(g, "d %d %s" % (d, name), failures, h, f, c["queries"], ef, k, ent, w, planned=planned)
            if k < ef and not np.array_equal(rh["ids"], hw.expected(orc, ("hw fast", d, name), c["queries"], c["wide"], off, nbr, ef, ef, ent)["ids"][:, ef - k]):
                failures.append((d, name, ef, k, "the answer is not the k-th best of the full list"))
        h.close()
        f.close()
    assert not failures, failures


def test_long_rows_pass_loop(g, orc):
    """Adjacency rows of more than 64 slots (66 .. 90 neighbours): walk_reg_hwalk_kernel<0, 1, false> at ef 64 and
    walk_reg_big_hwalk_kernel<0, false> at ef 200 run the second pass of their loop around l2_pair_rows_half; d = 300."""
    c = hw.random_halves(300)
    off, nbr = hw.three_pass_graph()
    assert _stride(off) == 96
    h, f = _pair(g, c["base"], off, nbr, c["db_low"])
    failures = []
    for ef, planned in ((64, "walk_reg_hwalk_kernel<0, 1, false>"), (200, "walk_reg_big_hwalk_kernel<0, false>")):
        assert g.half_walk_plan(0, 300, hw.N, 96, ef) == planned
        w = hw.expected(orc, ("hw three-pass", 300), c["queries"], c["wide"], off, nbr, ef, ef, c["ent"])
        _check(g, "three-pass graph d 300", failures, h, f, c["queries"], ef, ef, c["ent"], w, planned=planned)
    h.close()
    f.close()
    assert not failures, failures


def test_general_instance_on_the_fast_shapes(g, orc):
    """The handle knob half_walk_fast = 0: the general instance takes the batches the fast instances serve -- the same outputs."""
    failures = []
    for d, name, c in [(96, n, c) for n, c in _cases(96, ("contest", "random"))[:2]] + [(300, n, c) for n, c in _cases(300, ("random",))[1:]]:
        h, f = _pair(g, c["base"], c["off"], c["nbr"], c["db_low"])
        h.knob("half_walk_fast", 0)
        assert h.knob_get("half_walk_fast") == 0
        for ef in (64, 200):
            w = hw.expected(orc, ("hw fast", d, name), c["queries"], c["wide"], c["off"], c["nbr"], ef, ef, c["ent"])
            _, p = _check(g, "half_walk_fast 0, d %d %s" % (d, name), failures, h, f, c["queries"], ef, ef, c["ent"], w, planned="walk_general_kernel")
            if p["general_queries"] != hw.NQ:
                failures.append((d, name, ef, "general_queries %d" % p["general_queries"]))
        h.knob("half_walk_fast", 1)   # the default: the classes the measurement rule kept (d = 96) on their fast instance, the others on the general one
        w = hw.expected(orc, ("hw fast", d, name), c["queries"], c["wide"], c["off"], c["nbr"], 64, 64, c["ent"])
        _check(g, "half_walk_fast 1, d %d %s" % (d, name), failures, h, f, c["queries"], 64, 64, c["ent"], w,
               planned=g.half_walk_plan(0, d, hw.N, _stride(c["off"]), 64) if d == 96 else "walk_general_kernel")
        h.knob("half_walk_fast", 2)
        w = hw.expected(orc, ("hw fast", d, name), c["queries"], c["wide"], c["off"], c["nbr"], 64, 64, c["ent"])
        _check(g, "half_walk_fast 2 again, d %d %s" % (d, name), failures, h, f, c["queries"], 64, 64, c["ent"], w,
               planned=g.half_walk_plan(0, d, hw.N, _stride(c["off"]), 64))
        h.close()
        f.close()
    assert not failures, failures


# ---- 2. hand-overs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (96, 300))
def test_hand_overs_go_straight_to_the_general_instance(g, orc, d):
    """A visited set of 128 entries over the two-pass graph: at least three quarters of the batch is handed over, there is no retry pass,
    the profile shows time in the general kernel, every output is still the oracle's."""
    c = hw.random_halves(d)
    off, nbr = c["graphs"][2]
    failures = []
    h, f = _pair(g, c["base"], off, nbr, c["db_low"])
    for ef in (64, 200):
        w = hw.expected(orc, ("hw fast", d, "random graph 2"), c["queries"], c["wide"], off, nbr, ef, ef, c["ent"])
        planned = g.half_walk_plan(0, d, hw.N, _stride(off), ef)
        assert "hwalk_kernel" in planned
        _, p = _check(g, "hand-over d %d" % d, failures, h, f, c["queries"], ef, ef, c["ent"], w, planned=planned, hash_capacity=128)
        if p["general_queries"] * 4 < 3 * hw.NQ or p["retry_kernel"] != "" or not p["walk_general_ms"] > 0.0:
            failures.append((d, ef, "general_queries %d, retry_kernel %r, walk_general_ms %r" % (p["general_queries"], p["retry_kernel"], p["walk_general_ms"])))
    h.close()
    f.close()
    assert not failures, failures


# ---- 3. the general kernel's half-walk instance ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", hw.GENERAL_CONTESTS, ids=["m%d_d%d" % s for s in hw.GENERAL_CONTESTS])
def test_general_instance_other_shapes(g, orc, metric, d):
    """L2 with the d % 4 tail ignored (45: the tail holds arbitrary bit patterns, NaNs among them), five chunks, one chunk, the half-padded
    chunk; the negative dot without and with its masked tail: the contest fixtures."""
    failures = []
    c = hw.contest(metric, d)
    h, f = _pair(g, c["base"], c["off"], c["nbr"], c["db_low"], metric)
    for ef in (8, 64, 200):
        w = hw.expected(orc, ("hw general", metric, d), c["queries"], c["wide"], c["off"], c["nbr"], ef, ef, c["ent"], metric=metric)
        planned = g.half_walk_plan(metric, d, hw.N, _stride(c["off"]), ef)
        assert planned == "walk_general_kernel"
        _check(g, "metric %d d %d" % (metric, d), failures, h, f, c["queries"], ef, ef, c["ent"], w, planned=planned)
    h.close()
    f.close()
    assert not failures, failures


def test_general_instance_on_d96(g, orc):
    """What takes a d = 96 L2 call out of the fast instances' domain: three entry points per query, the auxiliary graph with and without
    llf and hops_bound, FLAG_WIDE_INDEX, a beam above 1 024; FLAG_BITMAP_PASS is ignored."""
    c = hw.random_halves(96)
    off, nbr = c["graphs"][1]
    rng = tu.rng_of(8890)
    h, f = _pair(g, c["base"], off, nbr, c["db_low"])
    failures = []
    ent3 = np.ascontiguousarray(np.stack([c["ent"], rng.integers(0, hw.N, size=hw.NQ), rng.integers(0, hw.N, size=hw.NQ)], axis=1).astype(np.uint32))
    w = hw.expected(orc, "hw ent3", c["queries"], c["wide"], off, nbr, 64, 64, ent3)
    _check(g, "three entry points", failures, h, f, c["queries"], 64, 64, ent3, w, planned="walk_general_kernel")
    aux = datagen.random_graph(rng, hw.N, 0, 20)
    for ix in (h, f):
        ix.set_aux_graph(aux[0], aux[1])
    for llf, hbound in ((False, 50), (True, 50), (True, 3)):
        w = hw.expected(orc, "hw aux", c["queries"], c["wide"], off, nbr, 64, 64, c["ent"], aux=aux, llf=llf, hops_bound=hbound)
        _check(g, "auxiliary graph llf %s hops_bound %d" % (llf, hbound), failures, h, f, c["queries"], 64, 64, c["ent"], w, planned="walk_general_kernel",
               aux=True, llf=llf, hops_bound=hbound)
    for ix in (h, f):
        ix.set_aux_graph(None, None)
    w = hw.expected(orc, ("hw fast", 96, "random graph 1"), c["queries"], c["wide"], off, nbr, 64, 64, c["ent"])
    _check(g, "wide index", failures, h, f, c["queries"], 64, 64, c["ent"], w, planned="walk_general_kernel", flags=g.FLAG_WIDE_INDEX,
           float_flags=g.FLAG_WIDE_INDEX)
    # (the float handle unflagged: FLAG_BITMAP_PASS changes no output there either, but it is the flagged call that must ignore it)
    _check(g, "bitmap pass flag", failures, h, f, c["queries"], 64, 64, c["ent"], w, planned=g.half_walk_plan(0, 96, hw.N, _stride(off), 64),
           flags=g.FLAG_BITMAP_PASS)
    w = hw.expected(orc, ("hw fast", 96, "random graph 1"), c["queries"], c["wide"], off, nbr, 1100, 1100, c["ent"])
    _check(g, "ef 1 100", failures, h, f, c["queries"], 1100, 1100, c["ent"], w, planned="walk_general_kernel")
    h.close()
    f.close()
    assert not failures, failures


# ---- 4. buffers and flight ---------------------------------------------------------------------------------------------------------
def test_device_buffers_and_batches_in_flight(g, orc):
    """DEVICE tensors in and out (the half table a borrowed torch.float16 tensor); three FLAG_DEFER_JOIN batches in flight with rotating
    buffers give byte-identical outputs to the synchronous HOST call of their batch, which is the oracle's; FLAG_SERIAL too; an entry id >= n
    in a DEVICE buffer gives the bad-entry row."""
    import torch
    c = hw.random_halves(96)
    off, nbr = c["graphs"][1]
    ef = 64
    rng = tu.rng_of(8891)
    ix = g.Index(_t(c["base"]), off, nbr, db_low=_t(c["db_low"]))
    assert ix.is_half_base
    ix.knob("coop", 0)
    assert ix.knob_get("half_walk_fast") == 1
    flt = g.Index(c["wide"], off, nbr, db_low=c["db_low"])
    flt.knob("coop", 0)
    batches = [(np.ascontiguousarray(c["queries"][rng.permutation(hw.NQ)]), rng.integers(0, hw.N, size=hw.NQ).astype(np.uint32)) for _ in range(3)]
    host = []
    for i, (q, ent) in enumerate(batches):
        r = ix.search(q, ef, mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=WANT, flags=g.FLAG_HALF_WALK)
        assert not hw.against(r, hw.expected(orc, ("hw flight", i), q, c["wide"], off, nbr, ef, ef, ent)), i
        s = ix.search(q, ef, mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=WANT, flags=g.FLAG_HALF_WALK | g.FLAG_SERIAL)
        assert not hw.same_bytes(r, s), i
        assert not hw.same_bytes(r, flt.search(q, ef, mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=WANT)), i   # the float handle, byte for byte
        host.append(r)
    assert len({r["cand"].tobytes() for r in host}) == 3
    dev_in = [(_t(q), _t(ent.view(np.int32))) for q, ent in batches]
    outs = [ix.search(dev_in[call % 3][0], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=dev_in[call % 3][1], out={}, want=WANT,
                      flags=g.FLAG_HALF_WALK | g.FLAG_DEFER_JOIN, defer_depth=3) for call in range(9)]
    ix.join()
    torch.cuda.synchronize()
    for call, r in enumerate(outs):
        for name in ("ids",) + WANT:
            assert r[name].cpu().numpy().tobytes() == host[call % 3][name].tobytes(), (call, name)
    # a bad entry id in a DEVICE buffer: data, not an error -- the all-0xFFFFFFFF row for that query, the others untouched
    q, ent = batches[0]
    bad = ent.copy()
    bad[5] = hw.N
    bad[17] = 0xFFFFFFF0
    for ef2 in (64, 200):
        want = hw.expected(orc, ("hw flight", 0), q, c["wide"], off, nbr, ef2, ef2, ent)
        r = ix.search(_t(q), ef2, mode=g.MODE_PLAIN, k=ef2, entry_ids=_t(bad.view(np.int32)), want=WANT, flags=g.FLAG_HALF_WALK)
        torch.cuda.synchronize()
        r = {n: v.cpu().numpy() for n, v in r.items()}
        ok = np.ones(hw.NQ, bool)
        ok[[5, 17]] = False
        assert np.array_equal(r["cand"].view(np.uint32)[ok], want["ids"][ok]) and np.array_equal(r["ids"].view(np.uint32)[ok], want["want"][ok])
        for i in (5, 17):
            assert (r["cand"].view(np.uint32)[i] == hw.NONE).all() and r["ids"].view(np.uint32)[i] == hw.NONE
            assert r["hops"][i] == 0 and r["dist_calc"][i] == 0 and r["edges"][i] == 0 and np.isinf(r["cand_dist"][i]).all()
    ix.close()
    flt.close()


def test_flagged_call_between_net_calls(g):
    """One handle: NET, the flagged PLAIN call (fast and general instance), NET again -- the NET answers are what they were, and the float
    handle's."""
    c = hw.contest(0, 96)
    h, f = _pair(g, c["base"], c["off"], c["nbr"], c["db_low"], net=c["net"])
    names = ("ids",) + WANT
    for ef in (64, 200):
        before = h.search(c["queries"], ef, entry_ids=c["ent"], want=WANT)
        assert not hw.same_bytes(before, f.search(c["queries"], ef, entry_ids=c["ent"], want=WANT), names)
        p1 = h.search(c["queries"], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=c["ent"], want=WANT, flags=g.FLAG_HALF_WALK)
        p2 = h.search(c["queries"], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=c["ent"], want=WANT, flags=g.FLAG_HALF_WALK | g.FLAG_WIDE_INDEX)
        assert not hw.same_bytes(p1, p2, names)
        assert not hw.same_bytes(p1, f.search(c["queries"], ef, mode=g.MODE_PLAIN, k=ef, entry_ids=c["ent"], want=WANT), names)
        after = h.search(c["queries"], ef, entry_ids=c["ent"], want=WANT)
        assert not hw.same_bytes(before, after, names), ef
    h.close()
    f.close()


# ---- 5. tagged -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [(0, 96), (1, 45)])
def test_tagged_and_bridged(g, orc, metric, d):
    """query_tags with half the rows allowed, cut and bridged: the oracle on cut_graph's / bridge_graph's CSR over the widened table; with
    every tag set: the untagged flagged call, counters and edges included."""
    import tag_util as tg
    c = hw.contest(metric, d)
    T = tg.row_tags()
    rng = tu.rng_of(8892 + d)
    pools = [np.arange(q * hw.PER, (q + 1) * hw.PER) for q in c["qg"]]
    h, f = _pair(g, c["base"], c["off"], c["nbr"], c["db_low"], metric)
    for ix in (h, f):
        ix.set_tags(T)
    failures = []
    ef = 64
    Q = np.full(hw.NQ, 0x0F, np.uint32)
    ent = tg.allowed_entries(rng, T, Q, pools)
    allowed = (T & 0x0F) != 0
    assert 0.3 < allowed.mean() < 0.7
    for what, graph_of, flags in (("cut", g.cut_graph, 0), ("bridged", g.bridge_graph, g.FLAG_TAG_BRIDGE)):
        off2, nbr2 = graph_of(c["off"], c["nbr"], allowed)
        w = hw.expected(orc, ("hw tagged", what, metric, d), c["queries"], c["wide"], off2, nbr2, ef, ef, ent, metric=metric)
        assert g.half_walk_plan(metric, d, hw.N, _stride(c["off"]), ef, tagged=True) == "walk_general_kernel"
        _check(g, "tagged, " + what, failures, h, f, c["queries"], ef, ef, ent, w, planned="walk_general_kernel", query_tags=Q, flags=flags,
               float_flags=flags)
    every = np.full(hw.NQ, tg.ALL, np.uint32)
    w = hw.expected(orc, ("hw untagged", metric, d), c["queries"], c["wide"], c["off"], c["nbr"], ef, ef, c["ent"], metric=metric)
    plain, _, _ = _plain(g, h, c["queries"], ef, ef, c["ent"], flags=g.FLAG_HALF_WALK)
    for flags in (0, g.FLAG_TAG_BRIDGE):
        rh, _ = _check(g, "every tag set", failures, h, f, c["queries"], ef, ef, c["ent"], w, query_tags=every, flags=flags, float_flags=flags)
        if hw.same_bytes(rh, plain):
            failures.append(("every tag set", flags, "differs from the untagged flagged call in %s" % hw.same_bytes(rh, plain)))
    h.close()
    f.close()
    assert not failures, failures


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(g):
    import byte_walk_util as bw
    c = hw.contest(0, 96)
    h = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    f = g.Index(c["wide"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"])
    cb = bw.contest(0, 128)
    b = g.Index(cb["base"], cb["off"], cb["nbr"], db_low=cb["db_low"])

    def code(ix, queries=c["queries"], ent=c["ent"], **kw):
        with pytest.raises(g.GbnnsError) as e:
            ix.search(queries, 64, entry_ids=ent, **kw)
        return e.value.code

    with pytest.raises(g.GbnnsError) as e:
        h.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"])
    assert e.value.code == 5 and "GBNNS_MODE_PLAIN" in str(e.value) and "GBNNS_FLAG_HALF_WALK" in str(e.value)   # PLAIN without the flag: still unsupported
    assert code(f, mode=g.MODE_PLAIN, k=1, flags=g.FLAG_HALF_WALK) == 1                                       # the flag on a float handle
    assert code(b, queries=cb["queries"], ent=cb["ent"], mode=g.MODE_PLAIN, k=1, flags=g.FLAG_HALF_WALK) == 1  # ... on a byte handle
    assert code(h, mode=g.MODE_LOWQ, queries_low=c["q_low"], flags=g.FLAG_HALF_WALK) == 1                     # ... with LOWQ
    assert code(h, mode=g.MODE_NET, flags=g.FLAG_HALF_WALK) == 1                                              # ... with NET
    assert code(h, mode=g.MODE_PLAIN, k=1, flags=g.FLAG_HALF_WALK | g.FLAG_BYTE_WALK) == 1                    # ... together with the byte walk's
    assert code(b, queries=cb["queries"], ent=cb["ent"], mode=g.MODE_PLAIN, k=1, flags=g.FLAG_HALF_WALK | g.FLAG_BYTE_WALK) == 1
    assert code(h, mode=g.MODE_PLAIN, k=64, flags=g.FLAG_HALF_WALK, top_k=5) == 1                             # top_k with PLAIN: still invalid
    assert code(h, mode=g.MODE_PLAIN, k=1, flags=g.FLAG_HALF_WALK | g.FLAG_HALF_ROWS) == 1                    # half rows with PLAIN: still invalid
    # uint8 and float16 queries stay refused
    with pytest.raises(TypeError):
        h.search(c["queries"].astype(np.uint8), 64, mode=g.MODE_PLAIN, k=1, flags=g.FLAG_HALF_WALK)
    with pytest.raises(TypeError):
        h.search(c["queries"].astype(np.float16), 64, mode=g.MODE_PLAIN, k=1, flags=g.FLAG_HALF_WALK)
    # the gbnns_multi_* searches
    m = g.MultiIndex(c["wide"], c["off"], c["nbr"], db_low=c["db_low"], devices=[0])
    with pytest.raises(g.GbnnsError) as e:
        m.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"], flags=g.FLAG_HALF_WALK)
    assert e.value.code == 1 and "GBNNS_FLAG_HALF_WALK" in str(e.value)
    with pytest.raises(g.GbnnsError) as e:
        m.search_device([_t(c["queries"])], 64, len(c["queries"]), mode=g.MODE_PLAIN, flags=g.FLAG_HALF_WALK)
    assert e.value.code == 1 and "GBNNS_FLAG_HALF_WALK" in str(e.value)
    m.close()
    # ... and the handles still serve
    r = h.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"], flags=g.FLAG_HALF_WALK)
    assert np.array_equal(r["ids"], f.search(c["queries"], 64, mode=g.MODE_PLAIN, k=1, entry_ids=c["ent"])["ids"])
    for ix in (h, f, b):
        ix.close()
