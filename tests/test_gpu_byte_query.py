"""Byte queries on a byte handle (Index.search(queries=<uint8>), gbnns_search_byte_queries) on an MI355X (run with -m gpu).  The contract:
every output equals, bit for bit, what the corresponding float-query call returns on the same handle with queries.astype(float32).  Expected
values are the unchanged CPU oracle's on the widened table with the widened queries (candidate ids in pop order, distance bit patterns, hops,
dist_calc, the k-th best as the answer), and every case is also compared byte for byte -- edges included -- with the float-query call on the
same handle in the same process.  Nothing takes a tolerance.  tests/test_byte_query_cpu.py shows that the fixtures tell a signed dot, a
partner's chunk and a missing row term apart and that the hand-over case does hand over.

The knob "byte_query_int" is set explicitly wherever the kernel's name is asserted (7: every beam class gets the integer first pass, which is
what byte_query_plan describes; 0: none does), so these tests hold whatever default the measurements give it.
"""
import ctypes as C

import numpy as np
import pytest

import byte_query_util as bq
import byte_rows_util as bu
import byte_walk_util as bw
import datagen
import topk_util as tu

pytestmark = pytest.mark.gpu

WANT = bq.WANT
NONE = bq.NONE


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(torch.device("cuda:0"))  # (a copy: the fixtures' arrays are read-only)


def _handle(g, base, off, nbr, db_low, metric=0, net=None, profile=True):
    ix = g.Index(base, off, nbr, db_low=db_low, metric=metric, net=net)
    assert ix.is_bytes
    ix.profile_enable(profile)
    ix.knob("coop", 0)
    return ix


def _plain(g, ix, queries, ef, k, ent, flags=0, **kw):
    """One profiled PLAIN search with FLAG_BYTE_WALK -> (results, name of the first-pass kernel, profile)."""
    ix.profile_read(reset=True)
    r = ix.search(queries, ef, mode=g.MODE_PLAIN, k=k, entry_ids=ent, want=WANT, flags=g.FLAG_BYTE_WALK | flags, **kw)
    p = ix.profile_read(reset=True)
    return r, p["walk_kernel"].split(" (")[0], p


def _check(g, what, failures, ix, q8, ef, k, ent, w, planned=None, **kw):
    """The byte-query call against the oracle and against the float-query call on the same handle."""
    rb, kb, pb = _plain(g, ix, q8, ef, k, ent, **kw)
    rf, kf, _ = _plain(g, ix, np.ascontiguousarray(q8.astype(np.float32)), ef, k, ent, **kw)
    bad = bq.against(rb, w)
    if bq.same_bytes(rb, rf):
        bad.append("differs from the float-query call in %s" % bq.same_bytes(rb, rf))
    if planned is not None and kb != planned:
        bad.append("launched %s, planned %s" % (kb, planned))
    if "beam_u8" in kf:
        bad.append("the float-query call launched %s" % kf)
    print("byte queries:", what, "ef", ef, "k", k, kb, "general_queries", pb["general_queries"])
    if bad:
        failures.append((what, ef, k, bad))
    return rb, pb


# ---- 1. the fast instances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", (1, 2), ids=["one_pass", "two_pass"])
@pytest.mark.parametrize("name", bq.FIXTURES)
def test_fast_instances(g, orc, name, graph):
    """beam_u8_kernel<1 | 2, ONE_CHUNK> and beam_u8_big_kernel<ONE_PASS> at ef 8, 64, 100, 200 with k = ef, and k = 1 / 5 at ef 64: the launched
    kernel is the one byte_query_plan names; with the knob at 0 the same cases run on walk_reg*_bytes_kernel with the same outputs."""
    c = bq.fixture(name)
    off, nbr = c["graphs"][graph]
    stride = bq.stride(off)
    assert (stride <= 32) == (graph == 1)
    ix = _handle(g, c["base"], off, nbr, c["db_low"])
    failures = []
    for ef, k in [(ef, ef) for ef in bq.BEAMS] + [(64, 1), (64, 5)]:
        w = bq.expected(orc, name, graph, ef, k)
        planned = g.byte_query_plan(0, 128, bq.N, stride, ef)
        assert planned.startswith("beam_u8_"), planned
        ix.knob("byte_query_int", 7)
        on, _ = _check(g, "%s graph %d" % (name, graph), failures, ix, c["queries_u8"], ef, k, c["ent"], w, planned=planned)
        ix.knob("byte_query_int", 0)
        fallback = g.byte_walk_plan(0, 128, bq.N, stride, ef)
        assert fallback.startswith("walk_reg_") and "bytes_kernel" in fallback
        off_, _ = _check(g, "%s graph %d, knob 0" % (name, graph), failures, ix, c["queries_u8"], ef, k, c["ent"], w, planned=fallback)
        if bq.same_bytes(on, off_):
            failures.append((name, graph, ef, k, "knob 7 and knob 0 differ in %s" % bq.same_bytes(on, off_)))
        if k < ef:  # (a list shorter than ef -- the extremes' own component holds 8 rows -- pops its k-th best at count - k)
            full = bq.expected(orc, name, graph, ef, ef)
            kth = full["ids"][np.arange(bq.NQ), np.maximum(full["count"] - k, 0)]
            if not np.array_equal(on["ids"], kth):
                failures.append((name, graph, ef, k, "the answer is not the k-th best of the full list"))
    ix.close()
    assert not failures, failures


def test_extreme_distance_comes_out(g, orc):
    """An all-0 query against an all-255 row: 128 * 255^2 = 8 323 200 exactly, from the integer instance, in cand_dist."""
    c = bq.fixture("extremes")
    off, nbr = c["graphs"][1]
    ix = _handle(g, c["base"], off, nbr, c["db_low"])
    ix.knob("byte_query_int", 7)
    for ef in (8, 200):
        r, kernel, _ = _plain(g, ix, c["queries_u8"], ef, ef, c["ent"])
        assert kernel.startswith("beam_u8_"), kernel
        for qi in range(8):
            d = r["cand_dist"][qi, :8]
            assert sorted(set(d.tolist())) == [0.0, float(bq.FAR)], (ef, qi, d)
    ix.close()


# ---- 2. hand-overs -----------------------------------------------------------------------------------------------------------------
def test_hand_overs_go_straight_to_the_general_instance(g, orc):
    """A visited set of 128 entries: at least three quarters of the batch is handed over to the general kernel's byte-walk instance (which
    reads the widened queries), there is no retry pass, every output is still the oracle's."""
    c = bq.fixture("random")
    failures = []
    for graph in (1, 2):
        off, nbr = c["graphs"][graph]
        ix = _handle(g, c["base"], off, nbr, c["db_low"])
        ix.knob("byte_query_int", 7)
        for ef in (64, 200):
            w = bq.expected(orc, "random", graph, ef, ef)
            _, p = _check(g, "hand-over, graph %d" % graph, failures, ix, c["queries_u8"], ef, ef, c["ent"], w,
                          planned=g.byte_query_plan(0, 128, bq.N, bq.stride(off), ef), hash_capacity=128)
            if p["general_queries"] * 4 < 3 * bq.NQ or p["retry_kernel"] != "":
                failures.append((graph, ef, "general_queries %d, retry_kernel %r" % (p["general_queries"], p["retry_kernel"])))
        ix.close()
    assert not failures, failures


# ---- 3. outside the domain: the general instance on the widened queries ------------------------------------------------------------------
@pytest.mark.parametrize("what,metric,d", [("d48", 0, 48), ("d100", 0, 100), ("dot_d45", 1, 45), ("dot_d128", 1, 128)])
def test_general_instance_other_shapes(g, orc, what, metric, d):
    """Three chunks; 112-byte rows with the d % 4 tail ignored; the negative dot with and without its masked tail."""
    failures = []
    if metric == 0:
        r = bw.random_bytes(d)
        off, nbr = r["graphs"][1]
        base, wide, ent, db_low, q8 = r["base"], r["wide"], r["ent"], r["db_low"], bq._bytes_of(r["queries"])
    else:
        t = bw.contest(metric, d)
        off, nbr, base, wide, ent, db_low = t["off"], t["nbr"], t["base"], t["wide"], t["ent"], t["db_low"]
        q8 = bq._bytes_of(t["queries"] + (np.arange(d) % 7)[None, :])   # (the groups' constant queries, made to vary along the row)
    ix = _handle(g, base, off, nbr, db_low, metric)
    ix.knob("byte_query_int", 7)
    for ef in (8, 64, 200):
        w = bw.expected(orc, ("byte query", what), q8.astype(np.float32), wide, off, nbr, ef, ef, ent, metric=metric)
        assert g.byte_query_plan(metric, d, bq.N, bq.stride(off), ef) == "walk_general_kernel"
        _check(g, what, failures, ix, q8, ef, ef, ent, w, planned="walk_general_kernel")
    ix.close()
    assert not failures, failures


def test_general_instance_on_d128(g, orc):
    """What takes a d = 128 L2 call out of the integer instances' domain: three entry points, the auxiliary graph, FLAG_WIDE_INDEX."""
    c = bq.fixture("random")
    off, nbr = c["graphs"][1]
    rng = tu.rng_of(7803)
    ix = _handle(g, c["base"], off, nbr, c["db_low"])
    ix.knob("byte_query_int", 7)
    failures = []
    q8, qf = c["queries_u8"], c["queries"]
    ent3 = np.ascontiguousarray(np.stack([c["ent"], rng.integers(0, bq.N, size=bq.NQ), rng.integers(0, bq.N, size=bq.NQ)], axis=1).astype(np.uint32))
    w = bw.expected(orc, ("byte query", "ent3"), qf, c["wide"], off, nbr, 64, 64, ent3)
    _check(g, "three entry points", failures, ix, q8, 64, 64, ent3, w, planned="walk_general_kernel")
    aux = datagen.random_graph(rng, bq.N, 0, 20)
    ix.set_aux_graph(aux[0], aux[1])
    for llf, hb in ((False, 50), (True, 3)):
        w = bw.expected(orc, ("byte query", "aux"), qf, c["wide"], off, nbr, 64, 64, c["ent"], aux=aux, llf=llf, hops_bound=hb)
        _check(g, "auxiliary graph llf %s hops_bound %d" % (llf, hb), failures, ix, q8, 64, 64, c["ent"], w, planned="walk_general_kernel",
               aux=True, llf=llf, hops_bound=hb)
    ix.set_aux_graph(None, None)
    w = bq.expected(orc, "random", 1, 64, 64)
    _check(g, "wide index", failures, ix, q8, 64, 64, c["ent"], w, planned="walk_general_kernel", flags=g.FLAG_WIDE_INDEX)
    ix.close()
    assert not failures, failures


def test_tagged_and_bridged(g, orc):
    """query_tags with half the rows allowed, cut and bridged: the oracle on cut_graph's / bridge_graph's CSR; the general kernel's instance."""
    import tag_util as tg
    c = bq.fixture("ties")
    t = bw.contest(0, 128, True)
    off, nbr = c["graphs"][1]
    T = tg.row_tags()
    rng = tu.rng_of(7804)
    pools = [np.arange(q * bu.PER, (q + 1) * bu.PER) for q in t["qg"]]
    ix = _handle(g, c["base"], off, nbr, c["db_low"])
    ix.knob("byte_query_int", 7)
    ix.set_tags(T)
    failures = []
    ef = 64
    Q = np.full(bq.NQ, 0x0F, np.uint32)
    ent = tg.allowed_entries(rng, T, Q, pools)
    allowed = (T & 0x0F) != 0
    for what, graph_of, flags in (("cut", g.cut_graph, 0), ("bridged", g.bridge_graph, g.FLAG_TAG_BRIDGE)):
        off2, nbr2 = graph_of(off, nbr, allowed)
        w = bw.expected(orc, ("byte query", "tagged", what), c["queries"], c["wide"], off2, nbr2, ef, ef, ent)
        assert g.byte_query_plan(0, 128, bq.N, bq.stride(off), ef, tagged=True) == "walk_general_kernel"
        _check(g, "tagged, " + what, failures, ix, c["queries_u8"], ef, ef, ent, w, planned="walk_general_kernel", query_tags=Q, flags=flags)
    ix.close()
    assert not failures, failures


# ---- 4. NET and LOWQ -----------------------------------------------------------------------------------------------------------------
NET_WANT = ("hops", "dist_calc", "cand", "cand_dist", "edges", "q_low")


def _net_case():
    c = bq.fixture("random")
    rng = tu.rng_of(7805)
    net = datagen.net_layers_full(rng, 128, 64, 32)
    q_low = datagen.full_mantissa(rng, bq.NQ, 32)
    return c, net, q_low


def _same(a, b, names):
    return [n for n in names if np.asarray(a[n]).tobytes() != np.asarray(b[n]).tobytes()]


@pytest.mark.parametrize("top_k", (1, 10))
def test_net_and_lowq_host_and_device(g, top_k):
    """A 128 -> 32 net: NET (the projection, the walk over db_low, the byte re-rank and the k-answer rows all read the widened copy) and LOWQ
    (queries_low stays float32), HOST and DEVICE buffers, fused and unfused re-rank -- every output identical to the float-query call."""
    import torch
    c, net, q_low = _net_case()
    off, nbr = c["graphs"][1]
    ix = _handle(g, c["base"], off, nbr, c["db_low"], net=net, profile=False)
    q8, qf = c["queries_u8"], c["queries"]
    names = ("ids", "top_ids", "top_dist") + NET_WANT
    for ef in (16, 64, 200):
        if top_k > ef:
            continue
        for flags in (0, g.FLAG_NO_FUSED_RERANK):
            for mode, kw, want in ((g.MODE_NET, {}, NET_WANT), (g.MODE_LOWQ, dict(queries_low=q_low), NET_WANT[:-1])):
                a = ix.search(q8, ef, mode=mode, entry_ids=c["ent"], want=want, top_k=top_k, flags=flags, **kw)
                b = ix.search(qf, ef, mode=mode, entry_ids=c["ent"], want=want, top_k=top_k, flags=flags, **kw)
                assert not _same(a, b, [n for n in names if n in a]), (ef, flags, mode, _same(a, b, [n for n in names if n in a]))
                assert (a["top_ids"][:, 0] == a["ids"]).all()
                kd = {n: _t(v) for n, v in kw.items()}
                ad = ix.search(_t(q8), ef, mode=mode, entry_ids=_t(c["ent"].view(np.int32)), want=want, top_k=top_k, flags=flags, **kd)
                torch.cuda.synchronize()
                ad = {n: v.cpu().numpy() for n, v in ad.items()}
                assert not _same(ad, b, [n for n in names if n in ad]), (ef, flags, mode, "device")
    # a DEVICE byte buffer that does not start on a 16-byte boundary (a view into a larger tensor)
    big = torch.empty(bq.NQ * 128 + 64, dtype=torch.uint8, device="cuda:0")
    odd = big[3:3 + bq.NQ * 128].view(bq.NQ, 128)
    odd.copy_(_t(q8))
    assert odd.data_ptr() % 16 != 0
    b = ix.search(qf, 64, mode=g.MODE_NET, entry_ids=c["ent"], want=NET_WANT, top_k=top_k)
    ad = ix.search(odd, 64, mode=g.MODE_NET, entry_ids=_t(c["ent"].view(np.int32)), want=NET_WANT, top_k=top_k)
    torch.cuda.synchronize()
    assert not _same({n: v.cpu().numpy() for n, v in ad.items()}, b, names)
    ix.close()


@pytest.mark.parametrize("mode_name", ("net", "plain"))
def test_three_batches_in_flight(g, mode_name):
    """Three FLAG_DEFER_JOIN batches in flight, DEVICE buffers and page-locked HOST buffers, three DISTINCT batches rotating over nine calls:
    every call's outputs are those of the synchronous float-query call of its batch -- a byte staging buffer or a widened copy reused before
    its batch was through would show."""
    import torch
    c, net, _ = _net_case()
    off, nbr = c["graphs"][1]
    ix = _handle(g, c["base"], off, nbr, c["db_low"], net=net, profile=False)
    ix.knob("byte_query_int", 7)
    rng = tu.rng_of(7806)
    ef = 64
    if mode_name == "net":
        kw, names = dict(mode=g.MODE_NET, want=NET_WANT, top_k=10), ("ids", "top_ids", "top_dist") + NET_WANT
    else:
        kw, names = dict(mode=g.MODE_PLAIN, k=ef, want=WANT, flags=g.FLAG_BYTE_WALK), ("ids",) + WANT
    flags = kw.pop("flags", 0)
    batches = [(np.ascontiguousarray(c["queries_u8"][rng.permutation(bq.NQ)]), rng.integers(0, bq.N, size=bq.NQ).astype(np.uint32)) for _ in range(3)]
    sync = [ix.search(np.ascontiguousarray(q.astype(np.float32)), ef, entry_ids=ent, flags=flags, **kw) for q, ent in batches]
    assert len({s["cand"].tobytes() for s in sync}) == 3
    dev_in = [(_t(q), _t(ent.view(np.int32))) for q, ent in batches]
    pin_in = [(torch.from_numpy(q).pin_memory(), torch.from_numpy(ent.view(np.int32)).pin_memory()) for q, ent in batches]
    for what, inputs in (("device", dev_in), ("pinned host", pin_in)):
        outs = [ix.search(inputs[call % 3][0], ef, entry_ids=inputs[call % 3][1], out={}, flags=flags | g.FLAG_DEFER_JOIN, defer_depth=3, **kw)
                for call in range(9)]
        ix.join()
        torch.cuda.synchronize()
        for call, r in enumerate(outs):
            for n in names:
                assert r[n].cpu().numpy().tobytes() == np.asarray(sync[call % 3][n]).tobytes(), (what, call, n)
        # ... and FLAG_SERIAL
        s = ix.search(batches[1][0], ef, entry_ids=batches[1][1], flags=flags | g.FLAG_SERIAL, **kw)
        assert not _same(s, sync[1], names)
    ix.close()


# ---- 5. a bad entry id ---------------------------------------------------------------------------------------------------------------
def test_bad_entry_id(g, orc):
    """An entry id >= n in a DEVICE buffer is data: the all-0xFFFFFFFF row for that query, the others untouched -- from the integer instance
    (register-list and two-list form) and from the general one."""
    import torch
    c = bq.fixture("random")
    off, nbr = c["graphs"][1]
    ix = _handle(g, c["base"], off, nbr, c["db_low"], profile=False)
    ix.knob("byte_query_int", 7)
    bad = c["ent"].copy()
    bad[5] = bq.N
    bad[17] = 0xFFFFFFF0
    ok = np.ones(bq.NQ, bool)
    ok[[5, 17]] = False
    for ef, flags in ((64, 0), (200, 0), (64, g.FLAG_WIDE_INDEX)):
        want = bq.expected(orc, "random", 1, ef, ef)
        r = ix.search(_t(c["queries_u8"]), ef, mode=g.MODE_PLAIN, k=ef, entry_ids=_t(bad.view(np.int32)), want=WANT, flags=g.FLAG_BYTE_WALK | flags)
        torch.cuda.synchronize()
        r = {n: v.cpu().numpy() for n, v in r.items()}
        assert np.array_equal(r["cand"].view(np.uint32)[ok], want["ids"][ok]) and np.array_equal(r["ids"].view(np.uint32)[ok], want["want"][ok])
        for i in (5, 17):
            assert (r["cand"].view(np.uint32)[i] == NONE).all() and r["ids"].view(np.uint32)[i] == NONE
            assert r["hops"][i] == 0 and r["dist_calc"][i] == 0 and r["edges"][i] == 0 and np.isinf(r["cand_dist"][i]).all()
    ix.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(g):
    from gbnns_dim_red_amd import binding
    t = bw.contest(0, 128, True)
    q8 = bq.fixture("ties")["queries_u8"]
    b = g.Index(t["base"], t["off"], t["nbr"], db_low=t["db_low"], net=t["net"])
    f = g.Index(t["wide"], t["off"], t["nbr"], db_low=t["db_low"], net=t["net"])
    lib = g.load_library()
    ids = np.zeros(bq.NQ, np.uint32)
    a = binding._SearchArgs(struct_size=C.sizeof(binding._SearchArgs), mode=g.MODE_NET, ef=64, k=64, mem_kind=binding.MEM_HOST, n_q=bq.NQ,
                            out_ids=ids.ctypes.data)
    assert lib.gbnns_search_byte_queries(f._h, C.byref(a), q8.ctypes.data, None, 0, None, None) == 1   # a float handle
    assert b"byte handle" in lib.gbnns_last_error()
    with pytest.raises(TypeError):
        f.search(q8, 64)
    a.queries = t["queries"].ctypes.data
    assert lib.gbnns_search_byte_queries(b._h, C.byref(a), q8.ctypes.data, None, 0, None, None) == 1   # args->queries beside queries_u8
    a.queries = None
    assert lib.gbnns_search_byte_queries(b._h, C.byref(a), None, None, 0, None, None) == 1             # no queries at all

    def code(**kw):   # what the corresponding float call refuses, with its own code
        with pytest.raises(g.GbnnsError) as e:
            b.search(q8, 64, entry_ids=t["ent"], **kw)
        with pytest.raises(g.GbnnsError) as e2:
            b.search(t["queries"], 64, entry_ids=t["ent"], **kw)
        assert e.value.code == e2.value.code
        return e.value.code

    assert code(mode=g.MODE_PLAIN, k=1) == 5                                              # PLAIN without FLAG_BYTE_WALK
    assert code(mode=g.MODE_NET, flags=g.FLAG_BYTE_WALK) == 1                             # the flag with NET
    assert code(mode=g.MODE_PLAIN, k=64, flags=g.FLAG_BYTE_WALK, top_k=5) == 1            # top_k with PLAIN
    assert code(mode=g.MODE_NET, flags=g.FLAG_TAG_BRIDGE) == 1                            # the bridge without tags
    assert code(mode=g.MODE_LOWQ) == 1                                                    # LOWQ without queries_low
    assert code(mode=g.MODE_NET, query_tags=np.full(bq.NQ, 1, np.uint32)) == 1            # tags without a tag table
    # ... and the handle still serves
    r = b.search(q8, 64, mode=g.MODE_NET, entry_ids=t["ent"])
    assert np.array_equal(r["ids"], b.search(t["queries"], 64, mode=g.MODE_NET, entry_ids=t["ent"])["ids"])
    b.close()
    f.close()
