"""The locality order of deep batches on an MI355X (run with -m gpu): the counting sort alone (gbnns_debug_query_order: the three kernels
of gd_order.hip at every key width, at the edges of their 256-thread blocks and with more queries than buckets), the rule that decides
which calls are ordered, and ordered batches in flight on three lanes.  The order inside a bucket is whatever the atomics gave, so an
order is checked for what it must be -- a permutation of the batch whose keys do not decrease (tests/locality_order_util.py) -- and an
ordered search for what it must not change: every output, byte for byte.  The instance tests of the walk families run their own cases
a second time in order (test_gpu_walk_instances.py, test_gpu_tags.py, test_gpu_bridge.py, test_gpu_half_rows.py, test_gpu_byte_rows.py,
test_gpu_topk.py, test_gpu_tag_auto.py, test_gpu_rounding.py).  Nothing takes a tolerance.
"""
import numpy as np
import pytest

import datagen
import golden_util as gu
import locality_order_util as lo
import walk_instances as wi

pytestmark = pytest.mark.gpu

WANT = ("hops", "dist_calc", "cand", "cand_dist")
NQS = (1, 2, 255, 256, 257, 1023, 1025, 70000)   # the edges of the 256-thread blocks; more queries than the 65 536 buckets of 16 bits
FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list((7300,) + key)))


def _edge_values():
    tiny = np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]   # the smallest positive subnormal
    big = np.finfo(np.float32).max
    return np.array([0.0, -0.0, np.nan, np.inf, -np.inf, tiny, -tiny, big, -big], np.float32)


def _contents(nq, dim):
    """name -> [nq x dim] float32 batches: what the key reads at its easiest and at its worst."""
    rng = _rng(nq, dim)
    rows = datagen.full_mantissa(rng, nq, dim)
    mag = np.abs(rows) + np.float32(2.0 ** -20)
    ends = np.where((rng.integers(0, 2, size=nq) == 1)[:, None], mag, -mag).astype(np.float32)
    nonpos = -np.abs(rows)
    nonpos[::3, ::2] = 0.0
    nonpos[1::3, 1::2] = -0.0
    edge = _edge_values()
    cyc = rows.copy()
    cyc[:, :16] = edge[(np.arange(nq)[:, None] * 5 + np.arange(16)[None, :]) % len(edge)]
    return {"random": rows, "all positive": mag, "none positive": nonpos, "two buckets at the ends": ends, "edge values": cyc}


# ---- a. the sort alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", NQS)
def test_the_sort_alone(g, nq):
    """gbnns_debug_query_order on rows of 16 coordinates (dim == bits at 16 bits) at 10, 12 and 16 key bits -- order_scan_kernel's 1, 4 and
    64 counters per thread -- over five contents, and on rows of 20 coordinates 28 floats apart: every result is a valid order; the
    one-bucket batches come back as permutations whatever the atomics did, and the keys of the edge-value batch are the reference's."""
    failures = []
    for name, q in _contents(nq, 16).items():
        for bits in lo.BITS:
            bad = lo.problems(g.query_order(q, bits), q, bits)
            if bad:
                failures.append((name, bits, bad))
    # rows further apart than they are long, in a buffer whose padding would give other keys
    rows = datagen.full_mantissa(_rng(nq, 20), nq, 20)
    padded = np.full((nq, 28), np.float32(7.0), np.float32)
    padded[:, :20] = rows
    for bits in lo.BITS:
        bad = lo.problems(g.query_order(padded, bits, dim=20), rows, bits)
        if bad:
            failures.append(("stride 28", bits, bad))
    assert not failures, failures
    # the batches are what they claim to be
    c = _contents(nq, 16)
    assert (lo.key(c["all positive"], 16) == 0xFFFF).all() and (lo.key(c["none positive"], 16) == 0).all()
    assert set(lo.key(c["two buckets at the ends"], 12).tolist()) <= {0, 0xFFF}
    if nq >= 255:
        assert len(set(lo.key(c["edge values"], 16).tolist())) >= 9 and len(set(lo.key(c["random"], 12).tolist())) > 4


def test_the_histogram_of_one_call_does_not_reach_the_next(g):
    """Two calls in a row with different batch sizes and widths, the larger first: counters left behind by the first call would shift the
    second call's buckets."""
    big, small = _contents(70000, 16)["random"], _contents(257, 16)["random"]
    for first, second in (((big, 16), (small, 10)), ((big, 10), (small, 16)), ((small, 12), (big, 12)), ((big, 12), (small, 12))):
        assert lo.problems(g.query_order(*first), *first) == []
        assert lo.problems(g.query_order(*second), *second) == [], (len(first[0]), first[1], len(second[0]), second[1])


def test_the_sort_clamps_its_width_and_refuses_short_rows(g):
    q = _contents(300, 16)["random"]
    assert lo.problems(g.query_order(q, 3), q, 10) == [] and lo.problems(g.query_order(q, 40), q, 16) == []   # clamped to 10 .. 16
    q12 = np.ascontiguousarray(q[:, :12])
    assert lo.problems(g.query_order(q12, 12), q12, 12) == [] and lo.problems(g.query_order(q12, 0), q12, 10) == []
    for dim, bits in ((12, 16), (9, 10), (15, 99)):   # fewer coordinates than key bits after clamping: the launcher's refusal
        with pytest.raises(g.GbnnsError) as e:
            g.query_order(np.ascontiguousarray(q[:, :dim]), bits)
        assert e.value.code == 3, (dim, bits, e.value)
    assert lo.problems(g.query_order(q, 12), q, 12) == []   # the refusals left nothing behind


# ---- d. where the rule says no -------------------------------------------------------------------------------------------------------
def _case():
    return next(c for c in wi.CASES if (c.metric, c.dim, c.deg, c.aux, c.ef, c.wide, c.bitmap, c.hash_capacity) == (0, 32, 30, 0, 64, 0, 0, 0))


def _against_walk(r, w, want=None, rows=slice(None)):
    bad = []
    if not np.array_equal(r["cand"], w["ids"][rows]):
        bad.append("candidate ids")
    if not np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"][rows])):
        bad.append("distance bits")
    if not np.array_equal(r["hops"], w["hops"][rows]) or not np.array_equal(r["dist_calc"], w["dist_calc"][rows]):
        bad.append("hops / dist_calc")
    if want is not None and not np.array_equal(r["ids"], want[rows]):
        bad.append("answers")
    return bad


def test_where_the_rule_says_no(g, orc):
    """With "order_min" = 1 a MODE_PLAIN call is not ordered, nor a LOWQ call over 12 walked coordinates; with "order_min" = 0 nothing is;
    with "order_min" = 96 a batch of 95 queries is not and a batch of 96 is.  Every call's outputs are the oracle's."""
    c = _case()
    v = wi.vectors(c.metric, c.dim, c.n)
    off, nbr = wi.graph(*c.graph_key)
    w, want = wi.oracle_walk(orc, c)
    ix = g.Index(v["base"], off, nbr, db_low=v["db_low"], metric=c.metric)
    assert (ix.knob_get("order_min"), ix.knob_get("order_bits"), ix.knob_get("order_last")) == (32768, 12, 0)
    with pytest.raises(g.GbnnsError) as e:   # no ordered call yet
        ix.order_last()
    assert e.value.code == 1
    for name, val in c.knobs.items():
        ix.knob(name, val)
    lowq = lambda n: ix.search(v["queries"][:n], c.ef, mode=g.MODE_LOWQ, queries_low=v["q_low"][:n], entry_ids=v["ent"][:n], want=WANT)
    # the defaults: 96 queries are far below 32 768
    assert not _against_walk(lowq(wi.NQ), w, want) and ix.knob_get("order_last") == 0
    ix.knob("order_min", 1)
    ix.knob("order_bits", 99)
    assert (ix.knob_get("order_min"), ix.knob_get("order_bits")) == (1, 16)
    assert not _against_walk(lowq(wi.NQ), w, want) and ix.knob_get("order_last") == wi.NQ
    assert lo.problems(ix.order_last(), v["q_low"], 16) == []
    # MODE_PLAIN: never ordered
    wp = orc.walk(v["queries"], v["base"], off, nbr, c.ef, entries=v["ent"], metric=c.metric, threads=8)
    r = ix.search(v["queries"], c.ef, mode=g.MODE_PLAIN, k=c.ef, entry_ids=v["ent"], want=WANT)
    assert not _against_walk(r, wp) and ix.knob_get("order_last") == 0
    assert lo.problems(ix.order_last(), v["q_low"], 16) == []   # still the last ORDERED call's
    # the threshold itself
    ix.knob("order_min", wi.NQ)
    ix.knob("order_bits", 12)
    r = lowq(wi.NQ - 1)
    assert not _against_walk(r, w, want, slice(0, wi.NQ - 1)) and ix.knob_get("order_last") == 0
    assert not _against_walk(lowq(wi.NQ), w, want) and ix.knob_get("order_last") == wi.NQ
    assert lo.problems(ix.order_last(), v["q_low"], 12) == []
    ix.knob("order_min", wi.NQ + 1)
    assert not _against_walk(lowq(wi.NQ), w, want) and ix.knob_get("order_last") == 0
    # never
    ix.knob("order_min", -4)
    assert ix.knob_get("order_min") == 0
    assert not _against_walk(lowq(wi.NQ), w, want) and ix.knob_get("order_last") == 0
    ix.close()
    # 12 walked coordinates: fewer than the rule's 16, whatever the key width
    rng = _rng(12)
    db12, q12 = datagen.full_mantissa(rng, c.n, 12), datagen.full_mantissa(rng, wi.NQ, 12)
    ix = g.Index(v["base"], off, nbr, db_low=db12, metric=c.metric)
    ix.knob("order_min", 1)
    ix.knob("order_bits", 10)
    w12 = orc.walk(q12, db12, off, nbr, c.ef, entries=v["ent"], metric=c.metric, threads=8)
    want12 = orc.rerank(v["queries"], w12["ids"], w12["count"], v["base"], metric=c.metric, threads=8)
    r = ix.search(v["queries"], c.ef, mode=g.MODE_LOWQ, queries_low=q12, entry_ids=v["ent"], want=WANT)
    assert not _against_walk(r, w12, want12) and ix.knob_get("order_last") == 0
    ix.close()


# ---- e. in flight ----------------------------------------------------------------------------------------------------------------------
def test_ordered_batches_in_flight(g):
    """Three lanes of one handle with "order_min" = 1 run DEVICE-buffer batches of 96, 2 048 and 300 queries side by side, two rounds; in
    the second round the lane that ordered 96 queries takes the 2 048-query batch, so its order buffer grows while the other lanes' calls
    are in flight.  Every output buffer is filled with 0xA5 bytes before its launch.  After the join every call's outputs equal the
    synchronous unordered result of its batch, and no slot holds the fill."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = _case()
    v = wi.vectors(c.metric, c.dim, c.n)
    off, nbr = wi.graph(*c.graph_key)
    rng = _rng(2048)
    q_all, ql_all = datagen.full_mantissa(rng, 2048, wi.D_ORIG), datagen.full_mantissa(rng, 2048, c.dim)
    ent_all = rng.integers(0, c.n, size=2048).astype(np.uint32)
    batches = [slice(0, 96), slice(0, 2048), slice(1000, 1300)]
    for s in batches:
        assert lo.moved(ql_all[s], 12) * 16 >= 15 * (s.stop - s.start)   # the sort moves nearly every work item of each batch
    ix = g.Index(v["base"], off, nbr, db_low=v["db_low"], metric=c.metric)
    kw = dict(mode=g.MODE_LOWQ, want=WANT)
    ix.knob("order_min", 0)
    host = [ix.search(q_all[s], c.ef, queries_low=ql_all[s], entry_ids=ent_all[s], **kw) for s in batches]
    assert ix.knob_get("order_last") == 0
    for h in host:
        for name in ("ids",) + WANT:
            assert not (np.ascontiguousarray(h[name]).view(np.uint32) == FILL).any(), name
    ix.knob("order_min", 1)
    dev_in = [(t(q_all[s]), t(ql_all[s]), t(ent_all[s].view(np.int32))) for s in batches]

    def filled(nq):
        i32 = lambda *shape: torch.full(shape, FILL - (1 << 32), dtype=torch.int32, device=dev)
        return dict(ids=i32(nq), hops=i32(nq), dist_calc=i32(nq), cand=i32(nq, c.ef), cand_dist=i32(nq, c.ef).view(torch.float32))

    calls = [0, 1, 2, 1, 2, 0]   # the lanes rotate: lane 0 takes 96 queries, then 2 048
    outs = []
    for b in calls:
        q, ql, ent = dev_in[b]
        out = filled(int(q.shape[0]))
        outs.append(ix.search(q, c.ef, queries_low=ql, entry_ids=ent, out=out, flags=g.FLAG_DEFER_JOIN, defer_depth=3, **kw))
        assert ix.knob_get("order_last") == int(q.shape[0])
    ix.join()
    torch.cuda.synchronize()
    for call, (b, r) in enumerate(zip(calls, outs)):
        for name in ("ids",) + WANT:
            got = r[name].cpu().numpy()
            assert not (got.view(np.uint32) == FILL).any(), (call, name, "a slot still holds the fill")
            assert got.tobytes() == host[b][name].tobytes(), (call, b, name)
    # the last ordered call ran on lane 2 with 96 queries: its permutation is read from that lane
    assert lo.problems(ix.order_last(), ql_all[batches[0]], 12) == []
    ix.close()
