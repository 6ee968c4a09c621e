"""What tests/test_locality_order_cpu.py and the GPU tests share about the locality order of a batch (gd_order.hip, WalkParams::order): the
reference key, the validity check of an order, the non-vacuity count, the fixtures the GPU tests run in order, and the second, ordered run
that the instance tests make inside their own case loops.

The contract: a search whose batch has at least "order_min" queries (handle knob; NET / LOWQ, at least 16 walked coordinates) sorts the
batch by key(q) = OR over j < bits of (q[j] > 0) << (bits - 1 - j) on the walked-space queries, and work item b walks query order[b].
Only the order of the work changes: every output of the ordered call equals the unordered call's byte for byte.  The order inside a bucket
is whatever the atomics gave, so an order is checked for what it must be -- a permutation with non-decreasing keys -- and not against one
particular sort.
"""
import numpy as np

BITS = (10, 12, 16)      # order_scan_kernel's `per` 1, 4 and 64
MOVED_MIN = 90           # of 96 positions: what every fixture run in order must reach under a stable sort (see moved)

RUNS = [0]               # ordered runs made through in_order so far in this process (the GPU tests print it)


def key(q, bits):
    """[nq] uint32 keys of float32 rows q [nq x >= bits]: coordinate 0 is the most significant bit, and a coordinate counts as 1 exactly
    where it compares > 0 in float32 -- so +-0, NaN and -inf give 0, +inf and the positive subnormals give 1."""
    q = np.asarray(q)
    assert q.dtype == np.float32 and q.ndim == 2 and q.shape[1] >= bits, (q.dtype, q.shape, bits)
    with np.errstate(invalid="ignore"):
        pos = q[:, :bits] > np.float32(0)
    weights = (np.uint32(1) << np.arange(bits - 1, -1, -1, dtype=np.uint32)).astype(np.uint32)
    return (pos.astype(np.uint32) * weights).sum(axis=1, dtype=np.uint32)


def problems(order, q, bits):
    """What keeps `order` from being a valid locality order of the rows q: [] when it is a permutation of 0 .. nq-1 whose keys do not
    decrease."""
    order = np.asarray(order)
    nq = len(q)
    if order.shape != (nq,):
        return ["%d entries for %d queries" % (order.size, nq)]
    o = order.astype(np.int64)
    bad = []
    outside = int(((o < 0) | (o >= nq)).sum())
    if outside:
        return ["%d entries outside 0 .. %d (first %d)" % (outside, nq - 1, int(order[(o < 0) | (o >= nq)][0]))]
    counts = np.bincount(o, minlength=nq)
    if (counts != 1).any():
        bad.append("not a permutation: %d queries missing, %d more than once" % (int((counts == 0).sum()), int((counts > 1).sum())))
    k = key(q, bits)[o].astype(np.int64)
    down = np.flatnonzero(k[1:] < k[:-1])
    if down.size:
        bad.append("keys decrease at %d positions (first at %d: %d then %d)" % (down.size, int(down[0]) + 1, int(k[down[0]]), int(k[down[0] + 1])))
    return bad


def stable_order(q, bits):
    return np.argsort(key(q, bits), kind="stable").astype(np.uint32)


def moved(q, bits):
    """Positions of the batch whose work item changes under a stable sort by key: how far the sort is from the identity.  An ordered run
    proves something only where this is nearly the whole batch."""
    return int((stable_order(q, bits) != np.arange(len(q))).sum())


def fixtures():
    """(name, bits tuple, walked-space queries [nq x dim]) of every batch the GPU tests run in order."""
    import bridge_util as bu
    import byte_rows_util as by
    import half_rows_util as hu
    import tag_auto_util as au
    import tag_util as tg
    import topk_util as tu
    import walk_instances as wi
    out = []
    for metric, dim, n in sorted({(c.metric, c.dim, c.n) for c in wi.CASES}):
        out.append((("census", metric, dim, n), BITS, wi.vectors(metric, dim, n)["q_low"]))
    for s in tg.SHAPES:
        out.append((("tag contest",) + s, (12,), tg.contest(*s)["q_low"]))
    for s in tg.TWO_PASS_SHAPES:
        out.append((("tag two-pass",) + s, (12,), tg.two_pass(*s)["q_low"]))
    for slots in (40, 72):
        for dlow in (32, 144):
            out.append((("tag odd_first", slots, dlow), (12,), tg.odd_first(slots, dlow)["q_low"]))
    for s in hu.SHAPES:
        out.append((("half contest",) + s, (12,), hu.contest(*s)["q_low"]))
    for s in hu.TWO_PASS_SHAPES:
        out.append((("half two-pass",) + s, (12,), hu.two_pass(*s)["q_low"]))
    out.append((("bridge parity",), (12,), bu.parity()["q_low"]))
    out.append((("bridge twins",), (12,), bu.twins()["q_low"]))
    for s in TOPK_SHAPES:
        out.append((("topk contest",) + s, (12,), tu.contest_index_data(*s)["q_low"]))
    for metric in (0, 1):
        out.append((("tag_auto", metric), (12,), au.fixture(metric)["q_low"]))
    out.append((("byte rows",), (12,), by.index_data(0, 128, 32)["q_low"]))
    return out


TOPK_SHAPES = [(0, 128, 32), (0, 960, 64), (0, 300, 32), (1, 200, 32)]   # test_gpu_topk.SEARCH_SHAPES
# The one MODE_NET search run in order (test_gpu_rounding.test_net_mode_on_a_contest_index): there the sort reads the PROJECTED queries.
# The contest batches are twelve copies of one original-space query per group, so their projections fall into at most eight buckets; on
# the other three shapes of that test they all share one key at 12 bits (a stable sort moves nothing), on this one every group moves.
NET_SHAPE = (0, 960, 64)


def net_fixture(orc):
    """(name, bits tuple, the projected queries [96 x 64]) of the MODE_NET batch run in order."""
    import topk_util as tu
    c = tu.contest_index_data(*NET_SHAPE)
    return (("net contest",) + NET_SHAPE, (12,), orc.project(c["net"], c["queries"]))


def in_order(ix, q_walked, run, bits=12):
    """run() once more with the handle's batches walked in locality order from one query on, at `bits` key bits; the handle is back at
    "never" afterwards.  -> (what run returned, problems): the call must have ordered its whole batch (knob "order_last") and the
    permutation it used, read back from the handle, must be a valid order of q_walked, the queries in the walked space."""
    ix.knob("order_min", 1)
    ix.knob("order_bits", bits)
    try:
        out = run()
        last = ix.knob_get("order_last")
        bad = [] if last == len(q_walked) else ["order_last %d, batch %d" % (last, len(q_walked))]
        if last:
            bad += problems(ix.order_last(), q_walked, bits)
    finally:
        ix.knob("order_min", 0)
    RUNS[0] += 1
    return out, bad


def same_kernels(po, p, explicit_capacity):
    """What the profile po of an ordered call names differently from the profile p of the unordered one: the first-pass kernel, and the
    retry kernel.  With the library's own visited-set capacity (explicit_capacity false) the retry launch is left out once calls of that
    beam have been calm (call_plan.cpp, skip_retry), so between two calls of one handle the retry name may turn into the empty string
    and back; there two NAMES have to be the same name.  With hash_capacity set the launch never depends on the handle's history."""
    bad = []
    if po["walk_kernel"].split(" (")[0] != p["walk_kernel"].split(" (")[0]:
        bad.append("first pass launched %s, unordered %s" % (po["walk_kernel"], p["walk_kernel"]))
    if po["retry_kernel"] != p["retry_kernel"] and (explicit_capacity or (po["retry_kernel"] and p["retry_kernel"])):
        bad.append("retry pass launched '%s', unordered '%s'" % (po["retry_kernel"], p["retry_kernel"]))
    return bad


def same_bytes(a, b, names):
    """Names among `names` whose arrays differ between the result dicts a and b, byte for byte."""
    return ["%s differs from the unordered run" % n for n in names if np.asarray(a[n]).tobytes() != np.asarray(b[n]).tobytes()]
