"""GPU parity on inputs that make the ORDER of the float32 roundings visible (run with -m gpu on an MI355X).

The vectors of datagen.Case are small dyadic rationals: every summation order returns their distance bits, so the
"distance bits equal the oracle's" assertions of test_gpu_parity.py pin ids, ties and counters in the original
space, not L2Metric::Dist's four running sums and ((s0+s1)+s2)+s3, Angular::Dist's eight sums, fold and
(m0+m1)+(m2+m3), or the absence of fused multiply-add.  Here the same kernels run on

  * datagen.full_mantissa vectors (about 22 significant bits per coordinate): a wrong order changes 17 % and more
    of the distance bit patterns;
  * the equal-distance contests datagen.contest_l2 / contest_dot: the candidates of a query are equidistant in real
    arithmetic, so a re-rank -- which returns ids only -- is decided by the order of the roundings (a wrong order moves
    the winner of 15 % and more of 32-candidate lists) and, among the several candidates tied at the float32 minimum,
    by pop position;
  * datagen.net_layers_full nets (about 20 significant bits per weight): layer 1 rounds at every step;
  * graph preparation, whose kernels restate the two distances on their own (knn.hip, gd_order.hip): the exact kNN on
    full-mantissa vectors and on the contests, GD pruning on datagen.gd_contest_l2 / gd_contest_dot, where a hub keeps its
    candidate or not by a comparison of two distances that are equal in real arithmetic, and on full-mantissa vectors.

tests/test_rounding_fixtures.py proves those shares on the CPU.  Everything here is bit-exact against the CPU oracle;
nothing takes a tolerance.  The first-pass kernel of every walk is asserted by name where test_gpu_parity.py
establishes the name for the shape, and is part of every assertion message.
"""
import functools

import numpy as np
import pytest

import datagen
import golden_util as gu
import locality_order_util as lo
import oracle as orc_mod

pytestmark = pytest.mark.gpu

GROUPS, PER = 8, 256       # the contests: 8 groups x 256 rows
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---- a. PLAIN walks: distance bits on full-mantissa vectors -------------------------------------------------------
PLAIN_SHAPES = [  # d, metric, beams -- the distance form each reaches is in the test's docstring
    (96, 0, (40, 128, 200)), (128, 0, (64, 200, 300)), (132, 0, (64,)), (516, 0, (64,)), (300, 0, (40, 300)), (960, 0, (8, 200)),
    (45, 0, (33,)), (200, 0, (64,)), (200, 1, (64,)),
]


def _plain_kernel(d, ef):
    """The first-pass kernel of a PLAIN walk over 384- / 512-byte rows with one-pass adjacency rows, as
    test_plain_walks_over_wide_rows_two_list_pair_form establishes it."""
    if ef <= 128:
        return "walk_reg_kernel<0, 24," if d == 96 else "walk_reg_kernel<0, 0,"
    return "walk_reg_big_kernel<0, 0," if d == 128 and ef <= 200 else "walk_reg_big_kernel<0, %d," % (d // 4)


@pytest.mark.parametrize("d,metric,efs", PLAIN_SHAPES, ids=["d%d_m%d" % s[:2] for s in PLAIN_SHAPES])
def test_plain_walk_distance_bits_on_full_mantissa_vectors(g, orc, d, metric, efs):
    """PLAIN walks (the graph walked in the ORIGINAL space) on full-mantissa vectors: candidate ids in pop order, the bit
    patterns of their distances, hops and dist_calc equal the oracle's.  d = 96: the pair-form list instances
    (walk_reg_kernel<0, 24, ...>) and the two-list pair form (walk_reg_big_kernel<0, 24, ...>); d = 128: four lanes per row
    (l2_quad_rows) in the list and the run-time-length two-list instances, the <0, 32, ...> pair form from ef = 201 on;
    d = 132 / 516: a masked last quad batch; d = 300 / 960: long rows, beams on either side of the two-list kernels;
    d = 45: the tail L2Metric::Dist ignores; d = 200: both metrics.  At d = 96 / 128 also rows requested before / after the
    visited test, the bitmap first pass, the non-compact instantiations, and a visited set too small (the hand-over chain into
    the retry and general kernels), with the kernel names asserted."""
    big = d >= 300
    n, nq = (2000, 64) if big else (3000, 100)
    rng = _rng(5100 + 2 * d + metric)
    base = datagen.full_mantissa(rng, n, d)
    queries = datagen.full_mantissa(rng, nq, d)
    off, nbr = datagen.random_graph(rng, n, 2, 30)
    ent = rng.integers(0, n, size=nq).astype(np.uint32)
    ix = g.Index(base, off, nbr, metric=metric)
    ix.profile_enable(True)
    named = d in (96, 128)
    variants = [("late0", {"late_rows": 0}, 0, 0), ("late1", {"late_rows": 1}, 0, 0), ("bitmap", {}, g.FLAG_BITMAP_PASS, 0),
                ("wide", {}, g.FLAG_WIDE_INDEX, 0), ("small table", {}, 0, 256)] if named else [("default", {}, 0, 0)]
    wrong_kernel = []
    for ef in efs:
        w = orc.walk(queries, base, off, nbr, ef, entries=ent, metric=metric, threads=8)
        for tag, knobs, flags, cap in variants:
            ix.knob("late_rows", knobs.get("late_rows", -1))
            ix.profile_read(reset=True)
            r = ix.search(queries, ef, mode=g.MODE_PLAIN, k=ef, entry_ids=ent, want=("hops", "dist_calc", "cand", "cand_dist"),
                          flags=flags, hash_capacity=cap)
            launched = ix.profile_read(reset=True)["walk_kernel"]
            key = (d, metric, ef, tag, launched)
            print("plain", key)
            assert np.array_equal(r["cand"], w["ids"]), key
            assert np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])), key
            assert np.array_equal(r["hops"], w["hops"]) and np.array_equal(r["dist_calc"], w["dist_calc"]), key
            if named and tag in ("late0", "late1") and not launched.startswith(_plain_kernel(d, ef)):
                wrong_kernel.append((key, _plain_kernel(d, ef)))
    ix.close()
    assert not wrong_kernel, wrong_kernel


# ---- b. the stand-alone re-rank on the equal-distance contests ------------------------------------------------------
RERANK_COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 200)
RERANK_SHAPES = [(128, 0), (960, 0), (388, 0), (300, 0), (300, 1), (200, 1), (45, 0), (45, 1)]


def rerank_contest(d, metric):
    """base, queries [nq x d], cand [nq x 200] (own group's rows in random order, 0xFFFFFFFF beyond count), count: twelve
    queries per entry of RERANK_COUNTS."""
    rng = _rng(5300 + 2 * d + metric)
    base, gq, _ = (datagen.contest_dot if metric else datagen.contest_l2)(rng, GROUPS, PER, d)
    count = np.repeat(np.array(RERANK_COUNTS, np.int32), 12)
    qg = rng.integers(0, GROUPS, size=len(count))
    cand = np.full((len(count), max(RERANK_COUNTS)), NONE, np.uint32)
    for i, (c, grp) in enumerate(zip(count, qg)):
        cand[i, :c] = grp * PER + rng.permutation(PER)[:c]
    return base, np.ascontiguousarray(gq[qg]), cand, count


@pytest.mark.parametrize("d,metric", RERANK_SHAPES, ids=["d%d_m%d" % s for s in RERANK_SHAPES])
def test_rerank_contest_stand_alone(g, orc, d, metric):
    """gbnns_rerank against getRealNearest on candidates that are equidistant in real arithmetic -- the winner is the first
    of the candidates at the float32 minimum of the reference's summation order.  d = 128: rerank_pair_kernel; 960: its DEEP = 24
    form; 388: DEEP = 24 plus the even lane's odd step; 300 L2: d % 8 == 4; 300 dot: a lane per row (rerank_kernel); 200 dot:
    the pair form's eight sums over two lanes; 45: a lane per row, the tail ignored (L2) / masked (dot).  Counts 0 .. 200 around the
    32-candidate passes of the pair form and the 64-candidate passes of the lane-per-row form; an empty list answers 0xFFFFFFFF."""
    base, q, cand, count = rerank_contest(d, metric)
    off, nbr = datagen.contest_graph(_rng(1), GROUPS, PER, 1, 2)
    some = count > 0
    want = np.full(len(count), NONE, np.uint32)
    want[some] = orc.rerank(q[some], cand[some], count[some], base, metric=metric, threads=8)
    # the contest is one: lists whose minimum is shared by several candidates, in different 32-candidate passes too
    dist = np.array([[(orc.negdot if metric else orc.l2)(base[c], qi) for c in row[:n]] + [np.inf] * (cand.shape[1] - n)
                     for qi, row, n in zip(q, cand, count)], np.float32)
    at_min = dist == dist.min(axis=1, keepdims=True)
    straddle = at_min[:, :32].any(1) & at_min[:, 32:].any(1)
    assert (at_min[some].sum(1) >= 2).sum() >= 20 and straddle[some].sum() >= 5, (at_min.sum(1), straddle.sum())
    ix = g.Index(base, off, nbr, metric=metric)
    got = ix.rerank(q, cand, count)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (d, metric, [(int(count[i]), int(got[i]), int(want[i])) for i in bad[:8]], bad.size)
    # full lists without a count array (count = stride)
    full = count == cand.shape[1]
    assert np.array_equal(ix.rerank(q[full], cand[full]), want[full]), (d, metric, "count = stride")
    ix.close()


# ---- c. the fused re-rank behind the walk kernels, on the contests --------------------------------------------------
@functools.lru_cache(maxsize=None)
def contest_index_data(metric, d, dlow):
    """A contest index: original-space rows from contest_l2 / contest_dot, independent full-mantissa low-dimensional rows, the groups
    disconnected components of the graph; twelve queries per group that share the group's original-space query and differ in their
    low-dimensional query and entry point; a full-mantissa net."""
    rng = _rng(5500 + 7 * d + 3 * dlow + metric)
    base, gq, group = (datagen.contest_dot if metric else datagen.contest_l2)(rng, GROUPS, PER, d)
    db_low = datagen.full_mantissa(rng, GROUPS * PER, dlow)
    off, nbr = datagen.contest_graph(rng, GROUPS, PER, 2, 30)
    qg = np.repeat(np.arange(GROUPS), 12)
    q_low = datagen.full_mantissa(rng, len(qg), dlow)
    ent = (qg * PER + rng.integers(0, PER, size=len(qg))).astype(np.uint32)
    net = datagen.net_layers_full(rng, d, 64, dlow)
    return dict(base=base, gq=gq, group=group, db_low=db_low, off=off, nbr=nbr, qg=qg, queries=np.ascontiguousarray(gq[qg]), q_low=q_low,
                ent=ent, net=net)


def _hosts(g, dlow, full):
    """(ef, knobs, flags, hash_capacity, first-pass kernel as test_two_list_kernels_by_name names it, None: recorded only)."""
    B, W, NF = g.FLAG_BITMAP_PASS, g.FLAG_WIDE_INDEX, g.FLAG_NO_FUSED_RERANK
    if dlow == 32:
        rows = [(200, {"coop": 0}, 0, 0, "walk_hot_big_kernel"), (200, {"coop": 1}, 0, 0, "walk_coop_kernel<8,")]
        if full:
            rows += [(8, {}, 0, 0, "walk_hot_kernel"), (64, {}, 0, 0, "walk_hot_kernel"), (100, {}, 0, 0, "walk_hot2_kernel"),
                     (200, {"coop": 0}, B, 0, "walk_bitmap_big_kernel<0, 8,"), (1100, {}, 0, 0, None),
                     (64, {}, W, 0, None), (200, {"coop": 0}, W, 0, None), (64, {}, 0, 128, None), (200, {"coop": 0}, 0, 128, None),
                     (64, {}, NF, 0, "walk_hot_kernel"), (200, {"coop": 0}, NF, 0, "walk_hot_big_kernel")]
        return rows
    if dlow == 48:
        return [(40, {}, 0, 0, "walk_reg_wide_kernel<12,"), (100, {}, 0, 0, "walk_reg_kernel<0, 12,"), (200, {"coop": 0}, 0, 0, "walk_reg_big_kernel<0, 12,")]
    if dlow == 64:
        return [(40, {}, 0, 0, "walk_reg_wide_kernel<16,"), (200, {"coop": 0}, 0, 0, "walk_reg_big_kernel<0, 16,")]
    return [(40, {}, 0, 0, "walk_reg_kernel<0, 24,"), (200, {}, 0, 0, "walk_reg_big_kernel<0, 24,")]   # d_low 96


FUSED_SHAPES = [(0, 128, 32), (0, 128, 48), (0, 128, 96), (0, 960, 32), (0, 960, 64), (0, 300, 32), (0, 300, 64), (1, 200, 32)]


@pytest.mark.parametrize("metric,d,dlow", FUSED_SHAPES, ids=["m%d_d%d_low%d" % s for s in FUSED_SHAPES])
def test_fused_rerank_contest_through_the_search_paths(g, orc, metric, d, dlow):
    """The two-stage search on a contest index (MODE_LOWQ: the walk over independent low-dimensional rows picks the candidates, every
    one of them equidistant from the query in the original space in real arithmetic): answers equal getRealNearest over the oracle's
    walk, candidate lists, their distance bits, hops and dist_calc equal the walk's.  Each walk kernel that re-ranks its own query
    (rerank_pairs_core fused into it): walk_hot, walk_hot2, walk_hot_big, the two-wavefront kernel's alternating passes, the bitmap
    first pass, walk_reg* over 192- / 256- / 384-byte walked rows, the non-compact instantiations, a forced hand-over to the retry /
    general kernels, plus the re-rank in its own launch (the LDS-list kernel at ef = 1 100, GBNNS_FLAG_NO_FUSED_RERANK); d = 960: the
    DEEP = 24 form inside the walk kernels; d = 300: d % 8 == 4; one dot-metric index."""
    c = contest_index_data(metric, d, dlow)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], metric=metric)
    ix.profile_enable(True)
    hosts = [(64, {}, 0, 0, "walk_hot_dot_kernel<1, false>"), (200, {}, 0, 0, "walk_hot_dot_big_kernel<false>")] if metric else \
        _hosts(g, dlow, full=(d == 128))
    wrong_kernel, walks = [], {}
    for ef, knobs, flags, cap, kname in hosts:
        if ef not in walks:
            w = orc.walk(c["q_low"], c["db_low"], c["off"], c["nbr"], ef, entries=c["ent"], metric=metric, threads=8)
            walks[ef] = (w, orc.rerank(c["queries"], w["ids"], w["count"], c["base"], metric=metric, threads=8))
        w, want = walks[ef]
        ix.knob("coop", knobs.get("coop", -1))
        ix.profile_read(reset=True)
        r = ix.search(c["queries"], ef, mode=g.MODE_LOWQ, queries_low=c["q_low"], entry_ids=c["ent"],
                      want=("hops", "dist_calc", "cand", "cand_dist"), flags=flags, hash_capacity=cap)
        launched = ix.profile_read(reset=True)["walk_kernel"]
        key = (metric, d, dlow, ef, tuple(knobs.items()), flags, cap, launched)
        print("fused", key)
        assert np.array_equal(r["cand"], w["ids"]), key
        assert np.array_equal(gu.bits(r["cand_dist"]), gu.bits(w["dists"])), key
        assert np.array_equal(r["hops"], w["hops"]) and np.array_equal(r["dist_calc"], w["dist_calc"]), key
        bad = np.flatnonzero(r["ids"] != want)
        assert bad.size == 0, (key, bad.size, [(int(r["ids"][i]), int(want[i])) for i in bad[:8]])
        assert (c["group"][r["ids"]] == c["qg"]).all(), key
        if kname is not None and not launched.startswith(kname):
            wrong_kernel.append((key, kname))
    ix.close()
    assert not wrong_kernel, wrong_kernel


NET_SHAPES = [(0, 128, 32), (0, 960, 64), (0, 300, 32), (1, 200, 32)]


@pytest.mark.parametrize("metric,d,dlow", NET_SHAPES, ids=["m%d_d%d_low%d" % s for s in NET_SHAPES])
def test_net_mode_on_a_contest_index(g, orc, metric, d, dlow):
    """The path the product ships (MODE_NET) on a contest index with a full-mantissa net: one distinct query per group, several entry
    points each; projected queries bit for bit, answers, hops, dist_calc against the oracle's two-stage search."""
    c = contest_index_data(metric, d, dlow)
    ix = g.Index(c["base"], c["off"], c["nbr"], db_low=c["db_low"], net=c["net"], metric=metric)
    ix.profile_enable(True)
    q_low = orc.project(c["net"], c["queries"])
    for ef in (8, 64, 200):
        s = orc.search_batch(orc_mod.MODE_NET, c["queries"], c["base"], c["off"], c["nbr"], ef, db_low=c["db_low"], net=c["net"],
                             entries=c["ent"], metric=metric, threads=8)
        ix.profile_read(reset=True)
        r = ix.search(c["queries"], ef, entry_ids=c["ent"], want=("hops", "dist_calc", "q_low"))
        p = ix.profile_read(reset=True)
        key = (metric, d, dlow, ef, p["walk_kernel"], p["project_kernel"])
        print("net", key)
        assert np.array_equal(gu.bits(r["q_low"]), gu.bits(q_low)), key
        assert np.array_equal(r["ids"], s["ids"]), key
        assert np.array_equal(r["hops"], s["hops"]) and np.array_equal(r["dist_calc"] + ef, s["dist_calc"]), key
        if (metric, d, dlow) == lo.NET_SHAPE and ef == 64:
            # once more in locality order: the sort reads the PROJECTED queries, rows dl_pad floats apart in the lane's buffer (the one
            # shape of this test whose projected batch the sort moves: locality_order_util.NET_SHAPE)
            ro, in_order = lo.in_order(ix, q_low, lambda: ix.search(c["queries"], ef, entry_ids=c["ent"], want=("hops", "dist_calc", "q_low")))
            in_order += lo.same_bytes(ro, r, ("ids", "hops", "dist_calc", "q_low")) + lo.same_kernels(ix.profile_read(reset=True), p, False)
            assert not in_order, (key, in_order)
    ix.close()


# ---- d. the projection: layer 1 on inexact inputs -------------------------------------------------------------------
PROJECT_SHAPES = [  # d, d_hidden, d_low, queries, the kernel the batch takes by default
    (128, 256, 32, 2049, "mlp_net_kernel"), (200, 72, 32, 2049, "mlp_net_kernel"),
    (960, 1024, 64, 130, "mlp_slab_kernel"), (520, 136, 16, 301, "mlp_slab_kernel"),
    (45, 27, 14, 100, "mlp_layer_kernels"),
]


def _projection_case(orc, seed, d, dh, dl, nq, n=1000):
    rng = _rng(seed)
    base = datagen.full_mantissa(rng, n, d)
    queries = datagen.full_mantissa(rng, nq, d)
    net = datagen.net_layers_full(rng, d, dh, dl)
    off, nbr = datagen.random_graph(rng, n, 4, 28)
    ent = rng.integers(0, n, size=nq).astype(np.uint32)
    db_low = orc.project(net, base, threads=8)
    return base, queries, net, off, nbr, ent, db_low


@pytest.mark.parametrize("d,dh,dl,nq,kernel", PROJECT_SHAPES, ids=["%d_%d_%d" % s[:3] for s in PROJECT_SHAPES])
def test_projection_of_full_mantissa_inputs(g, orc, d, dh, dl, nq, kernel):
    """GetLowQueryFromNet on full-mantissa queries through a full-mantissa net (every product and partial sum of layer 1 rounds):
    q_low bit patterns of a search and of gbnns_project over 700 base rows equal the oracle's -- on the one-launch kernel
    (mlp_net_kernel), the slab kernel (mlp_slab_kernel) and, with both switched off and for a net with d % 8 != 0, the per-layer
    kernels; answers equal the oracle's two-stage search."""
    base, queries, net, off, nbr, ent, db_low = _projection_case(orc, 5700 + d, d, dh, dl, nq)
    want_q = orc.project(net, queries, threads=8)
    want_b = orc.project(net, base[:700], threads=8)
    sref = orc.search_batch(orc_mod.MODE_NET, queries, base, off, nbr, 40, db_low=db_low, net=net, entries=ent, threads=8)
    ix = g.Index(base, off, nbr, db_low=db_low, net=net)
    for knobs, want_kernel in (({}, kernel), ({"mlp_net": 0, "mlp_slab": 0}, "mlp_layer_kernels")):
        for name, val in knobs.items():
            ix.knob(name, val)
        r = ix.search(queries, 40, entry_ids=ent, want=("q_low",))
        launched = ix.profile_read(reset=False)["project_kernel"]
        key = (d, dh, dl, nq, tuple(knobs.items()), launched)
        print("project", key)
        assert launched == want_kernel, key
        bad = int((gu.bits(r["q_low"]) != gu.bits(want_q)).sum())
        assert bad == 0, (key, bad, r["q_low"].size)
        assert np.array_equal(r["ids"], sref["ids"]), key
        pl = ix.project(base[:700])
        assert np.array_equal(gu.bits(pl), gu.bits(want_b)), (key, ix.profile_read(reset=False)["project_kernel"])
    ix.close()


def test_projection_of_full_mantissa_inputs_small_footprint_kernel(g, orc):
    """Batches in flight whose hidden layers run on mlp_layer_sw_kernel (deferred calls; d % 8 == 4, a hidden width that is no
    multiple of the block's 16 neurons, a batch that is no multiple of its 64 queries): same bits.  Knob "mlp_small" is the smallest
    batch that takes it, and 32 times the knob the largest: 64 serves the 777 queries (the value 1 would serve batches of up to 32).
    The kernel has no profile name of its own; that it ran shows in the slab kernel -- which these deferred calls take otherwise --
    NOT being reported: a small-footprint projection never uses it."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d, dh, dl, nq = 44, 72, 32, 777
    base, queries, net, off, nbr, ent, db_low = _projection_case(orc, 5790, d, dh, dl, nq)
    want_q = orc.project(net, queries, threads=8)
    sref = orc.search_batch(orc_mod.MODE_NET, queries, base, off, nbr, 48, db_low=db_low, net=net, entries=ent, threads=8)
    ix = g.Index(t(base), off, nbr, db_low=t(db_low), net=tuple(t(x) for x in net))
    q, e = t(queries), t(ent.astype(np.int32))
    for small, kernel in ((0, "mlp_slab_kernel"), (64, "mlp_layer_kernels")):
        ix.knob("mlp_small", small)
        outs = [ix.search(q, 48, entry_ids=e, want=("q_low",), out={}, flags=g.FLAG_DEFER_JOIN, defer_depth=3) for _ in range(4)]
        ix.join()
        torch.cuda.synchronize()
        assert ix.profile_read(reset=False)["project_kernel"] == kernel, small
        for r in outs:
            assert np.array_equal(gu.bits(r["q_low"].cpu().numpy()), gu.bits(want_q)), small
            assert np.array_equal(r["ids"].cpu().numpy().view(np.uint32), sref["ids"]), small
    pl = ix.project(t(base[:700]))
    torch.cuda.synchronize()
    assert np.array_equal(gu.bits(pl.cpu().numpy()), gu.bits(orc.project(net, base[:700], threads=8)))
    ix.close()


# ---- e. graph preparation: the exact kNN ----------------------------------------------------------------------------
@pytest.fixture
def knn_knobs(g):
    """Sets gbnns_exact_knn's process-wide knobs; the defaults (filter by size, pool from k = 64) come back afterwards."""
    lib = g.load_library()

    def set_knobs(knn_filter=1, knn_pool_min_k=64):
        assert lib.gbnns_debug_knob(b"knn_filter", knn_filter) == 0 and lib.gbnns_debug_knob(b"knn_pool_min_k", knn_pool_min_k) == 0
    try:
        yield set_knobs
    finally:
        lib.gbnns_debug_knob(b"knn_filter", 1)
        lib.gbnns_debug_knob(b"knn_pool_min_k", 64)


_KNN_CACHE = {}


def knn_full_mantissa(orc, metric, d, n=2500, nq=257, k=63):
    """full_mantissa rows and queries (257 queries: the last thread block is partial) and the oracle's k nearest, computed once."""
    key = (metric, d, n, nq, k)
    if key not in _KNN_CACHE:
        rng = _rng(5900 + 2 * d + metric)
        base, queries = datagen.full_mantissa(rng, n, d), datagen.full_mantissa(rng, nq, d)
        _KNN_CACHE[key] = (base, queries) + orc.exact_knn(base, queries, k, metric, threads=8)
    return _KNN_CACHE[key]


def _knn_equal(g, base, queries, k, metric, oi, od, key, **kw):
    """ids and distance bits of g.exact_knn against the first k columns of the oracle's lists."""
    ids, dist = g.exact_knn(base, queries, k, metric=metric, want_dist=True, **kw)
    bad = np.flatnonzero((ids != oi[:, :k]).any(axis=1) | (gu.bits(dist) != gu.bits(od[:, :k])).any(axis=1))
    assert bad.size == 0, (key, k, bad.size, bad[:8].tolist())


KNN_SCAN_SHAPES = [(0, 32), (0, 45), (0, 64), (0, 96), (0, 100), (0, 128), (0, 130), (0, 200), (0, 960), (1, 32), (1, 200), (1, 960)]


@pytest.mark.parametrize("metric,d", KNN_SCAN_SHAPES, ids=["m%d_d%d" % s for s in KNN_SCAN_SHAPES])
def test_exact_knn_heap_scan_on_full_mantissa_vectors(g, orc, knn_knobs, metric, d):
    """gbnns_exact_knn's plain scan (the filter off) on full-mantissa vectors against the oracle: ids and distance bits at k = 1 / 20 /
    63.  knn_scan_kernel<METRIC, 8 / 16 / 32>: d = 32; 45 (the tail Dist ignores) and 64; 96, 100 (d % 16 != 0) and 128.
    knn_scan_wide_kernel: d = 130 (d % 4 != 0, rows that are not 16-byte aligned), 200 (a last chunk of two steps) and 960."""
    base, queries, oi, od = knn_full_mantissa(orc, metric, d)
    knn_knobs(knn_filter=0)
    for k in (1, 20, 63):
        _knn_equal(g, base, queries, k, metric, oi, od, (metric, d))


@pytest.mark.parametrize("metric,d", [(0, 32), (0, 200), (1, 32), (1, 200)], ids=lambda v: str(v))
def test_exact_knn_of_a_set_over_itself_on_full_mantissa_vectors(g, orc, knn_knobs, metric, d):
    """The kNN lists of a set over itself (self_offset: row i + offset is query i and is left out), in two slices of queries."""
    n, k = 1500, 20
    base = datagen.full_mantissa(_rng(6000 + 2 * d + metric), n, d)
    oi, od = orc.exact_knn(base, base, k, metric, self_offset=0, threads=8)
    knn_knobs(knn_filter=0)
    half = n // 2 + 7
    _knn_equal(g, base, base[:half].copy(), k, metric, oi[:half], od[:half], (metric, d, "first slice"), self_offset=0)
    _knn_equal(g, base, base[half:].copy(), k, metric, oi[half:], od[half:], (metric, d, "second slice"), self_offset=half)


@pytest.mark.parametrize("d", (32, 64, 100, 128))
def test_exact_knn_behind_the_filter_on_full_mantissa_vectors(g, orc, knn_knobs, d):
    """The matrix-core filter forced on: the distances come from knn_rescore_kernel<8 / 16 / 32> (k = 20) and, lists on the pool path,
    from knn_pool_update_kernel (k = 64 and 300 on 2 048 rows -- the path needs n > 4 k -- and k = 7 with knob "knn_pool_min_k" = 1).
    Against the oracle, not against the other GPU path."""
    base, queries, oi, od = knn_full_mantissa(orc, 0, d)
    knn_knobs(knn_filter=2)
    _knn_equal(g, base, queries, 20, 0, oi, od, (d, "rescore"))
    pb, pq, pi, pd = knn_full_mantissa(orc, 0, d, n=2048, nq=130, k=300)
    for k in (64, 300):
        _knn_equal(g, pb, pq, k, 0, pi, pd, (d, "pool"))
    knn_knobs(knn_filter=2, knn_pool_min_k=1)
    _knn_equal(g, pb, pq, 7, 0, pi, pd, (d, "pool, short list"))


KNN_CONTEST_SHAPES = [(0, 32), (0, 128), (0, 300), (1, 32), (1, 200)]


@pytest.mark.parametrize("metric,d", KNN_CONTEST_SHAPES, ids=["m%d_d%d" % s for s in KNN_CONTEST_SHAPES])
def test_exact_knn_on_the_contests(g, orc, knn_knobs, metric, d):
    """The k nearest rows of the contest groups' queries (8 groups x 256 rows equidistant from their query in real arithmetic; every
    query five times, so that it also sits in other lanes): which rows are returned is decided by the order of the roundings
    (tests/test_rounding_fixtures.py: a wrong order changes every list) and, among the rows at the k-th float32 distance, by
    ascending id.  k = 1 .. 257: at 257 a group's rows run out.  L2 at d <= 128 also with the filter forced -- 256 rows at one real
    distance, with norms far larger than the distance, are the worst case for its c (|q|^2 + |x|^2) slack, and overflow its
    256-entry candidate lists into the exact fallback at k = 16 -- and with every list on the pool path."""
    rng = _rng(6100 + 2 * d + metric)
    base, gq, _ = (datagen.contest_dot if metric else datagen.contest_l2)(rng, GROUPS, PER, d)
    queries = np.ascontiguousarray(np.tile(gq, (5, 1)))
    oi, od = orc.exact_knn(base, queries, 257, metric, threads=8)
    # the contest is one: rows share the 16th float32 distance, so ids decide
    dist = np.array([[(orc.negdot if metric else orc.l2)(r, q) for r in base] for q in gq], np.float32)
    shared = (dist == od[:GROUPS, 15:16]).sum(axis=1)
    assert (shared >= 2).sum() * 2 >= GROUPS, shared
    modes = [("scan", 0, 64)] + ([("filter", 2, 1 << 20), ("pool", 2, 1)] if metric == 0 and d <= 128 else [])
    for tag, knn_filter, pool_min_k in modes:
        knn_knobs(knn_filter=knn_filter, knn_pool_min_k=pool_min_k)
        for k in (1, 16, 100, 255, 256, 257):
            _knn_equal(g, base, queries, k, metric, oi, od, (metric, d, tag))


# ---- f. graph preparation: GD pruning on the device -----------------------------------------------------------------
def _gd_equal(g, orc, koff, knbr, x, M, metric, key, host_share=100):
    """gbnns_build_graph_gd_device against the oracle's hnswlikeGD, reverse edges on and off; at most n / host_share nodes finished
    on the host."""
    for rev in (True, False):
        want_off, want_nbr = orc.hnswlike_gd(koff, knbr, x, M, metric=metric, reverse=rev, threads=8)
        off, nbr, on_host = g.build_graph_gd_device(koff, knbr, x, M, metric=metric, reverse=rev, threads=8)
        print("gd", key, M, rev, "on host", on_host, "of", len(x))
        assert np.array_equal(off, want_off) and np.array_equal(nbr, want_nbr), (key, M, rev)
        assert on_host <= len(x) // host_share, (key, M, rev, on_host)


GD_CONTEST_SHAPES = [(0, 32), (0, 44), (0, 96), (0, 128), (1, 32), (1, 128)]


@pytest.mark.parametrize("metric,d", GD_CONTEST_SHAPES, ids=["m%d_d%d" % s for s in GD_CONTEST_SHAPES])
def test_gd_pruning_on_device_contests(g, orc, metric, d):
    """gd_prune_kernel on datagen.gd_contest_l2 / gd_contest_dot (300 hubs, 4 rivals): whether a hub keeps its candidate c is
    Dist(c, hub) + eps > Dist(c, g) between two distances that are equal in real arithmetic -- the order of the roundings decides
    (tests/test_rounding_fixtures.py: a wrong order changes 10 % and more of the hubs' lists).  The graph equals the oracle's at
    M = 8 (the rivals fill the M / 2 always-linked slots) and at M = 2 (the loop stops at M kept, after the contest); no more than
    1 % of the nodes are finished on the host.  d = 44: d % 8 == 4."""
    base, (koff, knbr), _ = (datagen.gd_contest_dot if metric else datagen.gd_contest_l2)(_rng(6200 + 2 * d + metric), 300, d, 4)
    for M in (8, 2):
        _gd_equal(g, orc, koff, knbr, base, M, metric, (metric, d))


GD_FULL_SHAPES = [(32, 40, 12, 0), (128, 100, 30, 0), (14, 64, 16, 0), (16, 50, 10, 1)]


@pytest.mark.parametrize("d,K,M,metric", GD_FULL_SHAPES, ids=["d%d_K%d_M%d_m%d" % s for s in GD_FULL_SHAPES])
def test_gd_pruning_on_device_full_mantissa_vectors(g, orc, d, K, M, metric):
    """gd_prune_kernel on 3 000 full-mantissa vectors with exact K-NN lists from gbnns_exact_knn, cut to ragged lengths and shuffled
    (the builder sorts them itself): the oracle's graph, and at most 1 % of the nodes on the host.  Negative dot: signs as in
    test_gd_pruning_on_device, so that some distances are positive."""
    n = 3000
    rng = _rng(6300 + d)
    x = datagen.full_mantissa(rng, n, d)
    if metric == 1:
        x = -np.abs(x)
        x[::2] *= -1.0
    knn = g.exact_knn(x, x, K, self_offset=0)
    lists = []
    for i in range(n):
        row = knn[i][:int(rng.integers(1, K + 1))].copy()
        rng.shuffle(row)
        lists.append(row)
    koff, knbr = datagen.lists_to_csr(lists)
    _gd_equal(g, orc, koff, knbr, x, M, metric, (d, K, M, metric))
