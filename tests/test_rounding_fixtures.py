"""Which fixtures make the ORDER of the float32 roundings visible (no GPU).

DESIGN.md section 2 promises the reference's own operation order: four running sums and ((s0+s1)+s2)+s3 for
L2Metric::Dist, eight running sums, a fold and (m0+m1)+(m2+m3) for Angular::Dist, no fused multiply-add.  A parity
test pins that order only where another order would return other bits.  This file states the reference's order and
several WRONG orders as small numpy float32 functions, proves the restatement against the oracle (which kats.npz pins
to the compiled reference) bit for bit on every row it is used on, and then shows

  * that datagen.Case data cannot tell any of the orders apart (all arithmetic on it is exact),
  * that datagen.full_mantissa data can: each wrong order changes >= 10 % of the distance bit patterns,
  * that on the equal-distance contests (datagen.contest_l2 / contest_dot) each wrong order changes WHICH candidate a
    re-rank returns for >= 5 % of random 32-candidate lists,

so that tests/test_gpu_rounding.py, which runs the HIP kernels on these fixtures, would fail on a kernel that sums in
another order.  The thresholds are conditions on the reference side only; the measured shares are printed (-s).
Where the compiled reference is present it is compared with the oracle on the same inexact data.
"""
import numpy as np
import pytest

import datagen
import golden_util as gu
import oracle as orc_mod

F32 = np.float32
DIMS = (96, 128, 300, 960)


# ---- L2Metric::Dist (support_func.h:107-128) in numpy: the reference's order and wrong ones ----------------------
def _sq(rows, q):
    w = 4 * (rows.shape[1] // 4)
    e = rows[:, :w] - q[None, :w]
    assert e.dtype == F32
    return e, e * e


def _lanes(p, lanes):
    """Running sums: lane j owns columns j, j + lanes, ... of p (sequential float32 adds)."""
    steps = p.shape[1] // lanes
    if steps == 0:
        return np.zeros((p.shape[0], lanes), F32)
    # (a zero start: 0 + x = x exactly, so accumulate's first element equals the reference's 0 + p0)
    return np.add.accumulate(p[:, :steps * lanes].reshape(-1, steps, lanes), axis=1, dtype=F32)[:, -1, :]


def l2_ref(rows, q):
    _, p = _sq(rows, q)
    s = _lanes(p, 4)
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def l2_tree(rows, q):
    _, p = _sq(rows, q)
    s = _lanes(p, 4)
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def _fma_lanes(a, b, lanes):
    """Running sums with one rounding per step, s = round(s + a * b): the product of two float32 is exact in float64;
    the float64 sum rounds once more before the float32 rounding, which matters for a vanishing share of steps."""
    steps = a.shape[1] // lanes
    s = np.zeros((a.shape[0], lanes), F32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for t in range(steps):
        c = slice(t * lanes, (t + 1) * lanes)
        s = (s.astype(np.float64) + a64[:, c] * b64[:, c]).astype(F32)
    return s


def l2_fma(rows, q):
    e, _ = _sq(rows, q)
    s = _fma_lanes(e, e, 4)
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def l2_sequential(rows, q):
    _, p = _sq(rows, q)
    return _lanes(p, 1)[:, 0]


def l2_eight(rows, q):
    """Eight running sums, folded, the odd 4-wide step after the fold (the dot form's loop applied to L2)."""
    _, p = _sq(rows, q)
    w8 = 8 * (p.shape[1] // 8)
    a = _lanes(p[:, :w8], 8)
    m = a[:, 4:] + a[:, :4]
    if p.shape[1] > w8:
        m = m + p[:, w8:w8 + 4]
    return ((m[:, 0] + m[:, 1]) + m[:, 2]) + m[:, 3]


L2_WRONG_DIST = dict(tree=l2_tree, fma=l2_fma, sequential=l2_sequential)
L2_WRONG_RANK = dict(tree=l2_tree, fma=l2_fma, eight_lanes=l2_eight)


# ---- Angular::Dist (support_func.h:131-163) -------------------------------------------------------------------------
def _dot_tail(m, x, y, start):
    """The optional 4-wide step and the masked step (missing lanes add 0 * 0) onto the four sums m."""
    d = x.shape[1]
    if d - start >= 4:
        m = m + x[:, start:start + 4] * y[None, start:start + 4]
        start += 4
    if d - start > 0:
        pad = np.zeros((x.shape[0], 4), F32)
        pad[:, :d - start] = x[:, start:] * y[None, start:]
        m = m + pad
    return m


def negdot_ref(rows, q, final="tree", fma=False):
    d8 = 8 * (rows.shape[1] // 8)
    a = _fma_lanes(rows[:, :d8], np.broadcast_to(q[None, :d8], (rows.shape[0], d8)), 8) if fma else \
        _lanes(rows[:, :d8] * q[None, :d8], 8)
    m = _dot_tail(a[:, 4:] + a[:, :4], rows, q, d8)
    if final == "left":
        return -(((m[:, 0] + m[:, 1]) + m[:, 2]) + m[:, 3])
    return -((m[:, 0] + m[:, 1]) + (m[:, 2] + m[:, 3]))


def negdot_four(rows, q):
    d4 = 4 * (rows.shape[1] // 4)
    m = _dot_tail(_lanes(rows[:, :d4] * q[None, :d4], 4), rows, q, d4)
    return -((m[:, 0] + m[:, 1]) + (m[:, 2] + m[:, 3]))


DOT_WRONG = dict(fma=lambda r, q: negdot_ref(r, q, fma=True), left_final=lambda r, q: negdot_ref(r, q, final="left"),
                 four_lanes=negdot_four)


def _oracle_dists(orc, rows, q, metric=0):
    f = orc.negdot if metric else orc.l2
    return np.array([f(r, q) for r in rows], F32)


def _changed_share(orc, base, queries):
    """Share of the (row, query) distances whose bits change under each wrong L2 order (and the inexact share: the
    distances that differ from the float64 sum of the same squares)."""
    changed = {k: 0 for k in L2_WRONG_DIST}
    inexact = total = 0
    for q in queries:
        want = l2_ref(base, q)
        assert np.array_equal(gu.bits(want), gu.bits(_oracle_dists(orc, base, q)))   # the restatement IS the oracle's order
        w = 4 * (base.shape[1] // 4)
        e = base[:, :w].astype(np.float64) - q[None, :w].astype(np.float64)
        inexact += int(((e * e).sum(1) != want.astype(np.float64)).sum())
        for k, f in L2_WRONG_DIST.items():
            changed[k] += int((gu.bits(f(base, q)) != gu.bits(want)).sum())
        total += base.shape[0]
    return {k: v / total for k, v in changed.items()}, inexact / total


@pytest.mark.parametrize("d", DIMS)
def test_case_data_cannot_tell_summation_orders_apart(orc, d):
    """Why the new fixtures are needed: on datagen.Case data (coordinates k / 256, |k| <= 88) every difference, square and
    partial sum is exact, so the tree, fused multiply-add and one sequential sum all return the reference's bits."""
    c = datagen.Case("x", 7000 + d, 3000, 20, d, 8, 8)
    changed, inexact = _changed_share(orc, c.base, c.queries)
    print("Case d=%d: inexact %.4f changed %s" % (d, inexact, changed))
    assert inexact == 0 and all(v == 0 for v in changed.values()), (d, inexact, changed)


@pytest.mark.parametrize("d", DIMS)
def test_full_mantissa_data_tells_summation_orders_apart(orc, d):
    rng = np.random.Generator(np.random.PCG64(7100 + d))
    base = datagen.full_mantissa(rng, 3000, d)
    queries = datagen.full_mantissa(rng, 20, d)
    changed, inexact = _changed_share(orc, base, queries)
    print("full_mantissa d=%d: inexact %.4f changed %s" % (d, inexact, changed))
    assert inexact > 0.99, (d, inexact)
    assert all(v >= 0.10 for v in changed.values()), (d, changed)


def test_full_mantissa_net_is_inexact_from_layer_one(orc):
    """net_layers_full: already the layer-1 pre-activations of an exact (Case) input round, those of a full-mantissa
    input all the more; with net_layers on Case inputs they are exact."""
    rng = np.random.Generator(np.random.PCG64(7200))
    d, dh = 128, 64
    exact_in = datagen.Case("x", 7201, 10, 40, d, 8, dh)
    full_in = datagen.full_mantissa(rng, 40, d)
    l1_full = datagen.net_layers_full(rng, d, dh, 8)[0]

    def inexact_share(l1, x):
        pre64 = x.astype(np.float64) @ l1[:, :d].astype(np.float64).T          # (exact products, 53-bit sums)
        pre32 = np.stack([-negdot_ref(np.ascontiguousarray(l1[:, :d]), q) for q in x])
        return float((pre64 != pre32.astype(np.float64)).mean())

    assert inexact_share(exact_in.net[0], exact_in.queries) == 0
    assert inexact_share(l1_full, exact_in.queries) > 0.9
    assert inexact_share(l1_full, full_in) > 0.9
    for l in datagen.net_layers_full(rng, 45, 27, 14):
        assert np.abs(l).max() <= 0.25 and len(np.unique(l)) > l.size // 2


def _contest_lists(rng, group, n_lists, length):
    """n_lists candidate lists of `length` distinct rows of one group each, in random order -> (cand, group of list)."""
    groups = int(group.max()) + 1
    per = len(group) // groups
    gl = rng.integers(0, groups, size=n_lists)
    cand = np.stack([g * per + rng.permutation(per)[:length] for g in gl]).astype(np.uint32)
    return cand, gl


def _winners(dist_of_row, cand):
    """getRealNearest: the strict minimum in pop order, i.e. the FIRST minimum of the list."""
    return cand[np.arange(len(cand)), np.argmin(dist_of_row[cand], axis=1)]


def _contest_check(orc, base, queries, group, metric, ref_fn, wrong, key):
    rng = np.random.Generator(np.random.PCG64(7300 + base.shape[1] + metric))
    groups = len(queries)
    per = len(group) // groups
    dist = {name: np.empty(len(base), F32) for name in ("ref", *wrong)}
    for g in range(groups):
        rows = base[g * per:(g + 1) * per]
        dist["ref"][g * per:(g + 1) * per] = ref_fn(rows, queries[g])
        assert np.array_equal(gu.bits(dist["ref"][g * per:(g + 1) * per]), gu.bits(_oracle_dists(orc, rows, queries[g], metric))), key
        for name, f in wrong.items():
            dist[name][g * per:(g + 1) * per] = f(rows, queries[g])
        # equidistant in real arithmetic: the exact sums of the group agree (integers scaled by a power of two)
        w = base.shape[1] if metric else 4 * (base.shape[1] // 4)
        num = np.round(rows[:, :w].astype(np.float64) * 2.0**23).astype(np.int64).astype(object)
        qn = np.round(queries[g][:w].astype(np.float64) * 2.0**23).astype(np.int64).astype(object)
        real = (num * qn[None, :]).sum(1) if metric else ((num - qn[None, :]) ** 2).sum(1)
        assert len(set(real.tolist())) == 1, key
    cand, gl = _contest_lists(rng, group, 512, 32)
    distinct = np.array([len(np.unique(gu.bits(dist["ref"][c]))) for c in cand])
    share_distinct = float((distinct >= 2).mean())
    win = _winners(dist["ref"], cand)
    assert np.array_equal(win, orc.rerank(queries[gl], cand, None, base, metric=metric)), key
    moved = {name: float((_winners(dist[name], cand) != win).mean()) for name in wrong}
    print("contest %s: distinct values per list %d..%d, lists with >= 2: %.3f, winner moved %s"
          % (key, distinct.min(), distinct.max(), share_distinct, moved))
    assert share_distinct >= 0.90, (key, share_distinct)
    assert all(v >= 0.05 for v in moved.values()), (key, moved)


@pytest.mark.parametrize("d", DIMS)
def test_contest_l2_winner_depends_on_rounding_order(orc, d):
    rng = np.random.Generator(np.random.PCG64(7400 + d))
    base, queries, group = datagen.contest_l2(rng, 8, 256, d)
    _contest_check(orc, base, queries, group, 0, l2_ref, L2_WRONG_RANK, ("l2", d))


@pytest.mark.parametrize("d", (45, 200, 300))
def test_contest_dot_winner_depends_on_rounding_order(orc, d):
    rng = np.random.Generator(np.random.PCG64(7500 + d))
    base, queries, group = datagen.contest_dot(rng, 8, 256, d)
    _contest_check(orc, base, queries, group, 1, negdot_ref, DOT_WRONG, ("dot", d))


def test_contest_l2_ignores_the_tail(orc):
    """d = 45: the 45th coordinate is arbitrary jitter that L2Metric::Dist never reads; the rows stay equidistant over
    the 44 it does read (checked in real arithmetic by _contest_check) and the contest stays a contest."""
    rng = np.random.Generator(np.random.PCG64(7445))
    base, queries, group = datagen.contest_l2(rng, 8, 256, 45)
    assert len(np.unique(base[:256, 44])) > 200
    _contest_check(orc, base, queries, group, 0, l2_ref, L2_WRONG_RANK, ("l2", 45))


def test_new_generators_are_reproducible_and_additive():
    """Same seed, same bytes; and the generators the golden fixtures hash are untouched (tests/golden/*.npz store the
    sha256 of the regenerated Case inputs: test_oracle_golden.py checks them)."""
    def make(seed):
        rng = np.random.Generator(np.random.PCG64(seed))
        return [datagen.full_mantissa(rng, 50, 20), *datagen.net_layers_full(rng, 20, 16, 8),
                *datagen.contest_l2(rng, 2, 8, 13), *datagen.contest_dot(rng, 2, 8, 13), *datagen.contest_graph(rng, 2, 8, 1, 4),
                *(x for gen, d in ((datagen.gd_contest_l2, 13), (datagen.gd_contest_dot, 16)) for b, csr, hubs in [gen(rng, 3, d, 2)]
                  for x in (b, *csr, hubs))]
    a, b = make(5), make(5)
    assert [datagen.sha(x) for x in a] == [datagen.sha(x) for x in b]
    assert all(x.dtype == F32 for x in a[:5]) and a[-8].dtype == F32 and a[-4].dtype == F32
    # the GD contests: clusters of rivals + 2 consecutive ids, one hub each, every list inside its cluster
    for b, off, nbr, hubs in (a[-8:-4], a[-4:]):
        assert b.shape[0] == 12 and np.array_equal(hubs // 4, np.arange(3)) and off[-1] == len(nbr) == 3 * (3 + 1 + 2 * 3)
        assert all((nbr[int(off[i]):int(off[i + 1])] // 4 == i // 4).all() and i not in nbr[int(off[i]):int(off[i + 1])] for i in range(12))
    fm = a[0]
    # ~22 significant bits: the numerators over 2^23 are mostly odd multiples of small powers of two
    num = np.round(fm.astype(np.float64) * 2.0**23).astype(np.int64)
    assert np.array_equal((num.astype(np.float64) / 2.0**23).astype(F32), fm)
    assert (num % 16 != 0).mean() > 0.9 and np.abs(fm).max() < 0.36


# ---- the oracle itself against the compiled reference on the same inexact data -----------------------------------
@pytest.mark.parametrize("d", (128, 300, 960))
def test_reference_walk_in_the_original_space_on_full_mantissa_data(orc, ref, d):
    rng = np.random.Generator(np.random.PCG64(7600 + d))
    n, nq = 2000, 64
    base = datagen.full_mantissa(rng, n, d)
    queries = datagen.full_mantissa(rng, nq, d)
    off, nbr = datagen.random_graph(rng, n, 2, 30)
    ent = rng.integers(0, n, size=nq).astype(np.uint32)
    for ef in (8, 100):
        a = orc.walk(queries, base, off, nbr, ef, entries=ent, threads=4)
        b = ref.walk(queries, base, off, nbr, ef, entries=ent, threads=4)
        assert np.array_equal(a["ids"], b["ids"]), (d, ef)
        assert np.array_equal(gu.bits(a["dists"]), gu.bits(b["dists"])), (d, ef)
        assert np.array_equal(a["hops"], b["hops"]) and np.array_equal(a["dist_calc"], b["dist_calc"]), (d, ef)


@pytest.mark.parametrize("shape", ((128, 256, 32), (200, 72, 32), (45, 27, 14), (960, 1024, 64)))
def test_reference_projection_on_full_mantissa_data(orc, ref, shape):
    d, dh, dlow = shape
    rng = np.random.Generator(np.random.PCG64(7700 + d))
    x = datagen.full_mantissa(rng, 100, d)
    net = datagen.net_layers_full(rng, d, dh, dlow)
    assert np.array_equal(gu.bits(orc.project(net, x)), gu.bits(ref.project(net, x)))


@pytest.mark.parametrize("metric,d", ((0, 128), (0, 300), (0, 960), (1, 200)))
def test_reference_two_stage_search_on_a_contest_index(orc, ref, metric, d):
    rng = np.random.Generator(np.random.PCG64(7800 + d))
    groups, per, dlow = 8, 256, 32
    base, queries, group = (datagen.contest_dot if metric else datagen.contest_l2)(rng, groups, per, d)
    db_low = datagen.full_mantissa(rng, groups * per, dlow)
    off, nbr = datagen.contest_graph(rng, groups, per, 2, 30)
    qg = np.repeat(np.arange(groups), 6)
    q_low = datagen.full_mantissa(rng, len(qg), dlow)
    ent = (qg * per + rng.integers(0, per, size=len(qg))).astype(np.uint32)
    for ef in (8, 64, 200):
        kw = dict(db_low=db_low, q_low=q_low, entries=ent, metric=metric)
        a = orc.search_batch(orc_mod.MODE_LOWQ, queries[qg], base, off, nbr, ef, **kw)
        b = ref.search_batch(orc_mod.MODE_LOWQ, queries[qg], base, off, nbr, ef, **kw)
        for k in ("ids", "hops", "dist_calc"):
            assert np.array_equal(a[k], b[k]), (metric, d, ef, k)
        assert (group[a["ids"]] == qg).all()    # (disconnected components: the answer is a row of the query's own group)


# ---- graph preparation: hnswlikeGD's pruning and the exact kNN on inexact data -------------------------------------
EPS = F32(1e-10)        # getEps(), support_func.h:41-43, as the float the reference adds and compares


def gd_numpy(koff, knbr, ds, M, dist, reverse=True, nodes=None):
    """hnswlikeGD (support_func.h:529-563) and addReverseEdgesForGD (:417-442) with the distance as a parameter: dist(rows, q)
    -> float32 [rows].  std::sort on the distance alone is an insertion sort -- a stable one -- for the lists of up to 16
    entries this is used on.  nodes: prune these only, no reverse pass.  Returns the adjacency lists."""
    n = len(koff) - 1
    out = {}
    for i in (range(n) if nodes is None else nodes):
        cand = knbr[int(koff[i]):int(koff[i + 1])]
        assert len(cand) <= 16
        di = dist(ds[cand], ds[i])
        keep = di > EPS
        cand = cand[keep][np.argsort(di[keep], kind="stable")]
        di = np.sort(di[keep], kind="stable")
        g = [int(cand[0])] if len(cand) else []
        for c, dci in zip(cand[1:], di[1:]):
            if len(g) == M:
                break
            assert gu.bits(dist(ds[[i]], ds[c]))[0] == gu.bits(dci)       # Dist(c, i) is Dist(i, c) bit for bit
            if not (F32(dci + EPS) > dist(ds[g], ds[c])).any():
                g.append(int(c))
        g += [int(c) for c in cand[:M // 2] if c not in g]
        out[i] = g
    if nodes is not None or not reverse:
        return out
    rev = np.zeros(n, np.int64)
    for g in out.values():
        rev[g] += 1
    for i in range(n):
        thr = min(M - int(rev[i]), M // 2)
        if thr > 0:
            for c in list(out[i]):
                if len(out[c]) < 2 * M and i not in out[c]:
                    out[c].append(i)
                    thr -= 1
                    if thr <= 0:
                        break
    return out


def _adj(off, nbr):
    return {i: [int(v) for v in nbr[int(off[i]):int(off[i + 1])]] for i in range(len(off) - 1)}


def _tied_nodes(orc, koff, knbr, ds, metric):
    """Nodes whose candidate list holds two equal float32 distances above eps under the oracle's Dist."""
    tied = 0
    for i in range(len(koff) - 1):
        di = _oracle_dists(orc, ds[knbr[int(koff[i]):int(koff[i + 1])]], ds[i], metric)
        di = di[di > EPS]
        tied += len(np.unique(gu.bits(di))) != len(di)
    return tied


GD_HUBS = 300
GD_L2_WRONG = dict(L2_WRONG_DIST, eight_lanes=l2_eight)


def _same_graph(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _gd_contest(metric, d, rivals):
    gen = datagen.gd_contest_dot if metric else datagen.gd_contest_l2
    return gen(np.random.Generator(np.random.PCG64(7900 + 10 * d + rivals + metric)), GD_HUBS, d, rivals)


def _gd_contest_check(orc, lib, metric, d, rivals):
    ref_fn, wrong = (negdot_ref, DOT_WRONG) if metric else (l2_ref, GD_L2_WRONG)
    base, (koff, knbr), hubs = _gd_contest(metric, d, rivals)
    key = ("dot" if metric else "l2", d, rivals)
    n, M = len(base), 2 * rivals
    tied = _tied_nodes(orc, koff, knbr, base, metric)
    for m, rev in ((M, True), (M, False), (2, True)):
        want = orc.hnswlike_gd(koff, knbr, base, m, metric=metric, reverse=rev, threads=2)
        assert gd_numpy(koff, knbr, base, m, ref_fn, reverse=rev) == _adj(*want), (key, m, rev)
        assert _same_graph(lib.build_graph_gd(koff, knbr, base, m, metric=metric, reverse=rev, threads=3), want), (key, m, rev)
    pruned = gd_numpy(koff, knbr, base, M, ref_fn, nodes=hubs)
    c_kept = float(np.mean([len(pruned[h]) == rivals + 1 for h in hubs]))
    changed = {name: float(np.mean([g != pruned[h] for h, g in gd_numpy(koff, knbr, base, M, f, nodes=hubs).items()]))
               for name, f in wrong.items()}
    print("gd contest %s: nodes with a float32 tie %d of %d, c kept at %.3f of hubs, hubs changed %s" % (key, tied, n, c_kept, changed))
    assert tied <= n // 100, (key, tied, n)
    assert all(v >= 0.05 for v in changed.values()), (key, changed)


@pytest.fixture(scope="module")
def host_lib():
    import gbnns_dim_red_amd as g
    g.build_library()
    g.load_library()
    return g


@pytest.mark.parametrize("d,rivals", ((32, 4), (96, 3), (128, 4), (44, 4)))
def test_gd_contest_l2_pruning_depends_on_rounding_order(orc, host_lib, d, rivals):
    """hnswlikeGD on datagen.gd_contest_l2 at M = 2 * rivals (and at M = 2, where the loop stops at `size == M`): the numpy
    restatement with L2Metric::Dist's order gives the oracle's graph, and so does the library's host builder; each wrong order
    changes the adjacency list of >= 5 % of the hubs; at most 1 % of the nodes have a float32 tie in their list (such a node is
    finished by the host's std::sort and tests nothing on the device).  The thresholds are conditions on the fixture."""
    _gd_contest_check(orc, host_lib, 0, d, rivals)


@pytest.mark.parametrize("d", (32, 96, 128, 200))
def test_gd_contest_dot_pruning_depends_on_rounding_order(orc, host_lib, d):
    _gd_contest_check(orc, host_lib, 1, d, 4)


def _full_mantissa_lists(orc, seed, n, d, K):
    """full_mantissa vectors and their exact K-NN lists (self excluded) in CSR."""
    x = datagen.full_mantissa(np.random.Generator(np.random.PCG64(seed)), n, d)
    knn, _ = orc.exact_knn(x, x, K, 0, self_offset=0, threads=4)
    return x, datagen.dense_to_csr(knn)


@pytest.mark.parametrize("d", (14, 32, 128))
def test_host_builder_on_full_mantissa_data(orc, host_lib, d):
    """graph_build.cpp against the oracle on vectors whose distances round at every step (exact 40-NN lists, M = 12)."""
    x, (koff, knbr) = _full_mantissa_lists(orc, 8000 + d, 1500, d, 40)
    for rev in (True, False):
        want = orc.hnswlike_gd(koff, knbr, x, 12, reverse=rev, threads=2)
        assert _same_graph(host_lib.build_graph_gd(koff, knbr, x, 12, reverse=rev, threads=3), want), (d, rev)


@pytest.mark.parametrize("metric,d", ((0, 32), (0, 128), (0, 44), (1, 32), (1, 128)))
def test_reference_gd_on_the_contests(orc, ref, host_lib, metric, d):
    """The compiled reference's hnswlikeGD, the oracle and the host builder on the contests: one graph.  At M = 2: the reference
    links its M / 2 nearest without looking at the length of the list (support_func.h:559-563), so it can only be run where every
    list holds that many; the contest is met at M = 2 as well (the dot form always, L2 where the second rival is pruned)."""
    base, (koff, knbr), _ = _gd_contest(metric, d, 4)
    for rev in (True, False):
        want = ref.hnswlike_gd(koff, knbr, base, 2, metric=metric, reverse=rev, threads=2)
        assert _same_graph(orc.hnswlike_gd(koff, knbr, base, 2, metric=metric, reverse=rev, threads=2), want), (metric, d, rev)
        assert _same_graph(host_lib.build_graph_gd(koff, knbr, base, 2, metric=metric, reverse=rev, threads=3), want), (metric, d, rev)


@pytest.mark.parametrize("d", (14, 32, 128))
def test_reference_gd_on_full_mantissa_data(orc, ref, host_lib, d):
    x, (koff, knbr) = _full_mantissa_lists(orc, 8000 + d, 1500, d, 40)
    for rev in (True, False):
        want = ref.hnswlike_gd(koff, knbr, x, 12, reverse=rev, threads=2)
        assert _same_graph(orc.hnswlike_gd(koff, knbr, x, 12, reverse=rev, threads=2), want), (d, rev)
        assert _same_graph(host_lib.build_graph_gd(koff, knbr, x, 12, reverse=rev, threads=3), want), (d, rev)


# ---- the exact kNN on the equal-distance contests ----------------------------------------------------------------------
def _topk(dist, k):
    """ids of the k smallest (distance, id) pairs per row of dist: a stable sort of the distances, ids being ascending."""
    return np.argsort(dist, axis=1, kind="stable")[:, :k].astype(np.uint32)


def _knn_contest(metric, d):
    rng = np.random.Generator(np.random.PCG64(8100 + 2 * d + metric))
    return (datagen.contest_dot if metric else datagen.contest_l2)(rng, 8, 256, d)


KNN_CONTESTS = ((0, 32), (0, 100), (0, 128), (0, 300), (1, 32), (1, 200))


@pytest.mark.parametrize("metric,d", KNN_CONTESTS)
def test_contest_knn_lists_depend_on_rounding_order(orc, metric, d):
    """The k nearest rows of a contest group's query (8 groups x 256 rows, the groups' own queries): the numpy restatement's
    (distance, id)-ordered lists equal orc.exact_knn's, ids and distance bits, and each wrong order changes the id list of >= 50 %
    of the queries at k = 16 and at k = 100."""
    ref_fn, wrong = (negdot_ref, DOT_WRONG) if metric else (l2_ref, GD_L2_WRONG)
    base, queries, _ = _knn_contest(metric, d)
    dist = {name: np.stack([f(base, q) for q in queries]) for name, f in dict(wrong, ref=ref_fn).items()}
    for k in (16, 100):
        want = _topk(dist["ref"], k)
        oi, od = orc.exact_knn(base, queries, k, metric, threads=4)
        assert np.array_equal(want, oi), (metric, d, k)
        assert np.array_equal(gu.bits(np.take_along_axis(dist["ref"], want.astype(np.int64), axis=1)), gu.bits(od)), (metric, d, k)
        moved = {name: float((_topk(dist[name], k) != want).any(axis=1).mean()) for name in wrong}
        at_kth = (dist["ref"] == od[:, -1:]).sum(axis=1)
        print("knn contest metric %d d=%d k=%d: rows at the k-th distance %s, id list changed %s" % (metric, d, k, at_kth.tolist(), moved))
        assert all(v >= 0.5 for v in moved.values()), (metric, d, k, moved)


@pytest.mark.parametrize("metric,d", KNN_CONTESTS)
def test_reference_get_truth_on_the_contests(orc, ref, metric, d):
    base, queries, _ = _knn_contest(metric, d)
    assert np.array_equal(ref.get_truth(base, queries, metric=metric), orc.exact_knn(base, queries, 1, metric, threads=4)[0][:, 0]), (metric, d)
