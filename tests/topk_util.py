"""What tests/test_topk_cpu.py and tests/test_gpu_topk.py share: the fixtures (the recipes of tests/test_gpu_rounding.py, rebuilt here)
and the expected rows of gbnns_rerank_topk / gbnns_search_topk, computed on the CPU with the oracle's scalar distances.

Expected row of a list: dist_r = orc.l2 / orc.negdot (base[cand_r], q) for the pop indices r < count, the order
np.lexsort((r, dist_r))[:k] -- NumPy compares -0 == +0, as the library's keys do -- then 0xFFFFFFFF / +inf from column count on.
"""
import functools

import numpy as np

import datagen

GROUPS, PER = 8, 256       # the contests: 8 groups x 256 rows
NONE = 0xFFFFFFFF
RERANK_COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 200)
# every distance form of the re-rank: 128 the pair form, 960 its DEEP = 24 form, 388 DEEP = 24 plus the even lane's odd step, 300 L2
# d % 8 == 4, 300 dot a lane per row, 200 dot the pair form's eight sums over two lanes, 45 a lane per row with the tail ignored / masked
RERANK_SHAPES = [(128, 0), (960, 0), (388, 0), (300, 0), (300, 1), (200, 1), (45, 0), (45, 1)]


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


@functools.lru_cache(maxsize=None)
def rerank_contest(d, metric):
    """base, queries [nq x d], cand [nq x 200] (own group's rows in random order, 0xFFFFFFFF beyond count), count: twelve
    queries per entry of RERANK_COUNTS.  Candidates of a list are equidistant from its query in real arithmetic."""
    rng = rng_of(5300 + 2 * d + metric)
    base, gq, _ = (datagen.contest_dot if metric else datagen.contest_l2)(rng, GROUPS, PER, d)
    count = np.repeat(np.array(RERANK_COUNTS, np.int32), 12)
    qg = rng.integers(0, GROUPS, size=len(count))
    cand = np.full((len(count), max(RERANK_COUNTS)), NONE, np.uint32)
    for i, (c, grp) in enumerate(zip(count, qg)):
        cand[i, :c] = grp * PER + rng.permutation(PER)[:c]
    return base, np.ascontiguousarray(gq[qg]), cand, count


def list_distances(orc, base, q, cand, count, metric, memo=None):
    """[nq x stride] float32: the oracle's scalar distance of every candidate below its list's count, +inf beyond.  Rows that
    share (query, id) are computed once (`memo`: a dict to share them between calls over the same base)."""
    f = orc.negdot if metric else orc.l2
    out = np.full(cand.shape, np.inf, np.float32)
    memo = {} if memo is None else memo
    for i in range(len(cand)):
        qkey = q[i].tobytes()
        for r in range(int(count[i])):
            key = (qkey, int(cand[i, r]))
            if key not in memo:
                memo[key] = f(base[cand[i, r]], q[i])
            out[i, r] = memo[key]
    return out


def expected_topk(dist, cand, count, k):
    """ids [nq x k] uint32 and distances [nq x k] float32 of the contract, from list_distances' rows."""
    ids = np.full((len(cand), k), NONE, np.uint32)
    dd = np.full((len(cand), k), np.inf, np.float32)
    for i in range(len(cand)):
        c = int(count[i])
        order = np.lexsort((np.arange(c), dist[i, :c]))[:k]
        ids[i, :len(order)] = cand[i, order]
        dd[i, :len(order)] = dist[i, order]
    return ids, dd


def float64_distances(base, q, cand, count, metric):
    """The same distances accumulated in float64 and rounded once: the arithmetic a host that redoes them with NumPy gets."""
    d = base.shape[1]
    dd = d - d % 4 if metric == 0 else d   # (L2Metric::Dist ignores the d % 4 tail)
    out = np.full(cand.shape, np.inf, np.float32)
    for i in range(len(cand)):
        c = int(count[i])
        rows = base[cand[i, :c]].astype(np.float64)
        qi = q[i].astype(np.float64)
        out[i, :c] = (((rows[:, :dd] - qi[:dd]) ** 2).sum(1) if metric == 0 else -(rows @ qi)).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def contest_index_data(metric, d, dlow):
    """A contest index: original-space rows from contest_l2 / contest_dot, independent full-mantissa low-dimensional rows, the groups
    disconnected components of the graph; twelve queries per group that share the group's original-space query and differ in their
    low-dimensional query and entry point; a full-mantissa net."""
    rng = rng_of(5500 + 7 * d + 3 * dlow + metric)
    base, gq, group = (datagen.contest_dot if metric else datagen.contest_l2)(rng, GROUPS, PER, d)
    db_low = datagen.full_mantissa(rng, GROUPS * PER, dlow)
    off, nbr = datagen.contest_graph(rng, GROUPS, PER, 2, 30)
    qg = np.repeat(np.arange(GROUPS), 12)
    q_low = datagen.full_mantissa(rng, len(qg), dlow)
    ent = (qg * PER + rng.integers(0, PER, size=len(qg))).astype(np.uint32)
    net = datagen.net_layers_full(rng, d, 64, dlow)
    return dict(base=base, gq=gq, group=group, db_low=db_low, off=off, nbr=nbr, qg=qg, queries=np.ascontiguousarray(gq[qg]), q_low=q_low,
                ent=ent, net=net)
