"""Deterministic, bit-portable test inputs.

Everything here is built from numpy's PCG64 integer stream and exact integer->float32
conversions (no libm, no BLAS), so the same seed gives the same bytes on every host; the golden
fixtures store a sha256 of the regenerated inputs to prove it.

Two families.  `clustered`, `lattice` and `net_layers` (the `Case` kinds, the golden fixtures) emit
small dyadic rationals -- coordinates k/256 with |k| <= 88, weights k/2^s with |k| <= 128 -- on which
every difference, square and partial sum of a distance is exact in float32: they pin ids, ties,
hops and counters, but ANY summation order returns their distance bits.  `full_mantissa`,
`net_layers_full`, `contest_l2` and `contest_dot` carry 20 and more significant bits per number, so
that the order of the roundings shows: in the distance bits, and (the contests) in which candidate
a re-rank returns.  tests/test_rounding_fixtures.py proves both statements on the CPU.
"""
import hashlib

import numpy as np


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi, size=shape, dtype=np.int64)


def clustered(rng, n, d, n_centers=16, spread=40, scale=256.0):
    """n points around integer-grid centres (overlapping clusters, so kNN graphs stay connected);
    every coordinate is an exact multiple of 1/scale."""
    centers = _ints(rng, (n_centers, d), -12, 13)
    assign = _ints(rng, (n,), 0, n_centers)
    noise = _ints(rng, (n, d), -spread, spread + 1)
    return ((centers[assign] * 4 + noise).astype(np.float32) / np.float32(scale)).astype(np.float32)


def lattice(rng, n, d, levels=3, dup=3):
    """Small-integer coordinates with every vector repeated `dup` times: distances are small
    exact integers, so equal-distance ties (and exact duplicates) are everywhere."""
    m = (n + dup - 1) // dup
    base = _ints(rng, (m, d), 0, levels).astype(np.float32)
    out = np.repeat(base, dup, axis=0)[:n]
    perm = np.argsort(_ints(rng, (n,), 0, 1 << 40), kind="stable")
    return np.ascontiguousarray(out[perm])


def net_layers(rng, d, dh, dlow):
    """Three [d_out x (d_in+1)] layers (weights | bias), dyadic-rational entries."""
    def layer(dout, din, shift):
        w = _ints(rng, (dout, din + 1), -128, 129).astype(np.float32)
        return (w / np.float32(1 << shift)).astype(np.float32)
    # shifts keep activations O(1) for inputs of magnitude ~1
    s1 = 7 + max(0, int(np.log2(max(d, 2))) // 2)
    s2 = 7 + max(0, int(np.log2(max(dh, 2))) // 2)
    return layer(dh, d, s1), layer(dh, dh, s2), layer(dlow, dh, s2)


def full_mantissa(rng, n, d, n_centers=16, spread=40):
    """`clustered`'s geometry (same centres / noise recipe, same [-0.35, 0.35] range) with about 22
    significant bits per coordinate: the grid value times 2^15 plus a jitter from [-2^14, 2^14),
    over 2^23.  Squares and partial sums of such coordinates round at every step."""
    centers = _ints(rng, (n_centers, d), -12, 13)
    assign = _ints(rng, (n,), 0, n_centers)
    noise = _ints(rng, (n, d), -spread, spread + 1)
    v = (centers[assign] * 4 + noise) * (1 << 15) + _ints(rng, (n, d), -(1 << 14), 1 << 14)
    assert np.abs(v).max(initial=0) < (1 << 24)     # integer -> float32 stays exact
    return (v.astype(np.float32) / np.float32(1 << 23)).astype(np.float32)


def net_layers_full(rng, d, dh, dlow):
    """`net_layers` with about 20 significant bits per weight and bias (an integer of +-2^20 over a
    power of two, same magnitudes): layer 1 is inexact already on exact inputs."""
    def layer(dout, din, shift):
        w = _ints(rng, (dout, din + 1), -(1 << 20), (1 << 20) + 1).astype(np.float32)
        return (w / np.float32(1 << (shift + 13))).astype(np.float32)
    s1 = 7 + max(0, int(np.log2(max(d, 2))) // 2)
    s2 = 7 + max(0, int(np.log2(max(dh, 2))) // 2)
    return layer(dh, d, s1), layer(dh, dh, s2), layer(dlow, dh, s2)


def _permuted_rows(rng, v, per_group, width):
    """per_group copies of v, the first `width` entries of each under a fresh permutation."""
    rows = np.repeat(v[None, :], per_group, axis=0)
    for r in range(per_group):
        rows[r, :width] = v[:width][rng.permutation(width)]
    return rows


def contest_l2(rng, groups, per_group, d):
    """The equal-distance contest for L2Metric::Dist.  Group g has one query, ((80 + m) << 17) / 2^23
    with m in [0, 32]^d (coordinates in [1.25, 1.75]), and per_group rows query + pi(j) / 2^23 with
    j in (-2^21, 2^21)^d and a fresh permutation pi per row over the 4 * floor(d / 4) coordinates
    the reference reads (the rest: arbitrary jitter, which must not matter).  All numerators lie in
    [2^23, 2^24): conversions and row - query are exact, so in real arithmetic every row of a group
    is equidistant from its query, and in float32 the distances are a few values some ulp apart --
    decided by the order of the roundings alone.  Returns base [groups * per_group x d] (group-major),
    queries [groups x d], group [groups * per_group]."""
    width = 4 * (d // 4)
    base = np.empty((groups * per_group, d), np.int64)
    queries = np.empty((groups, d), np.int64)
    for g in range(groups):
        m = _ints(rng, (d,), 0, 33)
        j = _ints(rng, (d,), -(1 << 21) + 1, 1 << 21)
        q = (80 + m) << 17
        rows = _permuted_rows(rng, j, per_group, width)
        rows[:, width:] = _ints(rng, (per_group, d - width), -(1 << 21) + 1, 1 << 21)
        queries[g] = q
        base[g * per_group:(g + 1) * per_group] = q[None, :] + rows
    assert base.min() >= (1 << 23) and base.max() < (1 << 24)
    f = lambda a: (a.astype(np.float32) / np.float32(1 << 23)).astype(np.float32)
    return f(base), f(queries), np.repeat(np.arange(groups, dtype=np.int64), per_group)


def contest_dot(rng, groups, per_group, d):
    """The equal-distance contest for Angular::Dist.  Every query is c * (1, ..., 1) with
    c = 11184811 / 2^23 (1.333..., a full mantissa); the rows of a group are permutations of one vector
    of integers from (-2^23, 2^23) over 2^23 -- all d coordinates, the masked tail takes part.  The
    real dot products of a group are equal; every float32 product rounds.  Returns as contest_l2."""
    base = np.empty((groups * per_group, d), np.int64)
    for g in range(groups):
        v = _ints(rng, (d,), -(1 << 23) + 1, 1 << 23)
        base[g * per_group:(g + 1) * per_group] = _permuted_rows(rng, v, per_group, d)
    f = lambda a: (a.astype(np.float32) / np.float32(1 << 23)).astype(np.float32)
    queries = f(np.full((groups, d), 11184811, np.int64))
    return f(base), queries, np.repeat(np.arange(groups, dtype=np.int64), per_group)


def _gd_contest_lists(rng, hubs, rivals):
    """Node ids and candidate lists of the GD contests.  A cluster is rivals + 2 consecutive ids under a fresh permutation:
    slot[0] the hub, slot[1] the candidate c, slot[2:] the rivals g_1 .. g_rivals.  Lists (each shuffled: the builder sorts
    them itself): hub -> all its satellites; g_t -> hub, c and the other g; c -> the hub alone (its distances to the hub and to
    every g_t are equal in real arithmetic: two of them tie in float32 at two nodes c of three, and a node with a tie is not
    decided on the device).  Every cluster is a component of its own."""
    size = rivals + 2
    slots = np.stack([h * size + rng.permutation(size) for h in range(hubs)])
    lists = [None] * (hubs * size)
    for s in slots:
        lists[s[0]] = s[1:][rng.permutation(size - 1)]
        lists[s[1]] = s[:1]
        for t in range(rivals):
            other = np.concatenate([s[:2 + t], s[3 + t:]])
            lists[s[2 + t]] = other[rng.permutation(size - 1)]
    return slots, lists_to_csr(lists)


def gd_contest_l2(rng, hubs, d, rivals=4):
    """The equal-distance contest for hnswlikeGD's pruning test  Dist(c, i) + eps > Dist(c, g)  under L2Metric::Dist.  Per
    hub i = Q / 2^23 with Q = (96 + m) << 17, m in [0, 12]^d: one candidate c = Q + v with v = 2^19 + r, r in [0, 2^19)^d, and
    `rivals` nodes g_t = Q + v - pi_t(v), a fresh permutation pi_t each over the 4 * floor(d / 4) coordinates the reference
    reads (the rest: arbitrary jitter).  All numerators lie in [2^23, 2^24): conversions and differences are exact, c - g_t =
    pi_t(v), so Dist(c, i) = Dist(c, g_t) in real arithmetic and a few ulp apart in float32 -- which is larger is decided by the
    order of the roundings alone.  Dist(i, g_t) is about 0.07 Dist(i, c): the g_t sort first (and fill the M / 2 always-linked
    slots at M = 2 * rivals), c comes last and its survival is the contest; at a g_t, c meets the hub in the same way.
    Returns base [hubs * (rivals + 2) x d], (offsets, neighbours) of the candidate lists, hub ids [hubs]."""
    width = 4 * (d // 4)
    slots, csr = _gd_contest_lists(rng, hubs, rivals)
    base = np.empty((slots.size, d), np.int64)
    for s in slots:
        q = (96 + _ints(rng, (d,), 0, 13)) << 17
        v = (1 << 19) + _ints(rng, (d,), 0, 1 << 19)
        base[s[0]] = q
        base[s[1]] = q + v
        for t in range(rivals):
            pv = v - _ints(rng, (d,), -(1 << 19) + 1, 1 << 19)      # (the tail; overwritten where Dist reads)
            pv[:width] = v[:width][rng.permutation(width)]
            base[s[2 + t]] = q + v - pv
    assert base.min() >= (1 << 23) and base.max() < (1 << 24)
    return (base.astype(np.float32) / np.float32(1 << 23)).astype(np.float32), csr, np.ascontiguousarray(slots[:, 0])


def gd_contest_dot(rng, hubs, d, rivals=4):
    """The same contest under Angular::Dist (d % 8 == 0).  Hub = [x | -y] with x in [2^22, 2^23)^(d/2), y in [1, 2^21)^(d/2)
    over 2^23; g_t = [-sigma_t(y) | tau_t(x)] with fresh permutations; c = -(11184811 / 2^23) (1, ..., 1).  In real
    arithmetic Dist(c, hub) = Dist(c, g_t) = 1.333 (sum x - sum y) > 0, every float32 product rounds.  Dist(hub, g_t) is
    positive and smaller than Dist(hub, c); Dist(g_s, g_t) is negative, so at the hub only the nearest rival survives the
    pruning (the others are linked by the M / 2 rule) and c faces that one opponent, and in a rival's own list the other
    rivals fall to the `Dist > eps` filter.  Returns as gd_contest_l2."""
    assert d % 8 == 0
    half = d // 2
    slots, csr = _gd_contest_lists(rng, hubs, rivals)
    base = np.empty((slots.size, d), np.int64)
    for s in slots:
        x = _ints(rng, (half,), 1 << 22, 1 << 23)
        y = _ints(rng, (half,), 1, 1 << 21)
        base[s[0]] = np.concatenate([x, -y])
        base[s[1]] = -11184811
        for t in range(rivals):
            base[s[2 + t]] = np.concatenate([-y[rng.permutation(half)], x[rng.permutation(half)]])
    assert np.abs(base).max() < (1 << 24)
    return (base.astype(np.float32) / np.float32(1 << 23)).astype(np.float32), csr, np.ascontiguousarray(slots[:, 0])


def knn_bruteforce(x, k, block=512):
    """Exact-enough kNN lists (float64 distances, ties by id); excludes self.  Generator-side
    helper only: its output is an *input* (and is committed where bit-portability matters)."""
    x64 = x.astype(np.float64)
    n = x.shape[0]
    sq = (x64 * x64).sum(1)
    out = np.empty((n, k), np.uint32)
    for s in range(0, n, block):
        e = min(n, s + block)
        dmat = sq[s:e, None] + sq[None, :] - 2.0 * (x64[s:e] @ x64.T)
        dmat[np.arange(e - s), np.arange(s, e)] = np.inf
        idx = np.argsort(dmat, axis=1, kind="stable")[:, :k]
        out[s:e] = idx.astype(np.uint32)
    return out


def lists_to_csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    nbr = np.concatenate([np.asarray(l, np.uint32) for l in lists]) if len(lists) else \
        np.zeros(0, np.uint32)
    return off, np.ascontiguousarray(nbr, np.uint32)


def dense_to_csr(knn):
    n, k = knn.shape
    off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(k)).astype(np.uint64)
    return off, np.ascontiguousarray(knn.reshape(-1), np.uint32)


def random_graph(rng, n, deg_lo, deg_hi):
    """Ragged random adjacency (no self loops, no duplicate neighbours inside a list)."""
    lists = []
    for i in range(n):
        k = int(_ints(rng, (), deg_lo, deg_hi + 1))
        c = np.unique(_ints(rng, (k * 2 + 2,), 0, n))
        c = c[c != i]
        rng.shuffle(c)
        lists.append(c[:k].astype(np.uint32))
    return lists_to_csr(lists)


def contest_graph(rng, groups, per_group, deg_lo, deg_hi):
    """A random_graph per contest group, offset to the group's rows: the groups are disconnected components, so a
    walk entered inside a group returns candidates of that group only."""
    lists = []
    for g in range(groups):
        off, nbr = random_graph(rng, per_group, deg_lo, deg_hi)
        lists += [nbr[int(off[i]):int(off[i + 1])] + np.uint32(g * per_group) for i in range(per_group)]
    return lists_to_csr(lists)


KAT_DIMS =list(range(0, 41)) + [45, 96, 128, 200, 257, 960]


def kat_pairs():
    """Vector pairs for the scalar distance known-answer tests (4 per dimension in KAT_DIMS)."""
    rng = np.random.Generator(np.random.PCG64(4242))
    pairs = []
    for d in KAT_DIMS:
        for _ in range(4):
            a = rng.integers(-2**20, 2**20, size=d).astype(np.float32) / np.float32(2**18)
            b = rng.integers(-2**20, 2**20, size=d).astype(np.float32) / np.float32(2**18)
            pairs.append((a.astype(np.float32), b.astype(np.float32)))
    return pairs


class Case:
    """One seeded configuration: base, queries, net (all bit-portable)."""

    def __init__(self, name, seed, n, nq, d, dlow, dh, kind="clustered", metric=0):
        self.name, self.seed, self.n, self.nq = name, seed, n, nq
        self.d, self.dlow, self.dh, self.kind, self.metric = d, dlow, dh, kind, metric
        rng = np.random.Generator(np.random.PCG64(seed))
        if kind == "lattice":
            self.base = lattice(rng, n, d)
            self.queries = lattice(rng, nq, d, dup=1)
        else:
            self.base = clustered(rng, n, d)
            self.queries = clustered(rng, nq, d)
        self.net = net_layers(rng, d, dh, dlow)
        self.rng = rng

    def input_hash(self):
        h = hashlib.sha256()
        for a in (self.base, self.queries) + tuple(self.net):
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()


# Golden configurations (tests/golden/make_golden.py); shapes follow BASELINE.json's configs at
# toy size: SIFT 128->32 w256, GIST 960->64, GloVe 200->32 (neg-dot metric), DEEP 96->32, a tail
# case with d % 8 != 0, d % 4 != 0, d_low % 4 != 0, and a tie-heavy lattice case.
GOLDEN_CASES = [
    dict(name="sift_toy", seed=101, n=4096, nq=256, d=128, dlow=32, dh=256, efs=[1, 8, 64]),
    dict(name="gist_toy", seed=102, n=2048, nq=64, d=960, dlow=64, dh=128, efs=[8, 200]),
    dict(name="glove_toy", seed=103, n=2048, nq=128, d=200, dlow=32, dh=64, efs=[8, 64],
         metric=1),
    dict(name="deep_toy", seed=104, n=2048, nq=128, d=96, dlow=32, dh=64, efs=[1, 40]),
    dict(name="tail_toy", seed=105, n=1024, nq=64, d=45, dlow=14, dh=27, efs=[1, 8, 33]),
    dict(name="ties_toy", seed=106, n=3072, nq=128, d=16, dlow=8, dh=16, efs=[1, 2, 8, 64],
         kind="lattice"),
]
