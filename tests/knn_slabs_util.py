"""Shared by tests/test_knn_slabs_cpu.py and tests/test_gpu_knn_slabs.py: the fixtures that make an error of the query-slab loop of
gbnns_exact_knn_bytes / gbnns_exact_knn's pool path visible at "knn_slab" = 128 and 300 queries (slabs of 128, 128 and 44), and the
preconditions they rest on, each asserted from the CPU oracle's output.

A case has three groups of queries -- 128 near the base set, 128 in the middle of it, 44 far from it -- handed out in a shuffled order;
`ordered` sorts them by the oracle's k-th distance, so that the query at position i of a slab has a strictly larger k-th distance than the
query at position i of the slab before -- a heap, pool or root left over from that query holds smaller keys -- and a strictly smaller
threshold in the form the sweep kernels keep it (threshold_terms): a threshold left over from that query is too tight.
The tag words of the three groups come from three disjoint sets of words with different allowed rows, drawn at random inside a group (no
period): tag words read at the previous slab's offset allow other rows.  Nothing here has a tolerance."""
import numpy as np

import knn_bytes_util as ku
import knn_tagged_util as tu

NQ, SLAB, N, K_MAX = 300, 128, 6000, 200
GROUPS = (128, 128, 44)
GROUP_WORDS = ((0x02, 0x40, 0x42), (0x04, 0x80, 0x0C), (0x01, 0x10, 0x20))   # near / middle / far queries; bits of tag_table below


def tag_table(seed, n):
    """T [n] uint32: bit 0 on every row, bits 1 .. 5 on half the rows each, bits 6 and 7 on a quarter each, all independent."""
    rng = np.random.default_rng(seed)
    t = np.ones(n, np.uint32)
    for b in range(1, 8):
        t |= (rng.random(n) < (0.5 if b < 6 else 0.25)).astype(np.uint32) << np.uint32(b)
    return t


def _queries(rng, metric, d, centre):
    near_n, mid_n, far_n = GROUPS
    mid = rng.integers(128, 256, (mid_n, d))
    if metric == ku.L2:   # near: inside the cluster of base rows; far: below the half cube the rows fill, towards the middle of the byte range
        near = centre + rng.integers(-8, 9, (near_n, d))
        far = rng.integers(96, 128, (far_n, d))
    else:                 # the negative dot: large coordinates are "near" (a very negative -x.q), small ones "far"
        near = rng.integers(200, 256, (near_n, d))
        far = rng.integers(0, 31, (far_n, d))
    return np.concatenate([near, mid, far])


def byte_case(metric, d, seed, n=N):
    """base [n x d] uint8 -- uniform over 128 .. 255, two fifths of the rows (scattered over the set) in a cluster of +-8 around a point near
    the all-255 corner -- queries [300 x d] uint8 in a shuffled order, row tags, query tag words, and the group (0 near, 1 middle, 2 far)
    of every query.  The geometry serves BOTH orders `ordered` asserts: near queries have the smallest k-th distance and the largest
    threshold as the sweep kernels keep it, far queries the largest k-th distance and the smallest threshold."""
    rng = np.random.default_rng(seed)
    base = rng.integers(128, 256, (n, d))
    centre = rng.integers(225, 246, d)
    rows = rng.permutation(n)[:2 * n // 5]
    base[rows] = centre + rng.integers(-8, 9, (rows.size, d))
    q = _queries(rng, metric, d, centre)
    group = np.repeat(np.arange(3), GROUPS)
    Q = np.concatenate([rng.choice(np.array(GROUP_WORDS[j], np.uint32), GROUPS[j]) for j in range(3)]).astype(np.uint32)
    perm = rng.permutation(NQ)
    return base.astype(np.uint8), np.ascontiguousarray(q[perm].astype(np.uint8)), tag_table(seed + 1, n), np.ascontiguousarray(Q[perm]), group[perm]


def float_case(d, seed, n=N):
    """byte_case(L2) in float32 with a jitter of one byte step and an inexact scale: every product and partial sum rounds."""
    base, q, T, Q, group = byte_case(ku.L2, d, seed, n)
    rng = np.random.default_rng(seed + 2)
    fb = (ku.widen(base) + rng.random(base.shape, dtype=np.float32)) * np.float32(0.0123)
    fq = (ku.widen(q) + rng.random(q.shape, dtype=np.float32)) * np.float32(0.0123)
    return fb, np.ascontiguousarray(fq), T, Q, group


def threshold_terms(q, metric):
    """The query's part of a threshold as the sweep kernels keep it, so that a pair is kept where (the rows' part) >= term - (k-th distance):
    uint8 queries (knn_bytes.hip, operands x - 128): sum (q - 128)^2 over the first 4 floor(d / 4) dimensions, or -128 sum (q - 128) -
    16 384 d for the negative dot; float queries (knn.hip): |q|^2, but for a slack of a few float32 steps and a common factor 1/2."""
    if q.dtype != np.uint8:
        return (q.astype(np.float64) ** 2).sum(1)
    s = q.astype(np.int64) - 128
    if metric == ku.L2:
        return (s[:, :q.shape[1] // 4 * 4] ** 2).sum(1).astype(np.float64)
    return (-128 * s.sum(1) - 16384 * q.shape[1]).astype(np.float64)


def references(orc, base, q, T, Q, metric, k_max=K_MAX):
    """The oracle's k_max-lists of the shuffled queries: untagged, and over the allowed rows (knn_tagged_util.expected)."""
    return orc.exact_knn(ku.widen(base), ku.widen(q), k_max, metric, threads=8), tu.expected(orc, base, q, T, Q, k_max, metric)


def ordered(q, Q, ref, k, rank=None, metric=None):
    """Queries, tag words and the oracle's k-lists in ascending order of the oracle's k-th distance (`rank`: of that rank instead, 1-based).
    Asserts that the k-th distance at position i exceeds the one at position i - 128 STRICTLY for every i >= 128 -- a heap, pool or root
    left from the slab before holds smaller keys -- and, where `metric` is given, that the final threshold threshold_terms - (k-th distance)
    at position i is STRICTLY below the one at position i - 128 -- a threshold left from the slab before is too tight, not too loose."""
    ids, dist = ref
    kth = dist[:, (rank or k) - 1]
    assert np.isfinite(kth).all()
    order = np.argsort(kth, kind="stable")
    kth = kth[order]
    assert (kth[SLAB:] > kth[:-SLAB]).all(), "a tie at stride 128: another seed, not a weaker assertion"
    q = np.ascontiguousarray(q[order])
    if metric is not None:
        thr = threshold_terms(q, metric) - kth.astype(np.float64)
        margin = 1e-3 * np.abs(thr).max() if q.dtype != np.uint8 else 0   # (float: far more than the filter's slack)
        assert (thr[SLAB:] + margin < thr[:-SLAB]).all()
    return q, np.ascontiguousarray(Q[order]), (np.ascontiguousarray(ids[order, :k]), np.ascontiguousarray(dist[order, :k]))


def check_tag_offsets(T, Q):
    """For every i >= 128 the word of query i differs from the word of query i - 128, and so do the rows the two allow."""
    a, b = Q[SLAB:], Q[:-SLAB]
    assert (a != b).all()
    for w1, w2 in set(zip(a.tolist(), b.tolist())):
        assert (((T & np.uint32(w1)) != 0) != ((T & np.uint32(w2)) != 0)).any(), (w1, w2)
    for p in (32, 128):   # no period of 32 or 128
        assert (Q[p:] != Q[:-p]).any()


def overflow_case(k, nq=NQ, n=12000, d=32):
    """test_gpu_knn_bytes.test_overflowing_chunks_are_swept_again's construction with 300 queries: rows sorted farthest first from the
    centre, the queries the centre plus 0 .. 3 on four coordinates (query 0 the centre itself), and knn_tagged_util's tag table with bit 1
    -- half the rows -- as every query's filter."""
    rng = np.random.default_rng(k)
    base = rng.integers(0, 256, (n, d), dtype=np.uint8)
    dist = ((base.astype(np.int64) - 128) ** 2).sum(1)
    base = np.ascontiguousarray(base[np.lexsort((np.arange(n), -dist))])
    q = np.full((nq, d), 128, np.uint8)
    q[1:, :4] += rng.integers(0, 4, (nq - 1, 4)).astype(np.uint8)
    return base, q, tu.tag_table(600 + k, n), np.full(nq, 1 << 1, np.uint32)


FLOAT_OVERFLOW_N = {False: 12000, True: 20000}   # rows of overflow_case for gbnns_exact_knn's pool path: untagged / tagged (half the rows allowed)


def float_pool_plan(n, k, knn_chunk):
    """The chunks of gbnns_exact_knn's pool path (graph_api.cpp) in the form of a knn_bytes_plan dict, for knn_bytes_util.chunk_plan: the
    byte call's first chunk and key slots, later chunks of at most 4 knn_chunk rows AND at most a sixteenth of the set (in whole 64s)."""
    cap = 4 * k + 64
    return dict(cap=cap, first_rows=min(n, cap & ~63), max_chunk=min(4 * knn_chunk, max(64, (n // 16 + 63) & ~63)))


def kept_rows(plan, base, q, allowed, k):
    """[queries x chunks of knn_bytes_util.chunk_plan(plan, n)] how many rows of a chunk a query's key list has to take: the allowed rows
    no farther than the k-th nearest allowed row before the chunk (every allowed row while there are fewer than k).  From the integer
    distances of byte rows; a lower bound of what a sweep keeps, whose threshold is never tighter than that."""
    dist = ku.int_dist(base, q, ku.L2).astype(np.float64)
    dist[:, ~allowed] = np.inf
    out = []
    for r0, rows in ku.chunk_plan(plan, base.shape[0]):
        kth = np.partition(dist[:, :r0], k - 1, axis=1)[:, k - 1] if r0 >= k else np.full(q.shape[0], np.inf)
        part = dist[:, r0:r0 + rows]
        out.append((np.isfinite(part) & (part <= kth[:, None])).sum(1))
    return np.stack(out, axis=1)
