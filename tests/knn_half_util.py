"""Shared by the tests of gbnns_exact_knn_half (tests/test_gpu_knn_half.py, tests/knn_half_instances.py and its two tests,
tests/test_gpu_knn_half_edges.py): the plain reference -- the reference's ordered float32 sums (knn_bytes_util.f32_l2_four_sums /
f32_dot_eight_sums, restated over whole arrays: the same operations in the same order, checked against those functions pair by pair on a
sample) on the widened rows, then numpy's sort of (distance, id) -- and the comparison, ids and distance bit patterns.  Not another call
of the library, and no tolerance."""
import numpy as np

import knn_bytes_util as ku

F32 = np.float32
# the magnitude classes of the half-row tests: rows (and queries) x 2^e -- at -20 most halves are subnormal, at 13 the largest near 65 504
SCALE = {"unit": 0, "subnormal": -20, "large": 13}


def half_rows(rng, n, d, cls="unit"):
    """[n x d] float16: standard_normal x 2^SCALE[cls] rounded to binary16, every eighth row a duplicate of the row before it (ties)."""
    rows = (rng.standard_normal((n, d)).astype(F32) * F32(2.0 ** SCALE[cls])).astype(np.float16)
    rows[7::8] = rows[6::8][:len(rows[7::8])]
    return rows


def ordered_dist(rows, q, metric):
    """[nq x n] float32: L2Metric::Dist / Angular::Dist of the reference on float32(rows), every operation rounded to float32 in its order."""
    x, d = rows.astype(F32), rows.shape[1]
    if metric == ku.L2:
        s = [np.zeros((len(q), len(x)), F32) for _ in range(4)]
        for c in range(d // 4 * 4):
            e = x[None, :, c] - q[:, None, c]
            s[c % 4] = s[c % 4] + e * e
        out = ((s[0] + s[1]) + s[2]) + s[3]
        one = ku.f32_l2_four_sums
    else:
        s = [np.zeros((len(q), len(x)), F32) for _ in range(8)]
        for c in range(d):
            s[c % 8] = s[c % 8] + x[None, :, c] * q[:, None, c]
        m = [s[j + 4] + s[j] for j in range(4)]
        out = -((m[0] + m[1]) + (m[2] + m[3]))
        one = ku.f32_dot_eight_sums
    assert out.dtype == F32
    for i, j in ((0, 10), (5, 7), (len(q) - 1, len(x) - 1)):
        i, j = min(i, len(q) - 1), min(j, len(x) - 1)
        assert ku.bits(out[i, j]) == ku.bits(one(x[j], q[i]))
    return out + F32(0)   # (-0 reads +0, as in the float call)


def knn_of(dist, k, allowed=None, self_offset=-1):
    nq, n = dist.shape
    ids, out = np.full((nq, k), ku.NONE_ID, np.uint32), np.full((nq, k), np.inf, F32)
    rows = np.arange(n)
    for i in range(nq):
        order = np.lexsort((rows, dist[i]))
        if allowed is not None:
            order = order[allowed[i][order]]
        if self_offset >= 0:
            order = order[order != i + self_offset]
        order = order[:k]
        ids[i, :order.size], out[i, :order.size] = order, dist[i, order]
    return ids, out


def host(got):
    """A call's (ids, dist) as numpy arrays (torch tensors come back from device inputs)."""
    gi, gd = (np.asarray(a.cpu()) if hasattr(a, "cpu") else np.asarray(a) for a in got)
    return gi.view(np.uint32), gd


def same(got, want, what="", queries=None):
    """Every query's ids and distance bits; queries: the rows of `got` that `want` holds (a sample), default all."""
    (gi, gd), (wi, wd) = host(got), host(want)
    if queries is not None:
        gi, gd = gi[queries], gd[queries]
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.flatnonzero((gi != wi).any(1) | (ku.bits(gd) != ku.bits(wd)).any(1))
    print(what, "queries that differ:", bad.size, bad[:8])
    assert bad.size == 0, (what, bad[:8], gi[bad[0]][:8], wi[bad[0]][:8], gd[bad[0]][:8], wd[bad[0]][:8])
