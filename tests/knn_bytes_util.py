"""Shared by tests/test_knn_bytes_cpu.py and tests/test_gpu_knn_bytes.py: byte fixtures for gbnns_exact_knn_bytes, the plain
integer yardstick, the ordered float32 emulation of the reference's distances, and the knob handling."""
import contextlib

import numpy as np

L2, NEG_DOT = 0, 1
ROW_BLOCK = 32   # base rows of one matrix product of the sweep
K_STEP = 32      # K of v_mfma_i32_32x32x32_i8
NONE_ID = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def widen(a):
    return np.ascontiguousarray(a, np.float32)


def random_bytes(seed, n, d):
    """Uniform bytes over 0 .. 255 (values >= 128 everywhere: the signed view of the int8 instruction matters), row 0 all 0 and
    row 1 all 255 (their distance is the largest a row pair of that d can have: 65 025 d, 2^24 - 130 816 at d = 256)."""
    x = np.random.default_rng(seed).integers(0, 256, (n, d), dtype=np.uint8)
    x[0] = 0
    if n > 1:
        x[1] = 255
    return x


def int_dist(base, queries, metric):
    """[nq x n] int64 distances: sum (x - q)^2 over the first 4 floor(d / 4) dimensions, or -sum x q."""
    b, q = base.astype(np.int64), queries.astype(np.int64)
    if metric == L2:
        u = base.shape[1] // 4 * 4
        b, q = b[:, :u], q[:, :u]
        return (q * q).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (q @ b.T)
    return -(q @ b.T)


def int_knn(base, queries, k, metric, self_offset=-1):
    """The k smallest (distance, id) pairs per query with plain int64 numpy and np.lexsort((id, dist)); (ids uint32, dist float32),
    0xFFFFFFFF / +inf where fewer than k rows qualify."""
    dist = int_dist(base, queries, metric)
    n, nq = base.shape[0], queries.shape[0]
    ids = np.full((nq, k), NONE_ID, np.uint32)
    out = np.full((nq, k), np.inf, np.float32)
    rows = np.arange(n)
    for i in range(nq):
        order = np.lexsort((rows, dist[i]))
        if self_offset >= 0:
            order = order[order != i + self_offset]
        order = order[:k]
        ids[i, :order.size] = order
        out[i, :order.size] = dist[i, order].astype(np.float32) + np.float32(0.0)   # (-0 of a zero dot product reads +0, as in the float call)
    return ids, out


def f32_l2_four_sums(x, q):
    """L2Metric::Dist on float32(x), float32(q) with every operation rounded to float32 in the reference's order: four running sums over
    the first 4 floor(d / 4) dimensions, folded ((s0 + s1) + s2) + s3."""
    x, q = np.asarray(x, np.float32), np.asarray(q, np.float32)
    s = [np.float32(0)] * 4
    for c in range(0, x.size // 4 * 4, 4):
        for j in range(4):
            e = np.float32(x[c + j] - q[c + j])
            s[j] = np.float32(s[j] + np.float32(e * e))
    return np.float32(np.float32(np.float32(s[0] + s[1]) + s[2]) + s[3])


def f32_dot_eight_sums(x, q):
    """Angular::Dist the same way: eight running sums (dimension mod 8), the high half folded onto the low half, then pairs."""
    x, q = np.asarray(x, np.float32), np.asarray(q, np.float32)
    s = [np.float32(0)] * 8
    for c in range(0, x.size, 8):
        for j in range(8):
            s[j] = np.float32(s[j] + np.float32(x[c + j] * q[c + j]))
    m = [np.float32(s[j + 4] + s[j]) for j in range(4)]
    return np.float32(-np.float32(np.float32(m[0] + m[1]) + np.float32(m[2] + m[3])))


@contextlib.contextmanager
def knobs(g, knn_chunk=None, knn_pool_min_k=None, knn_slab=None, knn_filter=None):
    """gbnns_exact_knn*'s process-wide knobs for the duration of a with-block; the defaults (32 768 rows, pools from k = 64, slabs by the
    4 GiB rule: "knn_slab" 0; "knn_filter" 1 where the block set it) come back, also behind an exception."""
    lib = g.load_library()
    try:
        if knn_chunk is not None:
            assert lib.gbnns_debug_knob(b"knn_chunk", knn_chunk) == 0
        if knn_pool_min_k is not None:
            assert lib.gbnns_debug_knob(b"knn_pool_min_k", knn_pool_min_k) == 0
        if knn_slab is not None:
            assert lib.gbnns_debug_knob(b"knn_slab", knn_slab) == 0
        if knn_filter is not None:
            assert lib.gbnns_debug_knob(b"knn_filter", knn_filter) == 0
        yield
    finally:
        lib.gbnns_debug_knob(b"knn_chunk", 1 << 15)
        lib.gbnns_debug_knob(b"knn_pool_min_k", 64)
        lib.gbnns_debug_knob(b"knn_slab", 0)
        if knn_filter is not None:
            lib.gbnns_debug_knob(b"knn_filter", 1)


def slabs(slab, nq):
    """The query slabs [(first query, queries)] of a call with nq queries, from knn_bytes_plan(...)["slab"] or knn_slab(...)."""
    return [(q0, min(slab, nq - q0)) for q0 in range(0, nq, slab)]


def chunk_plan(plan, n):
    """The chunks [(first row, rows)] gbnns_exact_knn_bytes sweeps a set of n rows in, from a knn_bytes_plan dict."""
    out, r0 = [], 0
    while r0 < n:
        chunk = plan["first_rows"] if r0 == 0 else min(plan["max_chunk"], r0)
        rows = min(chunk, n - r0)
        out.append((r0, rows))
        r0 += rows
    return out
