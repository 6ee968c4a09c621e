"""knn_dot.hip on an MI355X (run with -m gpu): gbnns_exact_knn / gbnns_exact_knn_tagged under the negative dot with "knn_filter_dot" = 2 --
the K-looped matrix-core filter in front of the heaps -- against the CPU oracle (orc.exact_knn, knn_tagged_util.expected) and against the
same call with the knob at 0 (the exact scan), ids and distance bit patterns of every query; gbnns_debug_knn_plan, asked right before the
call, names the dot kernel.  No tolerance.

Shapes: "knn_chunk" = 64, n = 1 037, n_q = 128 + 37 -- sixteen chunks of 64 rows (each a partial block of 128 rows), a last one of 13, a
second workgroup of queries with 37 of its 128; d = 8 (dp = 16: one K step, half zeros, the stage's second K step all zeros), 72 (dp = 80:
five K steps, the last stage half zero), 200, 1024 (the longest row of the bound).

test_overflowing_chunks_are_scanned: 16 421 rows of full-mantissa uniform floats from [20, 21) at d = 960: 1 024 first rows, a chunk of
1 024, then chunks of 1 088.  All dots lie within a few parts in 10^4 of |q||x|, the scale of the slack: under the thresholds the first
1 024 rows leave, every query keeps more of the second chunk than its 256 slots (float64, this data: 316 to 332), so that chunk overflows
and is scanned exactly inside the call; under the final thresholds no query keeps 256 rows of a later chunk (at most 208), so those are
rescored.

test_cancellation: rows of +-2^20 at d = 96 -- |q||x| = 96 * 2^40 while most dots are small even multiples of 2^40, all exact: mass ties at
every threshold, which only the slack term lets through to the rescore."""
import numpy as np
import pytest

import knn_bytes_util as ku
import knn_instances as ki
import knn_tagged_util as kt

pytestmark = pytest.mark.gpu

NEG_DOT = 1
N, NQ, CHUNK = ki.N, 128 + 37, ki.CHUNK


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _both(g, base, q, k, tagged, **kw):
    """(dot filter's answer, scan's answer) of one call, the plan checked under the knob."""
    lib = g.load_library()
    scan = g.exact_knn(base, q, k, NEG_DOT, want_dist=True, **kw)
    try:
        assert lib.gbnns_debug_knob(b"knn_filter_dot", 2) == 0
        name = "knn_dot_filter_kernel<2, %s>" % ("true" if tagged else "false")
        assert g.knn_plan(False, NEG_DOT, base.shape[0], q.shape[0], base.shape[1], k, tagged) == (name, False)
        dot = g.exact_knn(base, q, k, NEG_DOT, want_dist=True, **kw)
    finally:
        lib.gbnns_debug_knob(b"knn_filter_dot", 0)
    return dot, scan


@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "tagged"])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", [8, 72, 200, 1024])
def test_equals_the_oracle_and_the_scan(g, orc, d, k, tagged):
    base, q = ki.data(False, d, NQ)
    kw = {}
    if tagged:   # (words that allow every row, none, a share, the last 40 rows only, and rows 0 .. 6 only: fewer than k = 10)
        T, Q = kt.tag_table(7900, N), kt.query_words(NQ)
        kw = dict(row_tags=T, query_tags=Q)
        want = kt.expected(orc, base, q, T, Q, k, NEG_DOT)
    else:
        want = orc.exact_knn(base, q, k, NEG_DOT, threads=8)
    with ku.knobs(g, knn_chunk=CHUNK):
        dot, scan = _both(g, base, q, k, tagged, **kw)
    kt.same(dot, want, "dot filter against the oracle")
    kt.same(dot, scan, "dot filter against the scan")


def test_self_lists(g, orc):
    base, _ = ki.data(False, 200, NQ)
    q = np.ascontiguousarray(base[:NQ])
    T, Q = kt.tag_table(7900, N), kt.query_words(NQ)
    want = kt.expected(orc, base, q, T, Q, 10, NEG_DOT, self_offset=0)
    with ku.knobs(g, knn_chunk=CHUNK):
        dot, scan = _both(g, base, q, 10, True, self_offset=0, row_tags=T, query_tags=Q)
    kt.same(dot, want, "self lists against the oracle")
    kt.same(dot, scan, "self lists against the scan")


def test_overflowing_chunks_are_scanned(g, orc):
    n, d, k, chunk, later, cap = 16 * 1024 + 37, 960, 10, 1024, 1088, 256
    rng = np.random.default_rng(9601)
    base = rng.random((n, d), dtype=np.float32) + np.float32(20)
    q = rng.random((NQ, d), dtype=np.float32) + np.float32(20)
    b, qq = base.astype(np.float64), q.astype(np.float64)
    D = qq @ b.T
    P = np.sqrt((qq * qq).sum(1))[:, None] * np.sqrt((b * b).sum(1))[None, :]
    # the second chunk overflows: over the first chunk's exact thresholds more rows than a list holds lie within 0.9 of the slack
    T1 = np.sort(D[:, :chunk], 1)[:, -k]
    second = slice(chunk, 2 * chunk)
    assert ((D[:, second] + 0.9 * P[:, second] / 1024 >= T1[:, None]).sum(1) > cap).any()
    # later chunks are rescored: over the final thresholds no query has a list's worth of any of them within 1.1 of the slack
    Tn = np.sort(D, 1)[:, -k]
    kept = D + 1.1 * P / 1024 >= Tn[:, None]
    assert max(kept[:, r0:r0 + later].sum(1).max() for r0 in range(2 * chunk, n, later)) < cap
    want = orc.exact_knn(base, q, k, NEG_DOT, threads=8)
    dot, scan = _both(g, base, q, k, False)   # ("knn_chunk" at its default: chunks of up to a sixteenth of the set, 1 088 rows)
    kt.same(dot, want, "overflowing chunks against the oracle")
    kt.same(dot, scan, "overflowing chunks against the scan")


def test_cancellation(g, orc):
    d, k = 96, 10
    signs = np.random.default_rng(96).integers(0, 2, (N, d)).astype(np.float32) * 2 - 1
    base = np.ascontiguousarray(signs * np.float32(2.0 ** 20))
    q = np.ascontiguousarray(base[7:7 + NQ])   # some rows' own patterns; not self lists: the row itself is the best answer
    want = orc.exact_knn(base, q, k, NEG_DOT, threads=8)
    assert (want[1][:, k - 1] == want[1][:, k - 2]).mean() > 0.5   # ties at the threshold are the rule
    with ku.knobs(g, knn_chunk=CHUNK):
        dot, scan = _both(g, base, q, k, False)
    kt.same(dot, want, "cancellation against the oracle")
    kt.same(dot, scan, "cancellation against the scan")
