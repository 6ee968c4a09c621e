"""knn_wide.hip on an MI355X (run with -m gpu): gbnns_exact_knn / gbnns_exact_knn_tagged on float rows wider than 128 dims with
"knn_filter_wide" = 2 -- the K-looped matrix-core filter in front of the heaps -- against the CPU oracle (orc.exact_knn,
knn_tagged_util.expected) and against the same call with the knob at 0 (the exact scan), ids and distance bit patterns of every query;
gbnns_debug_knn_plan, asked right before the call, names the wide kernel.  No tolerance.

Shapes: "knn_chunk" = 64, n = 1 037, n_q = 128 + 37 -- sixteen chunks of 64 rows (each a partial block of 128 rows), a last one of 13, a
second workgroup of queries with 37 of its 128; d = 132 (dp = 144: nine K steps, the last stage half zeros, the last K step 12 zero
columns), 300 (d % 16 = 12), 960, 1024 (the longest row of the bound).

test_overflowing_chunks_are_scanned: 16 421 rows of full-mantissa uniform floats from [2, 3) at d = 960: 1 024 first rows, a chunk of
1 024, then chunks of 1 088.  The slack c (|q|^2 + |x|^2) is about 11.9 there, two standard deviations (6.1) of the distances: under the
thresholds the first 1 024 rows leave, 41 % of the second chunk's pairs pass (float64, this data; every query at least 279 rows against
256 slots), so that chunk overflows its lists and is scanned exactly inside the call; under the final thresholds 14 % pass (at most
223 rows a query and chunk), so later chunks are rescored."""
import numpy as np
import pytest

import knn_bytes_util as ku
import knn_instances as ki
import knn_tagged_util as kt

pytestmark = pytest.mark.gpu

L2 = 0
N, NQ, CHUNK = ki.N, 128 + 37, ki.CHUNK


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def _both(g, base, q, k, tagged, **kw):
    """(wide filter's answer, scan's answer) of one call, the plan checked under the knob."""
    lib = g.load_library()
    scan = g.exact_knn(base, q, k, L2, want_dist=True, **kw)
    try:
        assert lib.gbnns_debug_knob(b"knn_filter_wide", 2) == 0
        name = "knn_wide_filter_kernel<2, %s>" % ("true" if tagged else "false")
        assert g.knn_plan(False, L2, base.shape[0], q.shape[0], base.shape[1], k, tagged) == (name, False)
        wide = g.exact_knn(base, q, k, L2, want_dist=True, **kw)
    finally:
        lib.gbnns_debug_knob(b"knn_filter_wide", 0)
    return wide, scan


@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "tagged"])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", [132, 300, 960, 1024])
def test_equals_the_oracle_and_the_scan(g, orc, d, k, tagged):
    base, q = ki.data(False, d, NQ)
    kw = {}
    if tagged:   # (words that allow every row, none, a share, the last 40 rows only, and rows 0 .. 6 only: fewer than k = 10)
        T, Q = kt.tag_table(7900, N), kt.query_words(NQ)
        kw = dict(row_tags=T, query_tags=Q)
        want = kt.expected(orc, base, q, T, Q, k, L2)
    else:
        want = orc.exact_knn(base, q, k, L2, threads=8)
    with ku.knobs(g, knn_chunk=CHUNK):
        wide, scan = _both(g, base, q, k, tagged, **kw)
    kt.same(wide, want, "wide filter against the oracle")
    kt.same(wide, scan, "wide filter against the scan")


def test_self_lists(g, orc):
    base, _ = ki.data(False, 300, NQ)
    q = np.ascontiguousarray(base[:NQ])
    T, Q = kt.tag_table(7900, N), kt.query_words(NQ)
    want = kt.expected(orc, base, q, T, Q, 10, L2, self_offset=0)
    with ku.knobs(g, knn_chunk=CHUNK):
        wide, scan = _both(g, base, q, 10, True, self_offset=0, row_tags=T, query_tags=Q)
    kt.same(wide, want, "self lists against the oracle")
    kt.same(wide, scan, "self lists against the scan")


def test_overflowing_chunks_are_scanned(g, orc):
    n, d, k, chunk, cap = 16 * 1024 + 37, 960, 10, 1024, 256
    rng = np.random.default_rng(9600)
    base = rng.random((n, d), dtype=np.float32) + np.float32(2)
    q = rng.random((NQ, d), dtype=np.float32) + np.float32(2)
    # the second chunk overflows: under the first chunk's exact thresholds more rows than a list holds lie within 0.9 of the slack
    b, qq = base[:2 * chunk].astype(np.float64), q.astype(np.float64)
    S = (qq * qq).sum(1)[:, None] + (b * b).sum(1)[None, :]
    D = S - 2 * qq @ b.T
    T1 = np.sort(D[:, :chunk], 1)[:, k - 1]
    assert ((D[:, chunk:] <= T1[:, None] + 0.9 * S[:, chunk:] / 1024).sum(1) > cap).any()
    want = orc.exact_knn(base, q, k, L2, threads=8)
    wide, scan = _both(g, base, q, k, False)   # ("knn_chunk" at its default: chunks of up to a sixteenth of the set, 1 088 rows)
    kt.same(wide, want, "overflowing chunks against the oracle")
    kt.same(wide, scan, "overflowing chunks against the scan")
