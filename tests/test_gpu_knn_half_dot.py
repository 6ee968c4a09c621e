"""knn_half_dot.hip on an MI355X (run with -m gpu): gbnns_exact_knn_half / gbnns_index_exact_knn_half under the negative dot with
"knn_half_dot" = 2 against the plain reference of tests/knn_half_util.py (Angular::Dist's ordered float32 sums on the widened rows, numpy's
sort of (distance, id)) and against the same call with the knob at 0 (the exact scan), ids and distance bit patterns; the plan is asked
right before the call.  No tolerance.  Shapes: "knn_chunk" = 64, n = 1 037, n_q = 128 + 37 -- sixteen chunks of 64 rows (each a partial
block of 128 rows), a last one of 13, a second workgroup of queries with 37 of its 128; d = 8 (dp = 16: one K step, half zeros), 72
(dp = 80: five K steps, the last stage half empty), 200, 1024 (the longest row of the bound).  test_overflowing_chunks_are_scanned and
test_cancellation mirror tests/test_gpu_knn_dot.py's on binary16 rows."""
import functools

import numpy as np
import pytest

import knn_bytes_util as ku
import knn_half_util as kh
import knn_instances as ki
import knn_tagged_util as kt

pytestmark = pytest.mark.gpu

NEG_DOT, F32, N, NQ, CHUNK = 1, np.float32, ki.N, 128 + 37, ki.CHUNK


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@functools.lru_cache(maxsize=None)
def data(d, cls="unit"):
    rng = np.random.default_rng(9900 + d + kh.SCALE[cls])
    rows = kh.half_rows(rng, N, d, cls)
    q = rng.standard_normal((NQ, d)).astype(F32) * F32(2.0 ** kh.SCALE[cls])
    q[:4] = rows[12:16].astype(F32)
    return rows, q, kh.ordered_dist(rows, q, NEG_DOT)   # (the first four queries are rows; the reference distances [NQ x N])


def both(g, call, n, nq, d, k, tagged, knn_chunk=None):
    lib, out = g.load_library(), {}   # (dot filter's answer, scan's answer) of call(), the plan checked under the knob right before it
    want = {"kernel": "knn_half_dot_filter_kernel<2, %s>" % ("true" if tagged else "false"), "path": "filter", "pool": False, "packed": False}
    for v in (0, 2):
        with ku.knobs(g, knn_chunk=knn_chunk):
            try:
                assert lib.gbnns_debug_knob(b"knn_half_dot", v) == 0
                plan = g.knn_half_plan(n, nq, d, k, NEG_DOT, tagged=tagged)
                assert plan == want if v else plan["path"] == "scan"
                out[v] = call()
            finally:
                lib.gbnns_debug_knob(b"knn_half_dot", 0)
    return out[2], out[0]


def check(g, rows, q, dist, k, tagged=False, self_offset=-1, what=""):
    kw, allowed = dict(self_offset=self_offset), None
    if tagged:   # (words that allow every row, none, a share, the last 40 rows only, and rows 0 .. 6 only: fewer than k = 10)
        T, Q = kt.tag_table(7900, len(rows)), kt.query_words(len(q))
        kw.update(row_tags=T, query_tags=Q)
        allowed = (T[None, :] & Q[:, None]) != 0
    dot, scan = both(g, lambda: g.exact_knn(rows, q, k, NEG_DOT, want_dist=True, **kw), len(rows), len(q), rows.shape[1], k, tagged, knn_chunk=CHUNK)
    kh.same(dot, kh.knn_of(dist, k, allowed=allowed, self_offset=self_offset), what + " against the reference")
    kh.same(dot, scan, what + " against the scan")


@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "tagged"])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", [8, 72, 200, 1024])
def test_equals_the_reference_and_the_scan(g, d, k, tagged):
    check(g, *data(d), k, tagged, what="d %d" % d)


@pytest.mark.parametrize("cls", ["subnormal", "large"])
def test_magnitude_classes(g, cls):
    rows, q, dist = data(200, cls)
    n2 = (rows.astype(np.float64) ** 2).sum(1)
    assert cls != "large" or (2.0 ** -96 <= n2.min() and n2.max() <= 2.0 ** 96)   # (covered: the filter's answer, not the scan's)
    check(g, rows, q, dist, 10, what=cls)


@pytest.mark.parametrize("case", ["query beyond 2^96", "zero row"])
def test_a_norm_beyond_the_bound_sends_the_call_to_the_scan(g, case):
    rows, q = (a.copy() for a in data(200)[:2])
    if case == "zero row":
        rows[500] = 0   # |x| = 0: no scale for the error
    else:
        q[77] = 0
        q[77, 3] = F32(2.0 ** 50)   # |q|^2 = 2^100 (the plan knows the shape, not the data, and names the filter)
    check(g, rows, q, kh.ordered_dist(rows, q, NEG_DOT), 10, what=case)


def test_self_lists(g):
    rows, _, _ = data(200)
    q = np.ascontiguousarray(rows[:NQ].astype(F32))
    check(g, rows, q, kh.ordered_dist(rows, q, NEG_DOT), 10, tagged=True, self_offset=0, what="self lists")


def test_a_handle_is_swept_in_place(g):
    rows, q, dist = data(200)
    off, nbr = np.arange(N + 1, dtype=np.uint64), ((np.arange(N) + 1) % N).astype(np.uint32)
    ix = g.Index(rows, off, nbr, db_low=np.ascontiguousarray(rows[:, :8].astype(F32)), metric=NEG_DOT)
    assert ix.is_half_base
    dot, scan = both(g, lambda: ix.exact_knn(q, 10, want_dist=True, half_scan=True), N, NQ, 200, 10, False, knn_chunk=CHUNK)
    ix.close()
    kh.same(dot, kh.knn_of(dist, 10), "handle against the reference")
    kh.same(dot, scan, "handle against the scan")


def test_cancellation(g):
    d, k = 96, 10
    signs = np.random.default_rng(96).integers(0, 2, (N, d)).astype(F32) * 2 - 1
    rows = (signs * F32(2.0 ** 10)).astype(np.float16)
    q = np.ascontiguousarray(rows[7:7 + NQ].astype(F32))   # some rows' own patterns; not self lists: the row itself is the best answer
    dist = kh.ordered_dist(rows, q, NEG_DOT)
    want = kh.knn_of(dist, k)
    assert (want[1][:, k - 1] == want[1][:, k - 2]).mean() > 0.5   # ties at the threshold are the rule
    check(g, rows, q, dist, k, what="cancellation")


def test_overflowing_chunks_are_scanned(g):
    n, d, k, chunk, later, cap = 16 * 1024 + 37, 960, 10, 1024, 1088, 256
    rng = np.random.default_rng(9601)
    rows = (rng.random((n, d), dtype=F32) + F32(20)).astype(np.float16)
    q = rng.random((NQ, d), dtype=F32) + F32(20)
    b, qq = rows.astype(np.float64), q.astype(np.float64)
    D = qq @ b.T
    n2 = (b * b).sum(1)
    assert 2.0 ** -96 <= n2.min() and n2.max() <= 2.0 ** 96   # (about 4e5)
    P = np.sqrt((qq * qq).sum(1))[:, None] * np.sqrt(n2)[None, :]
    T1, second = np.sort(D[:, :chunk], 1)[:, -k], slice(chunk, 2 * chunk)
    within = (D[:, second] + 0.9 * P[:, second] / 1024 >= T1[:, None]).sum(1)
    assert within.min() > cap, (within.min(), within.max())   # the second chunk overflows every query's list (318 to 338 rows within 0.9 of the slack)
    Tn = np.sort(D, 1)[:, -k]   # later chunks are rescored: under the final thresholds none holds a list's worth within 1.1 of the slack
    kept = D + 1.1 * P / 1024 >= Tn[:, None]
    assert max(kept[:, r0:r0 + later].sum(1).max() for r0 in range(2 * chunk, n, later)) < cap   # (at most 207)
    dot, scan = both(g, lambda: g.exact_knn(rows, q, k, NEG_DOT, want_dist=True), n, NQ, d, k, False)   # ("knn_chunk" at its default: chunks of 1 088 rows)
    kh.same(dot, scan, "overflowing chunks against the scan")
    sample = np.unique(np.concatenate([np.arange(0, NQ, 11), [int(within.argmax())]]))   # the reference for 16 queries, the worst among them
    kh.same(dot, kh.knn_of(kh.ordered_dist(rows, np.ascontiguousarray(q[sample]), NEG_DOT), k), "overflowing chunks against the reference", queries=sample)
