"""knn_half_wide.hip on an MI355X (run with -m gpu): gbnns_exact_knn_half / gbnns_index_exact_knn_half on binary16 rows wider than 128 dims
with "knn_half_wide" = 2 -- the K-looped f16 matrix-core filter in front of the heaps -- against the plain reference of
tests/knn_half_util.py (ordered float32 sums on the widened rows, numpy's sort of (distance, id)) and against the same call with the knob
at 0 (the exact scan), ids and distance bit patterns; gbnns_debug_knn_half_plan, asked right before the call, names the wide kernel.  No
tolerance.  Shapes: "knn_chunk" = 64, n = 1 037, n_q = 128 + 37 -- sixteen chunks of 64 rows (each a partial block of 128 rows), a last one of 13, a
second workgroup of queries with 37 of its 128; rows from knn_half_util.half_rows (every eighth row a duplicate: ties to the lower id).
d = 136 (in place; dp = 144: nine K steps, the last K step's second chunk beyond the row, the last stage half empty), 200 (in place), 300
(the free call sweeps a copy at stride 304, the handle its rows at stride 304 in place), 960, 1024 (the longest row of the bound).

test_overflowing_chunks_are_scanned mirrors tests/test_gpu_knn_wide.py's: 16 421 rows of float16(uniform [2, 3)) at d = 960; the second
chunk overflows a list of 256 (asserted in float64) and is scanned inside the call, the last (229 rows) cannot and is rescored."""
import contextlib
import functools

import numpy as np
import pytest

import knn_bytes_util as ku
import knn_half_util as kh
import knn_instances as ki
import knn_tagged_util as kt

pytestmark = pytest.mark.gpu

L2, F32 = 0, np.float32
N, NQ, CHUNK = ki.N, 128 + 37, ki.CHUNK


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@contextlib.contextmanager
def half_wide(g, v, **kw):
    lib = g.load_library()
    with ku.knobs(g, **kw):
        try:
            assert lib.gbnns_debug_knob(b"knn_half_wide", v) == 0
            yield
        finally:
            lib.gbnns_debug_knob(b"knn_half_wide", 0)


@functools.lru_cache(maxsize=None)
def data(d, cls="unit"):
    rng = np.random.default_rng(9800 + d + kh.SCALE[cls])
    rows = kh.half_rows(rng, N, d, cls)
    q = rng.standard_normal((NQ, d)).astype(F32) * F32(2.0 ** kh.SCALE[cls])
    q[:4] = rows[12:16].astype(F32)
    return rows, q, kh.ordered_dist(rows, q, L2)   # (the first four queries are rows; the reference distances [NQ x N])


def both(g, call, n, nq, d, k, tagged, stride=0, knn_chunk=None):
    """(wide filter's answer, scan's answer) of call(), the plan checked under the knob right before it."""
    with half_wide(g, 0, knn_chunk=knn_chunk):
        assert g.knn_half_plan(n, nq, d, k, stride=stride, tagged=tagged)["path"] == "scan"
        scan = call()
    with half_wide(g, 2, knn_chunk=knn_chunk):
        want = {"kernel": "knn_half_wide_filter_kernel<2, %s>" % ("true" if tagged else "false"), "path": "filter", "pool": False,
                "packed": (stride or d) % 8 != 0}
        assert g.knn_half_plan(n, nq, d, k, stride=stride, tagged=tagged) == want
        wide = call()
    return wide, scan


def check(g, rows, q, dist, k, tagged=False, self_offset=-1, what=""):
    kw, allowed = dict(self_offset=self_offset), None
    if tagged:   # (words that allow every row, none, a share, the last 40 rows only, and rows 0 .. 6 only: fewer than k = 10)
        T, Q = kt.tag_table(7900, len(rows)), kt.query_words(len(q))
        kw.update(row_tags=T, query_tags=Q)
        allowed = (T[None, :] & Q[:, None]) != 0
    wide, scan = both(g, lambda: g.exact_knn(rows, q, k, L2, want_dist=True, **kw), len(rows), len(q), rows.shape[1], k, tagged, knn_chunk=CHUNK)
    kh.same(wide, kh.knn_of(dist, k, allowed=allowed, self_offset=self_offset), what + " against the reference")
    kh.same(wide, scan, what + " against the scan")


@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "tagged"])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", [136, 200, 300, 960, 1024])
def test_equals_the_reference_and_the_scan(g, d, k, tagged):
    check(g, *data(d), k, tagged, what="d %d" % d)


@pytest.mark.parametrize("cls", ["subnormal", "large"])
def test_magnitude_classes(g, cls):
    check(g, *data(960, cls), 10, what=cls)


def test_a_query_beyond_the_bound_sends_the_call_to_the_scan(g):
    rows, q, _ = data(960)
    q = q.copy()
    q[77] = 0
    q[77, 3] = F32(2.0 ** 50)   # |q|^2 = 2^100: outside 2^-96 .. 2^96 (the plan knows the shape, not the queries, and names the filter)
    check(g, rows, q, kh.ordered_dist(rows, q, L2), 10, what="beyond 2^96")


def test_self_lists(g):
    rows, _, _ = data(300)
    q = np.ascontiguousarray(rows[:NQ].astype(F32))
    check(g, rows, q, kh.ordered_dist(rows, q, L2), 10, tagged=True, self_offset=0, what="self lists")


def test_a_handle_is_swept_in_place_at_its_stride(g):
    rows, q, dist = data(300)
    off, nbr = np.arange(N + 1, dtype=np.uint64), ((np.arange(N) + 1) % N).astype(np.uint32)
    ix = g.Index(rows, off, nbr, db_low=np.ascontiguousarray(rows[:, :8].astype(F32)))   # (resident rows at d_pad = 304 halves)
    assert ix.is_half_base
    wide, scan = both(g, lambda: ix.exact_knn(q, 10, want_dist=True, half_scan=True), N, NQ, 300, 10, False, stride=304, knn_chunk=CHUNK)
    ix.close()
    kh.same(wide, kh.knn_of(dist, 10), "handle against the reference")
    kh.same(wide, scan, "handle against the scan")


def test_overflowing_chunks_are_scanned(g):
    n, d, k, chunk, cap = 16 * 1024 + 37, 960, 10, 1024, 256
    rng = np.random.default_rng(9601)
    rows = (rng.random((n, d), dtype=F32) + F32(2)).astype(np.float16)
    q = rng.random((NQ, d), dtype=F32) + F32(2)
    # the second chunk overflows: under the first chunk's exact thresholds more rows than a list holds lie within 0.9 of the slack
    b, qq = rows[:2 * chunk].astype(np.float64), q.astype(np.float64)
    S = (qq * qq).sum(1)[:, None] + (b * b).sum(1)[None, :]
    D = S - 2 * qq @ b.T
    T1 = np.sort(D[:, :chunk], 1)[:, k - 1]
    within = (D[:, chunk:] <= T1[:, None] + 0.9 * S[:, chunk:] / 1024).sum(1)
    assert within.max() > cap, within.max()   # (470 rows for the worst query)
    # ("knn_chunk" at its default: chunks of up to a sixteenth of the set, 1 088 rows; the last, 229 rows, cannot overflow: rescored)
    wide, scan = both(g, lambda: g.exact_knn(rows, q, k, L2, want_dist=True), n, NQ, d, k, False)
    kh.same(wide, scan, "overflowing chunks against the scan")
    sample = np.unique(np.concatenate([np.arange(0, NQ, 11), [int(within.argmax())]]))   # the reference for 16 queries, the worst among them
    kh.same(wide, kh.knn_of(kh.ordered_dist(rows, np.ascontiguousarray(q[sample]), L2), k), "overflowing chunks against the reference", queries=sample)
