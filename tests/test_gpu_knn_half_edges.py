"""The edges of gbnns_exact_knn_half's matrix-core sweep on an MI355X (run with -m gpu), ids and distance bit patterns against the plain
reference of tests/knn_half_util.py (ordered float32 sums on the widened rows, numpy's sort of (distance, id)) -- no tolerance anywhere:
  - a workgroup that walks several blocks of 32 rows: the second register set and both exits of the ping-pong loop
  - query magnitudes inside one batch, and both sides of the range outside which the whole call takes the exact scan
  - cancellation and mass ties: lists that overflow, the chunk rescanned (heaps) and re-swept in pieces (pools)
  - half-base handles whose row stride is not the row length
  - the pool path: query slabs, self_offset, overflow, padding
Every test names the lines of knn_half.hip / graph_api.cpp it exists for."""
import functools
import time

import numpy as np
import pytest

import knn_bytes_util as ku
import knn_half_util as hu
from knn_half_util import F32

pytestmark = pytest.mark.gpu

MAX_HALF = 65504.0


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


def knobs(g, **kw):
    return ku.knobs(g, **dict(dict(knn_filter=2, knn_chunk=512, knn_pool_min_k=64), **kw))


# ---- a workgroup walks several row blocks ----

SWEEP_QB = {1: 4, 2: 4, 3: 2, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1}   # knn_half_sweep_pick: K steps of 16 halves -> query blocks a wavefront


def sweep_launch(nq, rows, qb, simds):
    """launch_half_sweep_tt and the kernel's division of a chunk's blocks of 32 rows, restated: gx, gy, per and the blocks each blockIdx.y
    walks (b_hi - b_lo; 0: it returns at b_lo >= b_hi)."""
    gx, blocks = -(-nq // (128 * qb)), -(-rows // 32)
    gy = 1 if gx >= simds else -(-simds // gx)
    gy = max(1, min(gy, blocks))
    per = -(-blocks // gy)
    return {"gx": gx, "gy": gy, "per": per, "blocks": blocks, "walks": [max(0, min(blocks, y * per + per) - y * per) for y in range(gy)]}


def swept_chunks(n, k, pool, knn_chunk=1 << 15):
    """knn_rows_call's chunk schedule, restated: [(first row, rows)] of every launch of the sweep.  Heaps: the first rows are scanned
    exactly and not swept; pools: knn_sweep_chunks, the first chunk of (4 k + 64) & ~63 rows included."""
    limit = max(64, (n // 16 + 63) & ~63)
    out = []
    if pool:
        max_chunk, r0 = min(4 * knn_chunk, limit), min(n, (4 * k + 64) & ~63)
        out.append((0, r0))
    else:
        max_chunk = min(knn_chunk, limit)
        r0 = min(n, (max(min(max_chunk, 8192), 4 * k) + 63) & ~63)
    while r0 < n:
        rows = min(max_chunk, r0, n - r0)
        out.append((r0, rows))
        r0 += rows
    return out


def loop_edges(n, nq, k, pool, qb, simds):
    """What a call of that shape reaches of the sweep's row loop (knn_half.hip, `for (uint32_t rb = b_lo;;)`)."""
    chunks = swept_chunks(n, k, pool)
    launches = [sweep_launch(nq, rows, qb, simds) for _, rows in chunks]
    walks = [w for l in launches for w in l["walks"]]
    return {"odd": any(w >= 3 and w % 2 == 1 for w in walks),      # leaves by the first break, behind a sweep of set 0 that followed one of set 1
            "even": any(w >= 2 and w % 2 == 0 for w in walks),    # leaves by the second break, behind a sweep of set 1
            "idle": any(w == 0 for w in walks),                   # returns at b_lo >= b_hi
            "partial": chunks[-1][1] % 32 != 0,                   # the set's last block holds fewer than 32 rows
            "chunks": chunks, "launches": launches}


def rows_for_loop_edges(nq, k, pool, qb, simds):
    """The smallest n = 64 j + 37 at which all four hold, on the device at hand."""
    for n in range(1024 + 37, (1 << 17) + 1, 64):
        e = loop_edges(n, nq, k, pool, qb, simds)
        if e["odd"] and e["even"] and e["idle"] and e["partial"]:
            return n, e
    pytest.fail("no n <= 2^17 lets a sweep workgroup walk three blocks of rows on a device of %d SIMDs at n_q = %d: the shape formula "
                "needs more than 2^17 rows" % (simds, nq))


LOOP_D, LOOP_NQ = 96, 4133


@functools.lru_cache(maxsize=2)
def loop_data(n):
    rng = np.random.default_rng(9100 + n)
    rows = hu.half_rows(rng, n, LOOP_D)
    q = rng.standard_normal((LOOP_NQ, LOOP_D)).astype(F32)
    q[:4] = rows[12:16].astype(F32)
    sample = np.concatenate([np.arange(16), np.linspace(16, LOOP_NQ - 17, 16).astype(np.int64), np.arange(LOOP_NQ - 16, LOOP_NQ)])
    assert len(set(sample.tolist())) == 48
    return rows, q, sample, hu.ordered_dist(rows, np.ascontiguousarray(q[sample]), ku.L2)


@pytest.mark.parametrize("k,tagged", [(10, False), (64, False), (10, True)])
def test_a_workgroup_walks_several_row_blocks(g, k, tagged):
    """knn_half.hip, the two register sets of knn_half_sweep_kernel (`request_block(b_lo, xa0, ...)` to the end of the kernel): set 1
    (xa1 / nx1 / tg1), the re-request into set 0 while set 1 is swept, both `break`s and the return at `b_lo >= b_hi`; the arithmetic of
    launch_half_sweep_tt (gx, gy) and of the kernel (per, b_lo, b_hi), and graph_api.cpp's chunk schedules (knn_rows_call: max_chunk,
    first; knn_sweep_chunks), restated above.  No shape elsewhere in the suite reaches them: a chunk is at most n / 16 rows, so below
    about 32 simds / gx rows -- 33 000 on 256 CUs at one query workgroup column per 128 queries -- every workgroup walks one block.
    n comes from the device's SIMD count.  On an MI355X (256 CUs, simds = 1 024) with n_q = 4 133 at d = 96 (QB = 1): gx = 33, gy = 32,
    n = 32 805 for both paths, chunks of at most 2 112 rows = 66 blocks: per = 3, blockIdx.y 0 .. 21 walk three blocks, 22 .. 31 return;
      k = 10 (filter):  14 such chunks from row 2 112 on, then 1 125 rows = 36 blocks (the last of 5 rows): per = 2, 18 walk two, 14 return
      k = 64 (pool):    chunks of 320, 320, 640, 1 280 (40 blocks: per = 2), 2 112 x 14 and 677 rows (22 blocks, the last of 5 rows)
    Every query byte for byte against the same call under "knn_filter" = 0 (the exact scan), 48 queries -- the first 16, the last 16,
    16 spread between -- against the plain reference."""
    import torch
    t0 = time.time()
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    pool = k >= 64
    n, e = rows_for_loop_edges(LOOP_NQ, k, pool, SWEEP_QB[LOOP_D // 16], simds)
    assert e["odd"] and e["even"] and e["idle"] and e["partial"] and n <= 1 << 17
    print("simds", simds, "n", n, "chunks", e["chunks"])
    for (r0, rows), l in zip(e["chunks"], e["launches"]):
        print("  rows", r0, rows, "gx", l["gx"], "gy", l["gy"], "per", l["per"], "blocks", l["blocks"], "walks", sorted(set(l["walks"])))
    rows, q, sample, dist = loop_data(n)
    kw, allowed = {}, None
    if tagged:
        T = np.where(np.arange(n) % 3 == 0, 1, 2).astype(np.uint32)
        Q = np.array([1, 2, 3], np.uint32)[np.arange(LOOP_NQ) % 3]
        kw, allowed = dict(row_tags=T, query_tags=Q), (T[None, :] & Q[sample, None]) != 0
    with ku.knobs(g, knn_filter=2):
        p = g.knn_half_plan(n, LOOP_NQ, LOOP_D, k, tagged=tagged)
        assert p == {"kernel": "knn_half_sweep_kernel<6, 1, %s>" % ("true" if tagged else "false"), "path": "pool" if pool else "filter",
                     "pool": pool, "packed": False}, p
        got = g.exact_knn(rows, q, k, want_dist=True, **kw)
    with ku.knobs(g, knn_filter=0):
        assert g.knn_half_plan(n, LOOP_NQ, LOOP_D, k, tagged=tagged)["path"] == "scan"
        scan = g.exact_knn(rows, q, k, want_dist=True, **kw)
    hu.same(got, scan, "the exact scan")
    hu.same(got, hu.knn_of(dist, k, allowed=allowed), "the reference, 48 queries", queries=sample)
    print("wall time %.2f s" % (time.time() - t0))


# ---- query magnitudes ----

N2, NQ2 = 2085, 130


def magnitude_rows(rng, d, cls="unit"):
    """Unit-scale (or `cls`) rows with zero rows and rows of +-65 504 in alternating sign among them."""
    rows = hu.half_rows(rng, N2, d, cls)
    alt = np.where(np.arange(d) % 2 == 0, MAX_HALF, -MAX_HALF).astype(np.float16)
    rows[100], rows[101], rows[1500] = 0, 0, 0
    if cls == "unit":
        rows[200], rows[201], rows[1700] = alt, -alt, alt
    return rows


def magnitude_batch(rng, rows, d):
    """130 finite queries: 2^e-scaled ones for e = -40 .. 40 in steps of 5, the zero query, a query whose coordinates are 2^-120 (|q|^2
    underflows to 0 and the split's exponent t is clamped -- as for the zero row plus one ulp below, a subnormal float), needles (one
    coordinate 2^6, the rest 2^-14 x normal: their lo parts are subnormal halves after scaling), +-65 504 everywhere, rows plus one
    float32 ulp in one coordinate, and unit queries for the rest."""
    q = rng.standard_normal((NQ2, d)).astype(F32)
    i = 0
    for e in range(-40, 41, 5):
        q[i] *= F32(2.0 ** e)
        i += 1
    q[i] = 0
    q[i + 1] = F32(2.0 ** -120) * np.round(4 * rng.standard_normal(d)).astype(F32)
    q[i + 1, 0] = F32(2.0 ** -120)
    i += 2
    for j in range(8):
        q[i] = F32(2.0 ** -14) * rng.standard_normal(d).astype(F32)
        q[i, (5 * j) % d] = F32(64.0) * (-1) ** j
        i += 1
    q[i] = F32(MAX_HALF)
    q[i + 1] = np.where(np.arange(d) % 2 == 0, F32(MAX_HALF), F32(-MAX_HALF))
    i += 2
    for j, row in enumerate((12, 14, 200, 100)):   # (14: a duplicated row, 200: +-65 504, 100: a zero row)
        q[i] = rows[row].astype(F32)
        q[i, (7 * j) % d] = np.nextafter(q[i, (7 * j) % d], F32(np.inf), dtype=F32)
        i += 1
    assert i < NQ2 - 60 and np.isfinite(q).all()
    return q


@pytest.mark.parametrize("d", (40, 128))
def test_query_magnitudes_in_one_batch(g, d):
    """knn_half.hip, knn_half_qsplit_kernel: the per-query scale s = 2^t (`t = m == 0.f ? 0 : 139 - eb`, its clamp, `inv[row]`), hi / lo
    with subnormal lo parts, the zero query's `covered`; knn_half_sweep_kernel's `fmaf(acc, qinv, cinit)` with a different qinv per lane.
    d = 40: K = 3, QB = 2, lane half h = 1 of the last K step clamped to chunk 4; d = 128: K = 8."""
    rng = np.random.default_rng(9200 + d)
    rows = magnitude_rows(rng, d)
    q = magnitude_batch(rng, rows, d)
    n2 = (q.astype(np.float64) ** 2).sum(1)
    assert n2.max() < 2.0 ** 95 and n2[n2 > 0].min() < 2.0 ** -70 and (n2 == 0).sum() == 1 and ((q * q).sum(1, dtype=F32) == 0).sum() == 3
    with knobs(g):
        assert g.knn_half_plan(N2, NQ2, d, 10)["path"] == "filter"
        got = g.exact_knn(rows, q, 10, want_dist=True)
    hu.same(got, hu.knn_of(hu.ordered_dist(rows, q, ku.L2), 10), "magnitudes d %d" % d)


def one_coordinate(d, value, at=3):
    q = np.zeros(d, F32)
    q[at] = value
    return q


# (what the odd query is, the rows' class): |q|^2 = 2^100 and 2^-100 are outside the bound's range -- the whole call takes the exact
# scan; 2^96 and 2^-96 themselves are inside, the next float32 beyond them is not
RANGE_CASES = {
    "2^100": (F32(2.0 ** 50), "unit"), "2^-100": (F32(2.0 ** -50), "unit"),
    "2^96": (F32(2.0 ** 48), "large"), "above 2^96": (np.nextafter(F32(2.0 ** 48), F32(np.inf), dtype=F32), "large"),
    "2^-96": (F32(2.0 ** -48), "subnormal"), "below 2^-96": (np.nextafter(F32(2.0 ** -48), F32(0), dtype=F32), "subnormal"),
}


@pytest.mark.parametrize("what", list(RANGE_CASES))
@pytest.mark.parametrize("d", (40, 128))
def test_query_range_boundary(g, d, what):
    """knn_half.hip, knn_half_qsplit_kernel's `covered` (2^-96 <= |q|^2 <= 2^96) and graph_api.cpp, knn_rows_call's `queries_covered` /
    `if (!covered) pool_path = filter = false`: one query of the batch at or beyond the range, the others at their rows' scale -- their
    lists must be right by whichever route the call takes.  The route itself cannot be observed: gbnns_debug_knn_half_plan knows the
    shape and not the queries, so it names the sweep here even where the call then takes the scan; the plan assertion below only says
    that the shape would be swept if every query were covered."""
    value, cls = RANGE_CASES[what]
    rng = np.random.default_rng(9300 + d)
    rows = magnitude_rows(rng, d, cls)
    q = rng.standard_normal((NQ2, d)).astype(F32) * F32(2.0 ** hu.SCALE[cls])
    q[:4] = rows[12:16].astype(F32)
    q[77] = one_coordinate(d, value)
    n2 = float((q[77] * q[77]).sum(dtype=F32))
    assert np.isfinite(q).all() and (2.0 ** -96 <= n2 <= 2.0 ** 96) == (what in ("2^96", "2^-96")), n2
    dist = hu.ordered_dist(rows, q, ku.L2)
    for k in (10, 64):
        with knobs(g):
            assert g.knn_half_plan(N2, NQ2, d, k)["path"] == ("pool" if k == 64 else "filter")
            got = g.exact_knn(rows, q, k, want_dist=True)
        hu.same(got, hu.knn_of(dist, k), "%s d %d k %d" % (what, d, k))


# ---- cancellation and ties ----

N3 = 8200   # (n / 16 = 512: chunks of 512 rows under "knn_chunk" = 512, longer than a list of 256 or of 464 entries)


@functools.lru_cache(maxsize=None)
def cancellation(d):
    """Rows 100 + 2^-4 round(4 normal) -- exact in binary16 --, every distinct row eight times (independent draws have no two equal
    distances: the ties must come from equal rows), sorted farthest first from the centre (100, .., 100); queries drawn like the rows, as
    floats, plus 2^-10 noise -- query 0 the centre itself, queries 1 .. 7 the centre plus that noise."""
    rng = np.random.default_rng(9400 + d)
    distinct = (100 + np.round(4 * rng.standard_normal((N3 // 8 + 1, d))) / 16).astype(np.float16)
    assert np.array_equal(distinct.astype(np.float64), 100 + np.round((distinct.astype(np.float64) - 100) * 16) / 16)
    rows = np.repeat(distinct, 8, axis=0)[rng.permutation(len(distinct) * 8)][:N3]
    rows = np.ascontiguousarray(rows[np.argsort(-((rows.astype(np.float64) - 100) ** 2).sum(1), kind="stable")])
    q = (100 + np.round(4 * rng.standard_normal((NQ2, d))) / 16).astype(F32)
    q[:8] = 100
    q += F32(2.0 ** -10) * rng.standard_normal((NQ2, d)).astype(F32)
    q[0] = 100
    return rows, q, hu.ordered_dist(rows, q, ku.L2)


@pytest.mark.parametrize("k", (10, 100))
@pytest.mark.parametrize("d", (32, 96))
def test_cancellation_and_mass_ties(g, d, k):
    """|q|^2 + |x|^2 (about 2 d 10^4) dwarfs the distances (a few units), so the sweep's slack keeps nearly every row, and for the centre
    query every row of a chunk is within its k-th distance so far whatever the slack: lists overflow in every swept chunk and the
    fallbacks run with ties at the threshold -- graph_api.cpp, knn_rows_call's `if (h_flag)` (the chunk scanned exactly, k = 10 on heaps)
    and knn_sweep_chunks' pieces of first_rows (k = 100 in pools), neither of which may offer a row twice; knn_half.hip's
    `else *p.overflow = 1u`.  Every distinct row eight times: the k-th distance is a tie.  Both preconditions are asserted from the
    restated schedule and the reference alone."""
    rows, q, dist = cancellation(d)
    pool = k == 100
    s = np.sort(dist, axis=1)
    assert np.count_nonzero(s[:, k - 1] == s[:, k]) >= NQ2 // 2
    cap = 4 * k + 64 if pool else max(256, 4 * k + 64)   # knn_rows_call: entries of a query's list
    chunks = swept_chunks(N3, k, pool, knn_chunk=512)
    long = [(r0, n) for r0, n in chunks if r0 > 0 and n > cap]
    assert len(long) >= 8 and max(n for _, n in chunks) == 512
    for r0, n in long:   # rows of the chunk within the k-th distance over the rows before it: the sweep must keep them, and cannot
        kth = np.partition(dist[:, :r0], k - 1, axis=1)[:, k - 1]
        within = (dist[:, r0:r0 + n] <= kth[:, None]).sum(1)
        assert within[0] == n and within.max() > cap, (r0, n, within[:8])
    with knobs(g):
        assert g.knn_half_plan(N3, NQ2, d, k)["path"] == ("pool" if pool else "filter")
        got = g.exact_knn(rows, q, k, want_dist=True)
    hu.same(got, hu.knn_of(dist, k), "cancellation d %d k %d" % (d, k))


# ---- handles and strides ----

@pytest.mark.parametrize("d", (20, 30, 8))
def test_handles_at_their_own_stride(g, d):
    """graph_api.cpp, knn_resident_call's `c.bstride = ix->d_pad` through KnnHalfWork::prepare / sweep (`stride`, `last_chunk`) and the
    scan / rescore launches at bstride != dim.  d = 20: d_pad 24, swept in place, pad columns inside chunk 2, chunk 3 clamped; d = 30: no
    sweep (d % 4 != 0), the scan at stride 32; d = 8: one chunk, lane half h = 1 always clamped."""
    import torch
    k, d_pad = 10, (d + 7) // 8 * 8
    rng = np.random.default_rng(9500 + d)
    rows = hu.half_rows(rng, N2, d)
    q = rng.standard_normal((NQ2, d)).astype(F32)
    q[:4] = rows[12:16].astype(F32)
    off, nbr = np.arange(N2 + 1, dtype=np.uint64), ((np.arange(N2) + 1) % N2).astype(np.uint32)
    T = np.where(np.arange(N2) % 2 == 0, 1, 2).astype(np.uint32)
    Q = np.array([1, 2, 3], np.uint32)[np.arange(NQ2) % 3]
    dist = hu.ordered_dist(rows, q, ku.L2)
    want, want_t = hu.knn_of(dist, k), hu.knn_of(dist, k, allowed=(T[None, :] & Q[:, None]) != 0)
    dq = torch.from_numpy(q).cuda()
    with knobs(g):
        p = g.knn_half_plan(N2, NQ2, d, k, stride=d_pad)
        assert p["path"] == ("scan" if d % 4 else "filter") and p["packed"] is False, p
        if d % 4 == 0:
            assert g.knn_half_plan(N2, NQ2, d, k)["packed"] is (d % 8 != 0)   # (the free call on the caller's array: d = 20 sweeps a copy)
        hu.same(g.exact_knn(rows, q, k, want_dist=True), want, "free call")
        hu.same(g.exact_knn(rows, q, k, want_dist=True, row_tags=T, query_tags=Q), want_t, "free call, tagged")
        ix = g.Index(rows, off, nbr, db_low=np.ascontiguousarray(rows[:, :8].astype(F32)))
        assert ix.is_half_base
        hu.same(ix.exact_knn(q, k, want_dist=True, half_scan=True), want, "handle, HOST")
        hu.same(ix.exact_knn(dq, k, want_dist=True, half_scan=True), want, "handle, DEVICE")
        ix.set_tags(T)
        hu.same(ix.exact_knn(q, k, want_dist=True, half_scan=True), want, "handle with a tag table, untagged")
        hu.same(ix.exact_knn(q, k, query_tags=Q, want_dist=True, half_scan=True), want_t, "handle, tagged, HOST")
        hu.same(ix.exact_knn(dq, k, query_tags=torch.from_numpy(Q.view(np.int32)).cuda(), want_dist=True, half_scan=True), want_t,
                "handle, tagged, DEVICE")
        ix.close()


# ---- the pool path ----

@functools.lru_cache(maxsize=None)
def pool_data(nq=300):
    rng = np.random.default_rng(9600 + nq)
    rows = hu.half_rows(rng, N2, 96)
    q = rng.standard_normal((nq, 96)).astype(F32)
    q[:4] = rows[12:16].astype(F32)
    return rows, q, hu.ordered_dist(rows, q, ku.L2)


@pytest.mark.parametrize("tagged", (False, True))
def test_pool_query_slabs(g, tagged):
    """graph_api.cpp, knn_rows_call's pool branch: `for (uint32_t q0 = 0; q0 < nq; q0 += slab)` with knn_slab_at's offsets -- the queries,
    their tag words (`sl.qtags`), the outputs -- at slabs of 128 / 128 / 44 queries."""
    rows, q, dist = pool_data()
    k, kw, allowed = 64, {}, None
    if tagged:
        import knn_tagged_util as kt
        T, Q = kt.tag_table(9601, N2), kt.query_words(300)   # (words that allow nothing, everything, 7 rows, the last 40 rows among them)
        kw, allowed = dict(row_tags=T, query_tags=Q), (T[None, :] & Q[:, None]) != 0
    with knobs(g, knn_slab=128):
        assert g.knn_half_plan(N2, 300, 96, k, tagged=tagged)["path"] == "pool"
        assert ku.slabs(g.knn_slab(300, k), 300) == [(0, 128), (128, 128), (256, 44)]
        got = g.exact_knn(rows, q, k, want_dist=True, **kw)
    hu.same(got, hu.knn_of(dist, k, allowed=allowed), "slabs")


def test_pool_self_offset(g):
    """graph_api.cpp, knn_slab_at's `sl.self_offset` into the pool kernels (knn_scan_kernels.h, knn_pool_update_kernel), two slabs."""
    rows, _, _ = pool_data()
    q = rows[5:5 + 300].astype(F32)
    with knobs(g, knn_slab=128):
        assert g.knn_half_plan(N2, 300, 96, 64)["path"] == "pool"
        got = g.exact_knn(rows, q, 64, want_dist=True, self_offset=5)
    want = hu.knn_of(hu.ordered_dist(rows, q, ku.L2), 64, self_offset=5)
    assert not (want[0] == (np.arange(300) + 5)[:, None]).any()
    hu.same(got, want, "self_offset")


def test_pool_overflow_is_swept_again_in_pieces(g):
    """graph_api.cpp, knn_sweep_chunks' `for (uint64_t r1 = r0; ...)`: rows sorted farthest first, so every row of a later chunk (512 rows,
    lists of 320) is nearer than all rows before it and the lists of queries near the origin overflow."""
    n, d, k = 8200, 32, 64
    rng = np.random.default_rng(9700)
    rows = hu.half_rows(rng, n, d)
    rows = np.ascontiguousarray(rows[np.argsort(-(rows.astype(np.float64) ** 2).sum(1), kind="stable")])
    q = (rng.standard_normal((NQ2, d)) * 0.01).astype(F32)
    q[0] = 0   # for the zero query the order is farthest first for certain
    assert (np.diff((rows.astype(np.float64) ** 2).sum(1)) <= 0).all()
    with knobs(g):
        assert g.knn_half_plan(n, NQ2, d, k)["path"] == "pool"
        chunks = swept_chunks(n, k, True, knn_chunk=512)
        assert max(r for _, r in chunks) == 512 > 4 * k + 64
        got = g.exact_knn(rows, q, k, want_dist=True)
    hu.same(got, hu.knn_of(hu.ordered_dist(rows, q, ku.L2), k), "pool overflow")


def test_pool_pads_where_a_word_allows_fewer_than_k_rows(g):
    """knn_scan_kernels.h, knn_pool_update_kernel / launch_knn_pool_finalize: a pool that never fills -- NONE_ID / +inf behind the rows a
    word allows (7 rows, 40 rows, none), full lists beside it in the same call."""
    import knn_tagged_util as kt
    rows, q, dist = pool_data()
    T, Q = kt.tag_table(9602, N2), kt.query_words(300)
    counts = {int(w): int(np.count_nonzero(T & w)) for w in np.unique(Q)}
    assert counts[1 << kt.FEW_BIT] == 7 and counts[1 << kt.LATE_BIT] == 40 and counts[0] == 0 and counts[1] == N2
    with knobs(g):
        p = g.knn_half_plan(N2, 300, 96, 64, tagged=True)
        assert p == {"kernel": "knn_half_sweep_kernel<6, 1, true>", "path": "pool", "pool": True, "packed": False}, p
        gi, gd = got = g.exact_knn(rows, q, 64, want_dist=True, row_tags=T, query_tags=Q)
    few = np.flatnonzero(Q == 1 << kt.FEW_BIT)
    assert (gi[few][:, 7:] == ku.NONE_ID).all() and np.isinf(gd[few][:, 7:]).all() and (gi[few][:, :7] != ku.NONE_ID).all()
    hu.same(got, hu.knn_of(dist, 64, allowed=(T[None, :] & Q[:, None]) != 0), "padding")
