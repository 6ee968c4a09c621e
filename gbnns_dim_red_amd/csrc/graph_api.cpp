// graph_api.cpp -- graph preparation entry points of the C ABI (include/gbnns.h): gbnns_exact_knn (getTruth, support_func.h:270-290,
// generalised to k results: heaps, the matrix-core filter, long lists as pools), gbnns_exact_knn_bytes (the same lists over uint8 rows,
// their distances from the int8 matrix cores: knn_bytes.hip) with gbnns_debug_knn_bytes_plan / gbnns_debug_knn_plan, their tagged forms gbnns_exact_knn_tagged /
// gbnns_exact_knn_bytes_tagged and gbnns_index_exact_knn over a handle's resident table, and gbnns_build_graph_gd_device (hnswlikeGD,
// support_func.h:521-575, pruning on the device).  Every kNN entry point fills a KnnCall<T> and ends in knn_call (one body for float rows,
// one for byte rows).  What the two bodies share exists once: knn_check (the refusals), KnnStaged (HOST buffers and the
// tag words), KnnSlab (every address that depends on the query slab) and knn_sweep_chunks (the row chunks and the answer to a key list
// that overflowed).  gbnns_index_exact_knn_gather (knn_gather_call: census, schedule, per round the lists' fill and the gathered scan --
// knn_gather.hip) shares the refusals and the staging and falls back to knn_call for a shape its kernel does not cover.  Cut out of api.cpp
// in round 5; api_internal.h lists the other units.

#include "api_internal.h"

using namespace gbnns;
using namespace gbnns_api;

namespace {
// One exact-kNN request, whichever entry point brought it: gbnns_exact_knn / _bytes (untagged, caller's arrays), their _tagged twins, and
// gbnns_index_exact_knn (the table and the row tags are the handle's, resident on the device at the handle's row stride).  T = float / uint8_t.
template <class T>
struct KnnCall {
    int device;
    const T* base;             // [n x bstride]; a buffer of mem_kind, or (resident) device memory whatever mem_kind says
    uint32_t bstride;          // elements between rows
    bool resident;
    uint64_t n;
    const T* queries;          // [n_q x d], mem_kind
    uint64_t n_q;
    uint32_t d;
    int k, metric;
    int64_t self_offset;
    bool tagged;
    const uint32_t* row_tags;  // [n]; where base is
    const uint32_t* query_tags;  // [n_q], mem_kind
    uint32_t* out_ids;
    float* out_dist;
    int mem_kind;
    void* stream;
};

// What a row type does not take, between the checks every call shares and those that need a device (knn_check).
int knn_refuse(const KnnCall<float>& c) {
    if (c.d > 8192) return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn: d <= 8192 (a tile of base rows is staged in LDS; got %u)", c.d);
    if (c.metric == GBNNS_METRIC_NEG_DOT && c.d % 8 != 0)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn: the negative-dot form needs d %% 8 == 0 (got %u)", c.d);
    return GBNNS_OK;
}
int knn_refuse(const KnnCall<uint8_t>& c) {
    if (c.d > 256)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn_bytes: d <= 256 (every sum of the distance must stay an integer below 2^24 to be exact "
                    "in float32 and on the int8 matrix cores; got %u): widen the rows and call gbnns_exact_knn", c.d);
    if (c.k > 4096) return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn_bytes: k <= 4096 (got %d): widen the rows and call gbnns_exact_knn", c.k);
    if (c.metric == GBNNS_METRIC_NEG_DOT && c.d % 8 != 0)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn_bytes: the negative-dot form needs d %% 8 == 0 (got %u)", c.d);
    return GBNNS_OK;
}

// The refusals of a call, in the order tests/test_cabi_cpu.py and tests/test_knn_bytes_cpu.py pin.  (A call without queries is valid
// and done: the caller returns behind this.)
template <class T>
int knn_check(const KnnCall<T>& c) {
    if (!c.base || !c.queries || !c.out_ids || (c.tagged && (!c.row_tags || !c.query_tags))) return fail(GBNNS_ERR_INVALID, "null argument");
    if (c.n == 0 || c.n >= (1ull << 32) - 1) return fail(GBNNS_ERR_INVALID, "n must be in [1, 2^32 - 1)");
    if (c.n_q >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "n_q too large");
    if (c.k < 1 || c.k > (1 << 20)) return fail(GBNNS_ERR_INVALID, "k must be in [1, 2^20]");
    if (c.d == 0) return fail(GBNNS_ERR_INVALID, "d must be >= 1");
    if (c.metric != GBNNS_METRIC_L2 && c.metric != GBNNS_METRIC_NEG_DOT) return fail(GBNNS_ERR_INVALID, "unknown metric %d", c.metric);
    if (c.mem_kind != GBNNS_MEM_HOST && c.mem_kind != GBNNS_MEM_DEVICE) return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", c.mem_kind);
    if (int rc = knn_refuse(c)) return rc;
    if (c.self_offset < -1) return fail(GBNNS_ERR_INVALID, "self_offset must be >= -1");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(GBNNS_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (c.device < 0 || c.device >= count) return fail(GBNNS_ERR_NO_DEVICE, "device %d out of range (%d devices)", c.device, count);
    return GBNNS_OK;
}

// The tag words of a tagged call on the device: the rows' in a copy of its own, 16-byte aligned and 64 words longer than the set (zero
// there) -- the sweep kernels read them in aligned groups of four to the end of a block of 32 rows, as they read bnorm / bterm -- and the
// queries' (uploaded for HOST buffers).
template <class T>
int knn_stage_tags(const KnnCall<T>& c, DevBuf& tag_dev, DevBuf& qtag_dev, const uint32_t*& qtags, hipStream_t s) {
    int rc;
    if ((rc = tag_dev.ensure(((size_t)c.n + 64) * 4))) return rc;
    HIP_TRY(hipMemsetAsync(tag_dev.as<uint32_t>() + c.n, 0, 64 * 4, s));
    const bool host = c.mem_kind == GBNNS_MEM_HOST;
    // (a HOST array never reaches the runtime's copy calls: h2d_staged says why)
    if (host && !c.resident) {
        if ((rc = h2d_staged(tag_dev.p, c.row_tags, (size_t)c.n * 4))) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(tag_dev.p, c.row_tags, (size_t)c.n * 4, hipMemcpyDeviceToDevice, s));
    }
    qtags = c.query_tags;
    if (host) {
        if ((rc = qtag_dev.ensure((size_t)c.n_q * 4))) return rc;
        if ((rc = h2d_staged(qtag_dev.p, c.query_tags, (size_t)c.n_q * 4))) return rc;
        qtags = qtag_dev.as<uint32_t>();
    }
    return GBNNS_OK;
}

// A call's arrays where the kernels read and write them: the caller's own (DEVICE buffers, a resident table), or copies (HOST).
template <class T>
struct KnnStaged {
    ScopedDevBuf b_dev, q_dev, ids_dev, dist_dev, tag_dev, qtag_dev;
    const T* base;
    const T* q;
    uint32_t* ids;
    float* dist;
    const uint32_t* tags = nullptr;   // tagged: the device copies of the tag words; a launch with null tags is the untagged instance
    const uint32_t* qtags = nullptr;

    int stage(const KnnCall<T>& c, hipStream_t s) {
        const size_t nq = c.n_q;
        int rc;
        base = c.base; q = c.queries; ids = c.out_ids; dist = c.out_dist;
        if (c.mem_kind == GBNNS_MEM_HOST) {  // (byte rows are uploaded as bytes: a quarter of the float call's traffic, and no float copy anywhere)
            if (!c.resident) {
                if ((rc = b_dev.ensure((size_t)c.n * c.d * sizeof(T)))) return rc;
                if ((rc = h2d_staged(b_dev.p, c.base, (size_t)c.n * c.d * sizeof(T)))) return rc;
                base = b_dev.as<T>();
            }
            if ((rc = q_dev.ensure(nq * c.d * sizeof(T)))) return rc;
            if ((rc = ids_dev.ensure(nq * c.k * 4))) return rc;
            if (c.out_dist && (rc = dist_dev.ensure(nq * c.k * 4))) return rc;
            if ((rc = h2d_staged(q_dev.p, c.queries, nq * c.d * sizeof(T)))) return rc;
            q = q_dev.as<T>(); ids = ids_dev.as<uint32_t>();
            dist = c.out_dist ? dist_dev.as<float>() : nullptr;
        }
        if (c.tagged) {
            if ((rc = knn_stage_tags(c, tag_dev, qtag_dev, qtags, s))) return rc;
            tags = tag_dev.as<uint32_t>();
        }
        return GBNNS_OK;
    }
    // The lists back to HOST buffers, and the end of the call: its temporaries are released behind this, so it waits for the work that uses them.
    int copy_back(const KnnCall<T>& c, hipStream_t s) const {
        if (c.mem_kind == GBNNS_MEM_HOST) {
            if (int rc = d2h_staged(c.out_ids, ids, (size_t)c.n_q * c.k * 4, s)) return rc;
            if (c.out_dist)
                if (int rc = d2h_staged(c.out_dist, dist, (size_t)c.n_q * c.k * 4, s)) return rc;
        }
        HIP_TRY(hipStreamSynchronize(s));
        return GBNNS_OK;
    }
};

// Queries the pool path of gbnns_exact_knn (keys of 4 bytes) and gbnns_exact_knn_bytes (keys of 8) serve at a time: as many as keep the
// key lists (cap = 4 k + 64 slots a query) within 4 GiB, a multiple of 128, never fewer than 1 024 -- or all of them.  "knn_slab" > 0
// caps that (a multiple of 128, at least 128: tests run several slabs at a few hundred queries); gbnns_debug_knn_slab reports it.
uint32_t knn_slab_queries(uint64_t nq, int k, uint32_t key_bytes) {
    const uint64_t cap = (uint64_t)(4 * k + 64);
    uint64_t slab = std::max<uint64_t>(1024, ((4ull << 30) / (cap * key_bytes)) & ~(uint64_t)127);
    const int knob = g_knob_knn_slab.load(std::memory_order_relaxed);
    if (knob > 0) slab = std::min<uint64_t>(slab, (uint64_t)std::max(128, knob & ~127));
    return (uint32_t)std::min<uint64_t>(nq, slab);
}

// Queries q0 .. q0 + qn of a call: everything a slab reads or writes at an offset of its own.  (The per-slab workspaces -- packed query
// operands, keys, thresholds, counts -- start at 0 in every slab and are set again by the body at the head of its slab loop.)
template <class T>
struct KnnSlab {
    uint32_t q0, qn;
    const T* q;
    int64_t self_offset;    // of the slab's first query, or -1
    const uint32_t* qtags;  // or nullptr
    uint32_t* out_ids;
    float* out_dist;        // or nullptr
};
template <class T>
KnnSlab<T> knn_slab_at(const KnnCall<T>& c, const KnnStaged<T>& st, uint32_t q0, uint32_t slab) {
    KnnSlab<T> sl{};
    sl.q0 = q0; sl.qn = std::min(slab, (uint32_t)c.n_q - q0);
    sl.q = st.q + (size_t)q0 * c.d;
    sl.self_offset = c.self_offset >= 0 ? c.self_offset + (int64_t)q0 : -1;
    sl.qtags = st.qtags ? st.qtags + q0 : nullptr;
    sl.out_ids = st.ids + (size_t)q0 * c.k;
    sl.out_dist = st.dist ? st.dist + (size_t)q0 * c.k : nullptr;
    return sl;
}

// The rows of a set in chunks, for `qn` queries whose thresholds start at "every row passes": sweep(r0, rows) collects what a chunk's rows
// leave in the queries' lists (`count`, and `flag` where a list overflowed), take() offers the lists to the heaps / pools and tightens the
// thresholds.  The first chunk, of first_rows <= cap rows, cannot overflow a list; a later one is at most as long as everything before it
// -- a query is then expected to keep about k rows of it, whatever the chunk -- and at most max_chunk rows.  Where some query kept more
// rows of a chunk than its list holds (rows in an adversarial order, a mass of ties at the threshold) nothing of the chunk has been
// offered yet: the chunk again in pieces of first_rows, which cannot overflow.
template <class Sweep, class Take>
int knn_sweep_chunks(uint64_t n, uint64_t first_rows, uint64_t max_chunk, uint32_t qn, uint32_t* count, uint32_t* flag, hipStream_t s, Sweep sweep,
                     Take take) {
    int rc;
    auto swept = [&](uint64_t r0, uint32_t rows) -> int {
        HIP_TRY(hipMemsetAsync(count, 0, (size_t)qn * 4, s));
        HIP_TRY(hipMemsetAsync(flag, 0, 4, s));
        return sweep(r0, rows);
    };
    uint32_t h_flag = 0;
    for (uint64_t r0 = 0, chunk = 0; r0 < n; r0 += chunk) {
        chunk = r0 == 0 ? first_rows : std::min<uint64_t>(max_chunk, r0);
        const uint32_t rows = (uint32_t)std::min<uint64_t>(chunk, n - r0);
        if ((rc = swept(r0, rows))) return rc;
        if (r0 != 0) {
            HIP_TRY(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (r0 == 0 || !h_flag) {
            if ((rc = take())) return rc;
            continue;
        }
        for (uint64_t r1 = r0; r1 < r0 + rows; r1 += first_rows) {
            if ((rc = swept(r1, (uint32_t)std::min<uint64_t>(first_rows, r0 + rows - r1)))) return rc;
            if ((rc = take())) return rc;
        }
    }
    return GBNNS_OK;
}

// What gbnns_exact_knn does with a shape under the current knobs (gbnns_debug_knn_plan reports it).
struct KnnFloatPlan {
    bool pool;    // the matrix-core filter in front of pools with a radix select (long lists)
    bool filter;  // the matrix-core filter in front of the heaps; neither: the exact scan alone
    uint32_t dp;  // floats of a packed row of the filter: d rounded up to its K step of 16
};
KnnFloatPlan knn_float_plan(uint64_t n, uint64_t nq, uint32_t d, int k, int metric) {
    KnnFloatPlan pl{};
    // Matrix-core filter in front of the exact distances (knn.hip): the L2 metric on rows of whole 16-byte steps, sets
    // large enough to amortise its passes.  Same output, byte for byte (tests/test_gpu_parity.py); "knn_filter" 0 = off.
    const int knob_filter = g_knob_knn_filter.load(std::memory_order_relaxed);  // 0 = never, 1 = by size, 2 = whenever the shape allows (tests)
    const bool filter_shape = metric == GBNNS_METRIC_L2 && d % 4 == 0 && d <= 128 && n > (uint64_t)4 * k &&
                              (knob_filter == 2 || (knob_filter == 1 && n >= (1u << 17) && nq >= 2048));
    // long lists keep a query's keys as an unordered pool instead of a heap (knn.hip, knn_pool_update_kernel)
    pl.pool = filter_shape && k >= g_knob_knn_pool_min_k.load(std::memory_order_relaxed) && k <= 4096;
    pl.filter = filter_shape && k <= 512 && !pl.pool;
    pl.dp = (d + 15u) & ~15u;
    return pl;
}

// The matrix-core filter's operands and lists (knn.hip) for `nq` queries at a time: the heap-filter path's whole call, a slab of the pool path.
struct KnnFilterWork {
    ScopedDevBuf bpack, bnorm, qpack, qnorm, rhs, cand, count, flag;
    uint32_t dp, cap;
    // the buffers, and the base set packed
    int prepare(const KnnParams& p, uint32_t nq, uint32_t dp_, uint32_t cap_, hipStream_t s) {
        int rc;
        dp = dp_; cap = cap_;
        if ((rc = bpack.ensure((size_t)p.n * dp * 4))) return rc;       // 2 dp bf16 per row
        if ((rc = bnorm.ensure(((size_t)p.n + 64) * 4))) return rc;  // (+inf behind the last row: the filter reads whole blocks of 32)
        if ((rc = qpack.ensure((size_t)nq * dp * 4))) return rc;
        if ((rc = qnorm.ensure((size_t)nq * 4))) return rc;
        if ((rc = rhs.ensure((size_t)nq * 4))) return rc;
        if ((rc = cand.ensure((size_t)nq * cap * 4))) return rc;
        if ((rc = count.ensure((size_t)nq * 4))) return rc;
        if ((rc = flag.ensure(4))) return rc;
        HIP_TRY(launch_fill_u32(bnorm.as<uint32_t>() + p.n, 0x7F800000u, 64, s));
        HIP_TRY(launch_knn_pack(p.base, p.bstride, p.dim, p.n, bpack.as<uint16_t>(), bnorm.as<float>(), s));
        return GBNNS_OK;
    }
    // rows r0 .. r0 + rows against the qn queries packed last (tags: the rows' words by row id, qtags: those queries'; or null)
    KnnFilterParams chunk(uint64_t r0, uint32_t rows, uint32_t qn, const uint32_t* tags, const uint32_t* qtags) const {
        KnnFilterParams f{};
        f.qpack = qpack.as<uint16_t>(); f.bpack = bpack.as<uint16_t>() + (size_t)r0 * dp * 2; f.bnorm = bnorm.as<float>() + r0;
        f.rhs = rhs.as<float>(); f.nq = qn; f.dp = dp; f.rows = rows; f.row0 = (uint32_t)r0; f.cap = cap;
        f.cand = cand.as<uint32_t>(); f.count = count.as<uint32_t>(); f.overflow = flag.as<uint32_t>();
        if (qtags) { f.btag = tags + r0; f.qtag = qtags; }
        return f;
    }
};

int knn_call(const KnnCall<float>& c) {
    int rc;
    if ((rc = knn_check(c)) || c.n_q == 0) return rc;
    HIP_TRY(hipSetDevice(c.device));
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    const int k = c.k, metric = c.metric;
    const uint64_t n = c.n;
    const uint32_t d = c.d, nq = (uint32_t)c.n_q;
    KnnStaged<float> st;
    ScopedDevBuf heap;
    if ((rc = st.stage(c, s))) return rc;
    KnnParams p{};
    p.base = st.base; p.q = st.q; p.out_ids = st.ids; p.out_dist = st.dist; p.row_tags = st.tags; p.query_tags = st.qtags;
    p.bstride = c.bstride; p.qstride = d; p.n = n; p.nq = nq; p.dim = d; p.k = k; p.self_offset = c.self_offset;
    p.heap_stride = ((size_t)nq + 63) & ~(size_t)63;
    const KnnFloatPlan pl = knn_float_plan(n, c.n_q, d, k, metric);
    const bool pool_path = pl.pool, filter = pl.filter;
    if (!pool_path) {  // (the pool path keeps its keys in slabs of its own: at k = 1 000 and 10^6 queries the heaps would be 9 GB)
        if ((rc = heap.ensure(p.heap_stride * (size_t)k * 8))) return rc;
        p.heap = heap.as<uint64_t>();
        HIP_TRY(hipMemsetAsync(p.heap, 0xFF, p.heap_stride * (size_t)k * 8, s));
    }
    if (pool_path) {
        const uint32_t cap = (uint32_t)(4 * k + 64);
        const uint64_t rows_first = cap & ~63u;  // a chunk of at most `cap` rows cannot overflow a query's list: the first chunk (no thresholds yet) and the fallback
        // (chunks four times the heap path's: every chunk costs a query a pass over its whole pool; measured at k = 1 000: 32 K rows 1.98 s, 64 K 1.86 s, 128 K 1.89 s)
        const uint64_t max_chunk = std::min<uint64_t>(4ull * (uint64_t)g_knob_knn_chunk.load(std::memory_order_relaxed), std::max<uint64_t>(64, (n / 16 + 63) & ~(uint64_t)63));
        const uint32_t slab = knn_slab_queries(nq, k, 4);  // queries in slabs whose candidate lists take at most 4 GiB
        KnnFilterWork w;
        ScopedDevBuf pool, root;
        if ((rc = pool.ensure((size_t)slab * (size_t)k * 8))) return rc;
        if ((rc = root.ensure((size_t)slab * 8))) return rc;
        if ((rc = w.prepare(p, slab, pl.dp, cap, s))) return rc;
        for (uint32_t q0 = 0; q0 < nq; q0 += slab) {
            const KnnSlab<float> sl = knn_slab_at(c, st, q0, slab);
            KnnPoolParams pp{};
            pp.k = p;
            pp.k.q = sl.q; pp.k.nq = sl.qn; pp.k.out_ids = sl.out_ids; pp.k.out_dist = sl.out_dist;
            pp.k.self_offset = sl.self_offset; pp.k.query_tags = sl.qtags;
            pp.pool = pool.as<uint64_t>(); pp.root = root.as<uint64_t>(); pp.cand = w.cand.as<uint32_t>(); pp.count = w.count.as<uint32_t>();
            pp.cap = cap; pp.qnorm = w.qnorm.as<float>(); pp.rhs = w.rhs.as<float>();
            HIP_TRY(launch_knn_pack(sl.q, d, d, sl.qn, w.qpack.as<uint16_t>(), w.qnorm.as<float>(), s));
            HIP_TRY(hipMemsetAsync(pool.p, 0xFF, (size_t)sl.qn * (size_t)k * 8, s));
            HIP_TRY(hipMemsetAsync(root.p, 0xFF, (size_t)sl.qn * 8, s));
            HIP_TRY(launch_fill_u32(w.rhs.as<uint32_t>(), 0xFF800000u, sl.qn, s));  // -inf: every row passes
            auto sweep = [&](uint64_t r0, uint32_t rows) -> int { HIP_TRY(launch_knn_filter(w.chunk(r0, rows, sl.qn, st.tags, sl.qtags), s)); return GBNNS_OK; };
            auto take = [&]() -> int { HIP_TRY(launch_knn_pool_update(pp, s)); return GBNNS_OK; };
            if ((rc = knn_sweep_chunks(n, rows_first, max_chunk, sl.qn, w.count.as<uint32_t>(), w.flag.as<uint32_t>(), s, sweep, take))) return rc;
            HIP_TRY(launch_knn_pool_finalize(pp, s));
        }
    } else if (filter) {
        const uint32_t cap = (uint32_t)std::max(256, 4 * k + 64);
        // The first rows are scanned exactly (they fill the heaps: thresholds exist afterwards); then filtered chunks, each
        // at most as long as everything before it -- a query is then expected to keep about k rows of a chunk, whatever
        // the chunk -- and at most 32 K rows (4 MB of packed rows at d = 32: L2 / Infinity-Cache resident while swept).
        // Chunks start on multiples of 64 rows (the filter reads the norms in aligned groups of four).
        const uint64_t max_chunk = std::min<uint64_t>((uint64_t)g_knob_knn_chunk.load(std::memory_order_relaxed), std::max<uint64_t>(64, (n / 16 + 63) & ~(uint64_t)63));  // (small sets, tests: a sixteenth)
        const uint64_t first = std::min<uint64_t>(n, (std::max<uint64_t>(std::min<uint64_t>(max_chunk, 8192), 4ull * (uint64_t)k) + 63) & ~(uint64_t)63);
        KnnFilterWork w;
        if ((rc = w.prepare(p, nq, pl.dp, cap, s))) return rc;
        HIP_TRY(launch_knn_pack(p.q, d, d, nq, w.qpack.as<uint16_t>(), w.qnorm.as<float>(), s));
        KnnParams ps = p;          // the first rows: the exact scan, heaps kept
        ps.n = first; ps.row0 = 0; ps.keep_heap = 1;
        HIP_TRY(launch_knn_scan(ps, metric, s));
        HIP_TRY(launch_knn_thresholds(p.heap, p.heap_stride, k, w.qnorm.as<float>(), nq, w.rhs.as<float>(), s));
        uint32_t h_flag = 0;
        for (uint64_t r0 = first, chunk = 0; r0 < n; r0 += chunk) {
            chunk = std::min<uint64_t>(max_chunk, r0);
            const uint32_t rows = (uint32_t)std::min<uint64_t>(chunk, n - r0);
            HIP_TRY(hipMemsetAsync(w.count.p, 0, (size_t)nq * 4, s));
            HIP_TRY(hipMemsetAsync(w.flag.p, 0, 4, s));
            HIP_TRY(launch_knn_filter(w.chunk(r0, rows, nq, st.tags, st.qtags), s));
            HIP_TRY(hipMemcpyAsync(&h_flag, w.flag.p, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (h_flag) {
                // some query kept more rows of this chunk than its list holds (adversarial order of the rows, or thresholds
                // not yet tight): the chunk is scanned exactly for everyone instead -- same heaps, nothing offered twice
                KnnParams pc = p;
                pc.base = p.base + (size_t)r0 * p.bstride; pc.n = rows; pc.row0 = r0; pc.keep_heap = 1;
                HIP_TRY(launch_knn_scan(pc, metric, s));
                HIP_TRY(launch_knn_thresholds(p.heap, p.heap_stride, k, w.qnorm.as<float>(), nq, w.rhs.as<float>(), s));
            } else {
                KnnRescoreParams rp{};
                rp.k = p; rp.cand = w.cand.as<uint32_t>(); rp.count = w.count.as<uint32_t>(); rp.cap = cap;
                rp.qnorm = w.qnorm.as<float>(); rp.rhs = w.rhs.as<float>();
                HIP_TRY(launch_knn_rescore(rp, s));
            }
        }
        HIP_TRY(launch_knn_finalize(p, s));
    } else {
        HIP_TRY(launch_knn_scan(p, metric, s));
    }
    return st.copy_back(c, s);
}

// What gbnns_exact_knn_bytes does with a shape under the current knobs (gbnns_debug_knn_bytes_plan reports it).
struct KnnBytesPlan {
    uint32_t dp;          // row bytes of the packed operands: d rounded up to the K step
    uint32_t cap;         // key slots of a query per chunk
    uint64_t first_rows;  // rows of the first chunk (thresholds at "everything passes") and of a piece of a chunk swept again: <= cap, so no list can overflow
    uint64_t max_chunk;   // most rows of a later chunk
    bool pool;            // lists kept as pools with a radix select, not as heaps
    uint32_t slab;        // queries served at a time: their key lists take at most 4 GiB
};
KnnBytesPlan knn_bytes_plan(uint64_t n, uint64_t nq, uint32_t d, int k) {
    KnnBytesPlan pl{};
    pl.dp = (d + kKnnBytesKStep - 1) / kKnnBytesKStep * kKnnBytesKStep;
    pl.cap = (uint32_t)(4 * k + 64);
    pl.first_rows = std::min<uint64_t>(n, pl.cap & ~63u);  // (chunks start on multiples of 64 rows: the sweep reads the row terms in aligned groups of four)
    pl.max_chunk = 4ull * (uint64_t)g_knob_knn_chunk.load(std::memory_order_relaxed);  // (the knob is a multiple of 64, at least 64)
    pl.pool = k >= g_knob_knn_pool_min_k.load(std::memory_order_relaxed);
    pl.slab = knn_slab_queries(nq, k, 8);
    return pl;
}

int knn_call(const KnnCall<uint8_t>& c) {
    int rc;
    if ((rc = knn_check(c)) || c.n_q == 0) return rc;
    HIP_TRY(hipSetDevice(c.device));
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    const int k = c.k, metric = c.metric;
    const uint64_t n = c.n;
    const uint32_t d = c.d, nq = (uint32_t)c.n_q;
    const KnnBytesPlan pl = knn_bytes_plan(n, c.n_q, d, k);
    const uint32_t dp = pl.dp, cap = pl.cap, slab = pl.slab;
    KnnStaged<uint8_t> st;
    ScopedDevBuf bpack, bterm, qpack, qterm, thr, cand, cnt, flag, keys, root;
    if ((rc = st.stage(c, s))) return rc;
    const size_t heap_stride = ((size_t)slab + 63) & ~(size_t)63;
    if ((rc = bpack.ensure((size_t)n * dp))) return rc;
    if ((rc = bterm.ensure(((size_t)n + 64) * 4))) return rc;  // (the sweep reads whole blocks of 32 rows' terms)
    if ((rc = qpack.ensure((size_t)slab * dp))) return rc;
    if ((rc = qterm.ensure((size_t)slab * 4))) return rc;
    if ((rc = thr.ensure((size_t)slab * 4))) return rc;
    if ((rc = cand.ensure((size_t)slab * cap * 8))) return rc;
    if ((rc = cnt.ensure((size_t)slab * 4))) return rc;
    if ((rc = flag.ensure(4))) return rc;
    if ((rc = keys.ensure(pl.pool ? (size_t)slab * (size_t)k * 8 : heap_stride * (size_t)k * 8))) return rc;
    if (pl.pool && (rc = root.ensure((size_t)slab * 8))) return rc;
    HIP_TRY(hipMemsetAsync(bterm.as<int32_t>() + n, 0, 64 * 4, s));
    HIP_TRY(launch_knn_bytes_pack(st.base, c.bstride, d, dp, metric, 0, n, bpack.as<int8_t>(), bterm.as<int32_t>(), s));
    for (uint32_t q0 = 0; q0 < nq; q0 += slab) {
        const KnnSlab<uint8_t> sl = knn_slab_at(c, st, q0, slab);
        KnnBytesOfferParams op{};
        op.cand = cand.as<uint64_t>(); op.count = cnt.as<uint32_t>(); op.cap = cap; op.nq = sl.qn; op.k = k;
        op.self_offset = sl.self_offset;
        op.qterm = qterm.as<int32_t>(); op.thr = thr.as<int32_t>();
        if (pl.pool) { op.pool = keys.as<uint64_t>(); op.root = root.as<uint64_t>(); }
        else { op.heap = keys.as<uint64_t>(); op.heap_stride = heap_stride; }
        HIP_TRY(launch_knn_bytes_pack(sl.q, d, d, dp, metric, 1, sl.qn, qpack.as<int8_t>(), qterm.as<int32_t>(), s));
        HIP_TRY(hipMemsetAsync(keys.p, 0xFF, pl.pool ? (size_t)sl.qn * (size_t)k * 8 : heap_stride * (size_t)k * 8, s));
        if (pl.pool) HIP_TRY(hipMemsetAsync(root.p, 0xFF, (size_t)sl.qn * 8, s));
        HIP_TRY(launch_fill_u32(thr.as<uint32_t>(), 0x80000000u, sl.qn, s));  // INT32_MIN: every row passes
        auto sweep = [&](uint64_t r0, uint32_t rows) -> int {
            KnnBytesSweepParams f{};
            f.qpack = qpack.as<int8_t>(); f.bpack = bpack.as<int8_t>() + (size_t)r0 * dp; f.bterm = bterm.as<int32_t>() + r0;
            f.qterm = qterm.as<int32_t>(); f.thr = thr.as<int32_t>(); f.nq = sl.qn; f.dp = dp; f.rows = rows; f.row0 = (uint32_t)r0; f.cap = cap;
            f.shift = metric == GBNNS_METRIC_L2 ? 1 : 0;
            f.cand = cand.as<uint64_t>(); f.count = cnt.as<uint32_t>(); f.overflow = flag.as<uint32_t>();
            if (sl.qtags) { f.btag = st.tags + r0; f.qtag = sl.qtags; }
            HIP_TRY(launch_knn_bytes_sweep(f, s));
            return GBNNS_OK;
        };
        auto take = [&]() -> int { HIP_TRY(launch_knn_bytes_offer(op, s)); return GBNNS_OK; };
        if ((rc = knn_sweep_chunks(n, pl.first_rows, pl.max_chunk, sl.qn, cnt.as<uint32_t>(), flag.as<uint32_t>(), s, sweep, take))) return rc;
        if (pl.pool) {
            KnnPoolParams pp{};
            pp.k.nq = sl.qn; pp.k.k = k; pp.k.out_ids = sl.out_ids; pp.k.out_dist = sl.out_dist;
            pp.pool = keys.as<uint64_t>();
            HIP_TRY(launch_knn_pool_finalize(pp, s));
        } else {
            KnnParams kp{};
            kp.nq = sl.qn; kp.k = k; kp.heap = keys.as<uint64_t>(); kp.heap_stride = heap_stride;
            kp.out_ids = sl.out_ids; kp.out_dist = sl.out_dist;
            HIP_TRY(launch_knn_finalize(kp, s));
        }
    }
    return st.copy_back(c, s);
}

template <class T>
KnnCall<T> knn_free_call(int device, const T* base, uint64_t n, const T* queries, uint64_t n_q, uint32_t d, int k, int metric, int64_t self_offset,
                         bool tagged, const uint32_t* row_tags, const uint32_t* query_tags, uint32_t* out_ids, float* out_dist, int mem_kind, void* stream) {
    KnnCall<T> c{};
    c.device = device; c.base = base; c.bstride = d; c.resident = false; c.n = n; c.queries = queries; c.n_q = n_q; c.d = d; c.k = k;
    c.metric = metric; c.self_offset = self_offset; c.tagged = tagged; c.row_tags = row_tags; c.query_tags = query_tags;
    c.out_ids = out_ids; c.out_dist = out_dist; c.mem_kind = mem_kind; c.stream = stream;
    return c;
}

// A request over a handle's resident table (float or byte), read in place at its device row stride; the row tags are the handle's.
template <class T>
KnnCall<T> knn_resident_call(gbnns_index* ix, const T* table, const T* queries, uint64_t n_q, const uint32_t* query_tags, int k, int64_t self_offset,
                             uint32_t* out_ids, float* out_dist, int mem_kind, void* stream) {
    KnnCall<T> c = knn_free_call(ix->device, table, ix->n, queries, n_q, ix->d, k, ix->metric, self_offset, query_tags != nullptr,
                                 ix->tags.as<uint32_t>(), query_tags, out_ids, out_dist, mem_kind, stream);
    c.bstride = ix->d_pad; c.resident = true;
    return c;
}

// gbnns_index_exact_knn behind its own refusals: `table` is the handle's float or byte table, read in place at its device row stride.
template <class T>
int knn_index_call(gbnns_index* ix, const T* table, const T* queries, uint64_t n_q, const uint32_t* query_tags, int k, int64_t self_offset,
                   uint32_t* out_ids, float* out_dist, int mem_kind, void* stream) {
    if (!table) return fail(GBNNS_ERR_INVALID, "gbnns_index_exact_knn: the handle has no original-space table");
    const KnnCall<T> c = knn_resident_call(ix, table, queries, n_q, query_tags, k, self_offset, out_ids, out_dist, mem_kind, stream);
    // (enter_stream: the deferred calls still owed are joined, as by any call without GBNNS_FLAG_DEFER_JOIN, and `stream` waits for the
    // handle's work in flight on another stream -- a gbnns_index_set_tags among it)
    HIP_TRY(hipSetDevice(ix->device));
    int rc;
    if ((rc = enter_stream(ix, static_cast<hipStream_t>(stream)))) return rc;
    rc = knn_call(c);
    if (rc == GBNNS_OK && n_q) ix->in_flight = false;  // (the call returned behind a synchronisation of its stream)
    return rc;
}

// Does the gathered scan (knn_gather.hip) cover a shape?  d <= 128 and lists the heaps take; else the call runs knn_call, the existing scan.
bool gather_serves(int metric, uint32_t d, bool bytes, int k, const char** name, uint32_t* W) {
    uint32_t w = 0;
    const char* nm = knn_gather_kernel_name(metric, d, bytes, &w);
    const bool ok = nm != nullptr && k <= 4096;
    if (name) *name = ok ? nm : nullptr;
    if (W) *W = ok ? w : 0;
    return ok;
}

// The stage times of a gathered call for the handle knob "gather_timing" (tools/exact_gather_timing.py): three events around census, fill and
// scan of a round, read at the round's end -- a diagnostic run serialises its rounds.
struct GatherClock {
    bool on = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double ms[3] = {0, 0, 0};  // census, fill, scan
    ~GatherClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t start(bool want) {
        on = want;
        for (int i = 0; on && i < 3; ++i)
            if (hipError_t e = hipEventCreate(&ev[i])) return e;
        return hipSuccess;
    }
    hipError_t mark(int i, hipStream_t s) { return on ? hipEventRecord(ev[i], s) : hipSuccess; }
    hipError_t take(int from, int stage) {  // ms[stage] += ev[from] .. ev[from + 1]
        if (!on) return hipSuccess;
        float t = 0;
        if (hipError_t e = hipEventSynchronize(ev[from + 1])) return e;
        if (hipError_t e = hipEventElapsedTime(&t, ev[from], ev[from + 1])) return e;
        ms[stage] += t;
        return hipSuccess;
    }
};

// gbnns_index_exact_knn_gather behind its refusals, the stream entered: census -> allowed (and the words) to the host -> gather_schedule ->
// per round the lists' fill and the gathered scan -> the heaps' finalize.  `table`: the handle's float or byte table, read in place.
template <class T>
int knn_gather_call(gbnns_index* ix, const T* table, const T* queries, uint64_t n_q, const uint32_t* query_tags, int k, int64_t self_offset,
                    uint32_t* out_ids, float* out_dist, int mem_kind, hipStream_t s) {
    constexpr bool bytes = sizeof(T) == 1;
    if (!table) return fail(GBNNS_ERR_INVALID, "gbnns_index_exact_knn_gather: the handle has no original-space table");
    const KnnCall<T> c = knn_resident_call(ix, table, queries, n_q, query_tags, k, self_offset, out_ids, out_dist, mem_kind, s);
    int rc;
    if ((rc = knn_check(c)) || n_q == 0) return rc;
    uint32_t W = 0;
    if (!gather_serves(c.metric, c.d, bytes, k, nullptr, &W)) return knn_call(c);  // a shape the gathered kernel does not cover: the same bytes from the scan
    const uint32_t nq = (uint32_t)n_q;
    const uint64_t n = c.n;
    const bool host = mem_kind == GBNNS_MEM_HOST;
    KnnCall<T> cs = c;
    cs.tagged = false;  // (the rows' tag words are read where the handle keeps them: no padded copy)
    KnnStaged<T> st;
    ScopedDevBuf qtag_dev, census, meta, lists, heap;
    if ((rc = st.stage(cs, s))) return rc;
    GatherClock clock;
    HIP_TRY(clock.start(ix->knob.gather_timing != 0));
    std::vector<uint32_t> h_words, h_allowed;
    GatherSchedule sch;
    try {
        h_words.resize(nq);
        h_allowed.resize(nq);
    } catch (...) {
        return fail(GBNNS_ERR_OOM, "host allocation failed");
    }
    // 1. the census
    const uint32_t* qtags = query_tags;
    if (host) {
        std::memcpy(h_words.data(), query_tags, (size_t)nq * 4);
        if ((rc = qtag_dev.ensure((size_t)nq * 4))) return rc;
        if ((rc = h2d_staged(qtag_dev.p, query_tags, (size_t)nq * 4))) return rc;
        qtags = qtag_dev.as<uint32_t>();
    }
    const size_t cws = (tag_census_ws_bytes(nq) + 15) & ~(size_t)15;
    if ((rc = census.ensure(cws + (size_t)nq * 4))) return rc;
    uint32_t* const allowed_dev = reinterpret_cast<uint32_t*>(census.as<char>() + cws);
    HIP_TRY(clock.mark(0, s));
    HIP_TRY(launch_tag_census(ix->tags.as<uint32_t>(), n, qtags, nq, census.p, allowed_dev, nullptr, s));
    HIP_TRY(clock.mark(1, s));
    HIP_TRY(clock.take(0, 0));
    if ((rc = d2h_staged(h_allowed.data(), allowed_dev, (size_t)nq * 4, s))) return rc;
    if (!host && (rc = d2h_staged(h_words.data(), qtags, (size_t)nq * 4, s))) return rc;
    // 2. the schedule
    const uint64_t budget = std::max<uint64_t>((uint64_t)std::max(1, ix->knob.gather_budget), n);
    try {
        gather_schedule(h_words.data(), h_allowed.data(), nq, n, budget, W, sch);
    } catch (...) {
        return fail(GBNNS_ERR_OOM, "host allocation failed");
    }
    const size_t G = sch.groups.size(), NW = sch.wgs.size(), R = sch.round_entries.size();
    // the heaps: all-ones, so that a query nobody scans for comes out as padding
    const size_t heap_stride = ((size_t)nq + 63) & ~(size_t)63;
    if ((rc = heap.ensure(heap_stride * (size_t)k * 8))) return rc;
    HIP_TRY(hipMemsetAsync(heap.p, 0xFF, heap_stride * (size_t)k * 8, s));
    if (G) {
        // the schedule on the device: [order nq][words G][caps G][cursor G] u32, then 8-byte aligned [offs G] u64, [workgroups NW] 6 x u32
        std::vector<uint32_t> h32;
        std::vector<uint64_t> h_offs;
        try {
            h32.reserve((size_t)nq + 3 * G);
            h32.insert(h32.end(), sch.order.begin(), sch.order.end());
            for (const GatherGroup& g : sch.groups) h32.push_back(g.word);
            for (const GatherGroup& g : sch.groups) h32.push_back(g.len);
            h32.resize((size_t)nq + 3 * G, 0u);  // the cursors
            h_offs.reserve(G);
            for (const GatherGroup& g : sch.groups) h_offs.push_back(g.list_off);
        } catch (...) {
            return fail(GBNNS_ERR_OOM, "host allocation failed");
        }
        const size_t b32 = (h32.size() * 4 + 7) & ~(size_t)7, boffs = G * 8, bwg = NW * sizeof(GatherWorkgroup);
        if ((rc = meta.ensure(b32 + boffs + bwg))) return rc;
        if ((rc = h2d_staged(meta.p, h32.data(), h32.size() * 4))) return rc;
        if ((rc = h2d_staged(meta.as<char>() + b32, h_offs.data(), boffs))) return rc;
        if ((rc = h2d_staged(meta.as<char>() + b32 + boffs, sch.wgs.data(), bwg))) return rc;
        const uint32_t* const order_dev = meta.as<uint32_t>();
        const uint32_t *const words_dev = order_dev + nq, *const caps_dev = words_dev + G;
        uint32_t* const cursor_dev = meta.as<uint32_t>() + nq + 2 * G;
        const uint64_t* const offs_dev = reinterpret_cast<const uint64_t*>(meta.as<char>() + b32);
        const GatherWorkgroup* const wgs_dev = reinterpret_cast<const GatherWorkgroup*>(meta.as<char>() + b32 + boffs);
        uint64_t most = 0;
        for (uint64_t e : sch.round_entries) most = std::max(most, e);
        if ((rc = lists.ensure((size_t)most * 4))) return rc;
        // 3. / 4. round by round: the lists, then their scans (one list buffer: a round's fill runs behind the scans of the round before)
        for (size_t r = 0; r < R; ++r) {
            const uint32_t g0 = sch.round_group0[r], g1 = sch.round_group0[r + 1], w0 = sch.round_wg0[r], w1 = sch.round_wg0[r + 1];
            GatherFillParams f{};
            f.tags = ix->tags.as<uint32_t>(); f.n = n; f.words = words_dev + g0; f.caps = caps_dev + g0; f.offs = offs_dev + g0;
            f.groups = g1 - g0; f.cursor = cursor_dev + g0; f.list = lists.as<uint32_t>();
            KnnGatherParams p{};
            if constexpr (bytes) { p.base_b = st.base; p.q_b = st.q; }
            else { p.base = st.base; p.q = st.q; }
            p.bstride = c.bstride; p.qstride = c.d; p.dim = c.d; p.k = k; p.self_offset = self_offset;
            p.heap = heap.as<uint64_t>(); p.heap_stride = heap_stride; p.order = order_dev;
            p.wgs = wgs_dev + w0; p.n_wgs = w1 - w0; p.list = lists.as<uint32_t>();
            HIP_TRY(clock.mark(0, s));
            HIP_TRY(launch_gather_fill(f, s));
            HIP_TRY(clock.mark(1, s));
            HIP_TRY(launch_knn_gather(p, c.metric, s));
            HIP_TRY(clock.mark(2, s));
            HIP_TRY(clock.take(0, 1));
            HIP_TRY(clock.take(1, 2));
        }
    }
    KnnParams kp{};
    kp.nq = nq; kp.k = k; kp.heap = heap.as<uint64_t>(); kp.heap_stride = heap_stride; kp.out_ids = st.ids; kp.out_dist = st.dist;
    HIP_TRY(launch_knn_finalize(kp, s));
    if ((rc = st.copy_back(c, s))) return rc;
    if (clock.on) {
        for (int i = 0; i < 3; ++i) ix->gather_us[i] = (int)std::min(clock.ms[i] * 1000.0 + 0.5, 2e9);
        ix->gather_rounds = (int)R;
    }
    return GBNNS_OK;
}

// gbnns_index_exact_knn's refusals, which are this call's too, in its order
int knn_index_refuse(const char* fn, gbnns_index* ix, const float* queries, const uint8_t* queries_u8, const uint32_t* query_tags) {
    if ((queries != nullptr) == (queries_u8 != nullptr)) return fail(GBNNS_ERR_INVALID, "%s: exactly one of queries / queries_u8", fn);
    if (!ix) return fail(GBNNS_ERR_INVALID, "null argument");
    if (ix->is(RowKind::F16))
        return fail(GBNNS_ERR_UNSUPPORTED, "%s on a half-base handle (gbnns_index_create_half_base): there is no exact scan over the resident binary16 rows; "
                    "widen the table and call gbnns_exact_knn", fn);
    if (queries_u8 && !ix->is(RowKind::U8)) return fail(GBNNS_ERR_INVALID, "%s: queries_u8 needs a byte handle (gbnns_index_create_bytes)", fn);
    if (queries && ix->is(RowKind::U8))
        return fail(GBNNS_ERR_UNSUPPORTED, "%s: float queries on a byte handle: there is no mixed-pair scan (uint8 rows against "
                    "float queries); pass queries_u8, or widen the table and call gbnns_exact_knn", fn);
    if (query_tags && !ix->tags.p) return fail(GBNNS_ERR_INVALID, "%s with query_tags but without gbnns_index_set_tags", fn);
    return GBNNS_OK;
}
}  // namespace

namespace gbnns_api {
int knn_scan_resident(gbnns_index* ix, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags, int k,
                      uint32_t* out_ids, float* out_dist, hipStream_t s) {
    if (queries) return knn_call(knn_resident_call(ix, ix->base_as<float>(), queries, n_q, query_tags, k, -1, out_ids, out_dist, GBNNS_MEM_DEVICE, s));
    return knn_call(knn_resident_call(ix, ix->base_as<uint8_t>(), queries_u8, n_q, query_tags, k, -1, out_ids, out_dist, GBNNS_MEM_DEVICE, s));
}
int knn_gather_resident(gbnns_index* ix, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags, int k,
                        uint32_t* out_ids, float* out_dist, hipStream_t s) {
    if (queries) return knn_gather_call(ix, ix->base_as<float>(), queries, n_q, query_tags, k, -1, out_ids, out_dist, GBNNS_MEM_DEVICE, s);
    return knn_gather_call(ix, ix->base_as<uint8_t>(), queries_u8, n_q, query_tags, k, -1, out_ids, out_dist, GBNNS_MEM_DEVICE, s);
}
}  // namespace gbnns_api

extern "C" {

int gbnns_exact_knn(int device, const float* base, uint64_t n, const float* queries, uint64_t n_q,
                    uint32_t d, int k, int metric, int64_t self_offset, uint32_t* out_ids, float* out_dist,
                    int mem_kind, void* stream) {
    return knn_call(knn_free_call(device, base, n, queries, n_q, d, k, metric, self_offset, false, nullptr, nullptr, out_ids, out_dist, mem_kind, stream));
}

int gbnns_exact_knn_tagged(int device, const float* base, uint64_t n, const float* queries, uint64_t n_q, uint32_t d, int k, int metric,
                           int64_t self_offset, const uint32_t* row_tags, const uint32_t* query_tags, uint32_t* out_ids, float* out_dist,
                           int mem_kind, void* stream) {
    return knn_call(knn_free_call(device, base, n, queries, n_q, d, k, metric, self_offset, true, row_tags, query_tags, out_ids, out_dist, mem_kind, stream));
}

int gbnns_exact_knn_bytes(int device, const uint8_t* base, uint64_t n, const uint8_t* queries, uint64_t n_q,
                          uint32_t d, int k, int metric, int64_t self_offset, uint32_t* out_ids, float* out_dist,
                          int mem_kind, void* stream) {
    return knn_call(knn_free_call(device, base, n, queries, n_q, d, k, metric, self_offset, false, nullptr, nullptr, out_ids, out_dist, mem_kind, stream));
}

int gbnns_exact_knn_bytes_tagged(int device, const uint8_t* base, uint64_t n, const uint8_t* queries, uint64_t n_q, uint32_t d, int k, int metric,
                                 int64_t self_offset, const uint32_t* row_tags, const uint32_t* query_tags, uint32_t* out_ids, float* out_dist,
                                 int mem_kind, void* stream) {
    return knn_call(knn_free_call(device, base, n, queries, n_q, d, k, metric, self_offset, true, row_tags, query_tags, out_ids, out_dist, mem_kind, stream));
}

// The same computation over the handle's own table, read in place at its device row stride (d_pad floats / bytes); the row tags are the
// handle's.  The packed workspace is the call's own: none of the lanes' workspaces is touched.
int gbnns_index_exact_knn(gbnns_index* ix, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags, int k,
                          int64_t self_offset, uint32_t* out_ids, float* out_dist, int mem_kind, void* stream) {
    if (int rc = knn_index_refuse("gbnns_index_exact_knn", ix, queries, queries_u8, query_tags)) return rc;
    if (queries) return knn_index_call(ix, ix->base_as<float>(), queries, n_q, query_tags, k, self_offset, out_ids, out_dist, mem_kind, stream);
    return knn_index_call(ix, ix->base_as<uint8_t>(), queries_u8, n_q, query_tags, k, self_offset, out_ids, out_dist, mem_kind, stream);
}

// The gathered form: the same bytes, from distances to the allowed rows only (knn_gather.hip).  This call's own refusals need no handle and
// come first; then gbnns_index_exact_knn's, in its order.
int gbnns_index_exact_knn_gather(gbnns_index* ix, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags, int k,
                                 int64_t self_offset, uint32_t* out_ids, float* out_dist, int mem_kind, void* stream) {
    if ((queries != nullptr) == (queries_u8 != nullptr))
        return fail(GBNNS_ERR_INVALID, "gbnns_index_exact_knn_gather: exactly one of queries / queries_u8");
    if (!query_tags) return fail(GBNNS_ERR_INVALID, "gbnns_index_exact_knn_gather: query_tags missing (an untagged call has nothing to gather: gbnns_index_exact_knn)");
    if (k < 1 || k > (1 << 20)) return fail(GBNNS_ERR_INVALID, "k must be in [1, 2^20]");
    if (int rc = knn_index_refuse("gbnns_index_exact_knn_gather", ix, queries, queries_u8, query_tags)) return rc;
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    if ((rc = enter_stream(ix, s))) return rc;
    rc = queries ? knn_gather_call(ix, ix->base_as<float>(), queries, n_q, query_tags, k, self_offset, out_ids, out_dist, mem_kind, s)
                 : knn_gather_call(ix, ix->base_as<uint8_t>(), queries_u8, n_q, query_tags, k, self_offset, out_ids, out_dist, mem_kind, s);
    if (rc == GBNNS_OK && n_q) ix->in_flight = false;  // (the call returned behind a synchronisation of its stream)
    return rc;
}

int gbnns_debug_gather_plan(int bytes, int metric, uint32_t d, int k, char* name, uint32_t name_bytes, uint32_t* queries_per_workgroup) {
    if (!name || name_bytes == 0 || !queries_per_workgroup) return fail(GBNNS_ERR_INVALID, "gbnns_debug_gather_plan: null output");
    if ((bytes != 0 && bytes != 1) || (metric != GBNNS_METRIC_L2 && metric != GBNNS_METRIC_NEG_DOT) || d == 0 || k < 1 || k > (1 << 20))
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_gather_plan: not a shape gbnns_index_exact_knn_gather takes");
    if (bytes) {
        KnnCall<uint8_t> c{};
        c.d = d; c.k = k; c.metric = metric;
        if (int rc = knn_refuse(c)) return rc;
    } else {
        KnnCall<float> c{};
        c.d = d; c.k = k; c.metric = metric;
        if (int rc = knn_refuse(c)) return rc;
    }
    const char* kernel = nullptr;
    if (!gather_serves(metric, d, bytes != 0, k, &kernel, queries_per_workgroup))  // the fallback: the tagged instance of the existing scan
        kernel = bytes ? knn_bytes_sweep_kernel_name((d + kKnnBytesKStep - 1) / kKnnBytesKStep * kKnnBytesKStep, true) : knn_scan_kernel_name(metric, d, true);
    if (!kernel) return fail(GBNNS_ERR_INTERNAL, "gbnns_debug_gather_plan: no kernel instance for the plan");
    std::snprintf(name, name_bytes, "%s", kernel);
    return GBNNS_OK;
}

int gbnns_debug_gather_schedule(const uint32_t* words, const uint32_t* allowed, uint64_t n_q, uint64_t n, uint64_t budget, uint32_t W, uint32_t* order,
                                uint32_t* round_of, uint64_t* list_offset_of, uint32_t* n_rounds, uint32_t* n_workgroups) {
    if (!order || !round_of || !list_offset_of || !n_rounds || !n_workgroups || (n_q && (!words || !allowed)))
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_gather_schedule: null argument");
    if (n == 0 || n >= (1ull << 32) - 1 || n_q >= (1ull << 31) || W == 0 || budget == 0)
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_gather_schedule: n in [1, 2^32 - 1), n_q < 2^31, W >= 1, budget >= 1");
    for (uint64_t i = 0; i < n_q; ++i)
        if (allowed[i] > n) return fail(GBNNS_ERR_INVALID, "gbnns_debug_gather_schedule: allowed[%llu] = %u exceeds n", (unsigned long long)i, allowed[i]);
    GatherSchedule sch;
    try {
        gather_schedule(words, allowed, n_q, n, budget, W, sch);
    } catch (...) {
        return fail(GBNNS_ERR_OOM, "host allocation failed");
    }
    for (uint64_t i = 0; i < n_q; ++i) { order[i] = sch.order[i]; round_of[i] = 0xFFFFFFFFu; list_offset_of[i] = 0; }
    for (const GatherGroup& g : sch.groups)
        for (uint32_t e = 0; e < g.q_count; ++e) {
            const uint32_t i = sch.order[g.q_begin + e];
            round_of[i] = g.round;
            list_offset_of[i] = g.list_off;
        }
    *n_rounds = (uint32_t)sch.round_entries.size();
    *n_workgroups = (uint32_t)sch.wgs.size();
    return GBNNS_OK;
}

int gbnns_debug_knn_bytes_plan(uint64_t n, uint64_t n_q, uint32_t d, int k, uint32_t* dp, uint32_t* cap, uint64_t* first_rows,
                               uint64_t* max_chunk, int* pool) {
    if (!dp || !cap || !first_rows || !max_chunk || !pool) return fail(GBNNS_ERR_INVALID, "gbnns_debug_knn_bytes_plan: null output");
    if (n == 0 || n >= (1ull << 32) - 1 || n_q >= (1ull << 31) || d == 0 || d > 256 || k < 1 || k > 4096)
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_knn_bytes_plan: not a shape gbnns_exact_knn_bytes takes");
    const KnnBytesPlan pl = knn_bytes_plan(n, n_q, d, k);
    *dp = pl.dp; *cap = pl.cap; *first_rows = pl.first_rows; *max_chunk = pl.max_chunk; *pool = pl.pool ? 1 : 0;
    return GBNNS_OK;
}

int gbnns_debug_knn_slab(int bytes, uint64_t n_q, int k, uint32_t* slab) {
    if (!slab) return fail(GBNNS_ERR_INVALID, "gbnns_debug_knn_slab: null output");
    if ((bytes != 0 && bytes != 1) || n_q >= (1ull << 31) || k < 1 || k > 4096)
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_knn_slab: not a shape the pool path of gbnns_exact_knn / gbnns_exact_knn_bytes takes");
    *slab = knn_slab_queries(n_q, k, bytes ? 8 : 4);
    return GBNNS_OK;
}

int gbnns_debug_knn_plan(int bytes, int metric, uint64_t n, uint64_t n_q, uint32_t d, int k, int tagged, char* name, uint32_t name_bytes, int* pool) {
    if (!name || name_bytes == 0 || !pool) return fail(GBNNS_ERR_INVALID, "gbnns_debug_knn_plan: null output");
    if ((bytes != 0 && bytes != 1) || (metric != GBNNS_METRIC_L2 && metric != GBNNS_METRIC_NEG_DOT) || n == 0 || n >= (1ull << 32) - 1 ||
        n_q >= (1ull << 31) || d == 0 || k < 1 || k > (1 << 20))
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_knn_plan: not a shape gbnns_exact_knn / gbnns_exact_knn_bytes takes");
    // the plan functions of the two knn_call bodies and the tables their launches read
    const char* kernel;
    if (bytes) {
        KnnCall<uint8_t> c{};
        c.d = d; c.k = k; c.metric = metric;
        if (int rc = knn_refuse(c)) return rc;
        const KnnBytesPlan pl = knn_bytes_plan(n, n_q, d, k);
        kernel = knn_bytes_sweep_kernel_name(pl.dp, tagged != 0);
        *pool = pl.pool ? 1 : 0;
    } else {
        KnnCall<float> c{};
        c.d = d; c.k = k; c.metric = metric;
        if (int rc = knn_refuse(c)) return rc;
        const KnnFloatPlan pl = knn_float_plan(n, n_q, d, k, metric);
        kernel = pl.pool || pl.filter ? knn_filter_kernel_name(pl.dp, tagged != 0) : knn_scan_kernel_name(metric, d, tagged != 0);
        *pool = pl.pool ? 1 : 0;
    }
    if (!kernel) return fail(GBNNS_ERR_INTERNAL, "gbnns_debug_knn_plan: no kernel instance for the plan");
    std::snprintf(name, name_bytes, "%s", kernel);
    return GBNNS_OK;
}

// graph_build.cpp
extern "C" int gbnns_internal_gd_finish(const uint64_t* knn_offsets, const uint32_t* knn_nbrs, const float* ds,
                                        uint64_t n, uint32_t d, int M, int metric, int reverse, int threads,
                                        uint32_t* adj, uint32_t* deg, uint64_t* host_nodes, uint64_t** out_offsets,
                                        uint32_t** out_nbrs);

int gbnns_build_graph_gd_device(int device, const uint64_t* knn_offsets, const uint32_t* knn_nbrs, const float* ds,
                                uint64_t n, uint32_t d, int M, int metric, int reverse, int threads,
                                uint64_t** out_offsets, uint32_t** out_nbrs, uint64_t* out_host_nodes) {
    if (!knn_offsets || !knn_nbrs || !ds || !out_offsets || !out_nbrs || M < 2 || n == 0)
        return fail(GBNNS_ERR_INVALID, "gbnns_build_graph_gd_device: bad argument");
    if (n >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "n must be < 2^31");
    if (metric != GBNNS_METRIC_L2 && metric != GBNNS_METRIC_NEG_DOT) return fail(GBNNS_ERR_INVALID, "unknown metric %d", metric);
    *out_offsets = nullptr;
    *out_nbrs = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(GBNNS_ERR_NO_DEVICE, "no HIP device available (use gbnns_build_graph_gd for the host builder)");
    if (device < 0 || device >= count) return fail(GBNNS_ERR_NO_DEVICE, "device %d out of range (%d devices)", device, count);
    const uint32_t cap = 2u * (uint32_t)M;
    std::vector<uint32_t> adj, deg;
    try {
        adj.resize((size_t)n * cap);
        deg.assign(n, 0xFFFFFFFFu);
    } catch (...) {
        return fail(GBNNS_ERR_OOM, "host allocation failed");
    }
    // shapes the kernel does not take (kept neighbours sit one per lane; the node's vector is staged in LDS) stay
    // on the host entirely -- same result, the host path is the reference's own algorithm
    const bool on_device = M <= 64 && d <= 128;
    if (on_device) {
        HIP_TRY(hipSetDevice(device));
        ScopedDevBuf ds_dev, off_dev, nbr_dev, adj_dev, deg_dev;
        const uint64_t total = knn_offsets[n];
        const uint32_t dpad = round_up(d, 4);
        int rc;
        if ((rc = upload(ds_dev, ds, n, d, dpad, GBNNS_MEM_HOST))) return rc;
        if ((rc = off_dev.ensure((n + 1) * 8))) return rc;
        if ((rc = nbr_dev.ensure(std::max<uint64_t>(total, 1) * 4))) return rc;
        if ((rc = adj_dev.ensure((size_t)n * cap * 4))) return rc;
        if ((rc = deg_dev.ensure((size_t)n * 4))) return rc;
        if (int rc2 = h2d_staged(off_dev.p, knn_offsets, (n + 1) * 8)) return rc2;
        if (int rc2 = h2d_staged(nbr_dev.p, knn_nbrs, total * 4)) return rc2;
        GdParams p{};
        p.ds = ds_dev.as<float>(); p.dstride = dpad; p.dim = d; p.n = (uint32_t)n; p.M = M;
        p.knn_off = off_dev.as<uint64_t>(); p.knn_nbr = nbr_dev.as<uint32_t>();
        p.adj = adj_dev.as<uint32_t>(); p.deg = deg_dev.as<uint32_t>();
        HIP_TRY(launch_gd_prune(p, metric, nullptr));
        if ((rc = d2h_staged(adj.data(), adj_dev.p, (size_t)n * cap * 4, nullptr))) return rc;
        if ((rc = d2h_staged(deg.data(), deg_dev.p, (size_t)n * 4, nullptr))) return rc;
    }
    const int rc = gbnns_internal_gd_finish(knn_offsets, knn_nbrs, ds, n, d, M, metric, reverse, threads, adj.data(),
                                            deg.data(), out_host_nodes, out_offsets, out_nbrs);
    if (rc == GBNNS_ERR_INVALID) return fail(rc, "gbnns_build_graph_gd_device: neighbour id out of range");
    if (rc) return fail(rc, "gbnns_build_graph_gd_device: host allocation failed");
    return GBNNS_OK;
}

}  // extern "C"
