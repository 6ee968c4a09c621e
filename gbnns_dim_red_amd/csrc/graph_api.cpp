// graph_api.cpp -- graph preparation entry points of the C ABI (include/gbnns.h): gbnns_exact_knn (getTruth, support_func.h:270-290,
// generalised to k results: heaps, the matrix-core filter, long lists as pools), gbnns_exact_knn_bytes (the same lists over uint8 rows,
// their distances from the int8 matrix cores: knn_bytes.hip) with gbnns_debug_knn_bytes_plan, their tagged forms gbnns_exact_knn_tagged /
// gbnns_exact_knn_bytes_tagged and gbnns_index_exact_knn over a handle's resident table (one body each for float and byte rows, whichever
// entry point brought the call), and gbnns_build_graph_gd_device (hnswlikeGD,
// support_func.h:521-575, pruning on the device).  Cut out of api.cpp in round 5; api_internal.h lists the other units.

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

// The tag words of a tagged call on the device: the rows' in a copy of its own, 16-byte aligned and 64 words longer than the set (zero
// there) -- the sweep kernels read them in aligned groups of four to the end of a block of 32 rows, as they read bnorm / bterm -- and the
// queries' (uploaded for HOST buffers).
template <class T>
int knn_stage_tags(const KnnCall<T>& c, DevBuf& tag_dev, DevBuf& qtag_dev, const uint32_t*& qtags, hipStream_t s) {
    int rc;
    if ((rc = tag_dev.ensure(((size_t)c.n + 64) * 4))) return rc;
    HIP_TRY(hipMemsetAsync(tag_dev.as<uint32_t>() + c.n, 0, 64 * 4, s));
    const bool host = c.mem_kind == GBNNS_MEM_HOST;
    HIP_TRY(hipMemcpyAsync(tag_dev.p, c.row_tags, (size_t)c.n * 4, host && !c.resident ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    qtags = c.query_tags;
    if (host) {
        if ((rc = qtag_dev.ensure((size_t)c.n_q * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(qtag_dev.p, c.query_tags, (size_t)c.n_q * 4, hipMemcpyHostToDevice, s));
        qtags = qtag_dev.as<uint32_t>();
    }
    return GBNNS_OK;
}

// Queries the pool path of gbnns_exact_knn (keys of 4 bytes) and gbnns_exact_knn_bytes (keys of 8) serve at a time: as many as keep the
// key lists (cap = 4 k + 64 slots a query) within 4 GiB, a multiple of 128, never fewer than 1 024 -- or all of them.  "knn_slab" > 0
// caps that (a multiple of 128, at least 128: tests run several slabs at a few hundred queries); gbnns_debug_knn_slab reports it.
uint32_t knn_slab(uint64_t nq, int k, uint32_t key_bytes) {
    const uint64_t cap = (uint64_t)(4 * k + 64);
    uint64_t slab = std::max<uint64_t>(1024, ((4ull << 30) / (cap * key_bytes)) & ~(uint64_t)127);
    const int knob = g_knob_knn_slab.load(std::memory_order_relaxed);
    if (knob > 0) slab = std::min<uint64_t>(slab, (uint64_t)std::max(128, knob & ~127));
    return (uint32_t)std::min<uint64_t>(nq, slab);
}

int knn_float_call(const KnnCall<float>& c) {
    const int device = c.device, k = c.k, metric = c.metric, mem_kind = c.mem_kind;
    const float* const base = c.base;
    const float* const queries = c.queries;
    const uint64_t n = c.n, n_q = c.n_q;
    const uint32_t d = c.d;
    const int64_t self_offset = c.self_offset;
    uint32_t* const out_ids = c.out_ids;
    float* const out_dist = c.out_dist;
    void* const stream = c.stream;
    if (!base || !queries || !out_ids || (c.tagged && (!c.row_tags || !c.query_tags))) return fail(GBNNS_ERR_INVALID, "null argument");
    if (n == 0 || n >= (1ull << 32) - 1) return fail(GBNNS_ERR_INVALID, "n must be in [1, 2^32 - 1)");
    if (n_q >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "n_q too large");
    if (k < 1 || k > (1 << 20)) return fail(GBNNS_ERR_INVALID, "k must be in [1, 2^20]");
    if (d == 0) return fail(GBNNS_ERR_INVALID, "d must be >= 1");
    if (metric != GBNNS_METRIC_L2 && metric != GBNNS_METRIC_NEG_DOT) return fail(GBNNS_ERR_INVALID, "unknown metric %d", metric);
    if (mem_kind != GBNNS_MEM_HOST && mem_kind != GBNNS_MEM_DEVICE) return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", mem_kind);
    if (d > 8192) return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn: d <= 8192 (a tile of base rows is staged in LDS; got %u)", d);
    if (metric == GBNNS_METRIC_NEG_DOT && d % 8 != 0)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn: the negative-dot form needs d %% 8 == 0 (got %u)", d);
    if (self_offset < -1) return fail(GBNNS_ERR_INVALID, "self_offset must be >= -1");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(GBNNS_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(GBNNS_ERR_NO_DEVICE, "device %d out of range (%d devices)", device, count);
    if (n_q == 0) return GBNNS_OK;
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool host = mem_kind == GBNNS_MEM_HOST;
    const uint32_t nq = (uint32_t)n_q;
    DevBuf b_dev, q_dev, ids_dev, dist_dev, heap, tag_dev, qtag_dev;
    struct Release {  // DevBuf has no destructor (index members are released by gbnns_index_destroy)
        DevBuf* b[7];
        ~Release() { for (DevBuf* x : b) x->release(); }
    } release{{&b_dev, &q_dev, &ids_dev, &dist_dev, &heap, &tag_dev, &qtag_dev}};
    int rc;
    KnnParams p{};
    p.base = base; p.q = queries; p.out_ids = out_ids; p.out_dist = out_dist;
    if (host) {
        if (!c.resident) {
            if ((rc = b_dev.ensure((size_t)n * d * 4))) return rc;
            HIP_TRY(hipMemcpyAsync(b_dev.p, base, (size_t)n * d * 4, hipMemcpyHostToDevice, s));
            p.base = b_dev.as<float>();
        }
        if ((rc = q_dev.ensure((size_t)nq * d * 4))) return rc;
        if ((rc = ids_dev.ensure((size_t)nq * k * 4))) return rc;
        if (out_dist && (rc = dist_dev.ensure((size_t)nq * k * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(q_dev.p, queries, (size_t)nq * d * 4, hipMemcpyHostToDevice, s));
        p.q = q_dev.as<float>(); p.out_ids = ids_dev.as<uint32_t>();
        p.out_dist = out_dist ? dist_dev.as<float>() : nullptr;
    }
    const uint32_t* qtags = nullptr;  // tagged: the device copies of the tag words; a launch with null tags is the untagged instance
    if (c.tagged) {
        if ((rc = knn_stage_tags(c, tag_dev, qtag_dev, qtags, s))) return rc;
        p.row_tags = tag_dev.as<uint32_t>(); p.query_tags = qtags;
    }
    const uint32_t* const tags = tag_dev.as<uint32_t>();
    p.bstride = c.bstride; p.qstride = d; p.n = n; p.nq = nq; p.dim = d; p.k = k; p.self_offset = self_offset;
    p.heap_stride = ((size_t)nq + 63) & ~(size_t)63;
    // Matrix-core filter in front of the exact distances (knn.hip): the L2 metric on rows of whole 16-byte steps, sets
    // large enough to amortise its passes.  Same output, byte for byte (tests/test_gpu_parity.py); "knn_filter" 0 = off.
    const int knob_filter = g_knob_knn_filter.load(std::memory_order_relaxed);  // 0 = never, 1 = by size, 2 = whenever the shape allows (tests)
    const bool filter_shape = metric == GBNNS_METRIC_L2 && d % 4 == 0 && d <= 128 && n > (uint64_t)4 * k &&
                              (knob_filter == 2 || (knob_filter == 1 && n >= (1u << 17) && nq >= 2048));
    // long lists keep a query's keys as an unordered pool instead of a heap (knn.hip, knn_pool_update_kernel)
    const bool pool_path = filter_shape && k >= g_knob_knn_pool_min_k.load(std::memory_order_relaxed) && k <= 4096;
    const bool filter = filter_shape && k <= 512 && !pool_path;
    if (!pool_path) {  // (the pool path keeps its keys in slabs of its own: at k = 1 000 and 10^6 queries the heaps would be 9 GB)
        if ((rc = heap.ensure(p.heap_stride * (size_t)k * 8))) return rc;
        p.heap = heap.as<uint64_t>();
        HIP_TRY(hipMemsetAsync(p.heap, 0xFF, p.heap_stride * (size_t)k * 8, s));
    }
    if (pool_path) {
        const uint32_t dp = (d + 15u) & ~15u;
        const uint32_t cap = (uint32_t)(4 * k + 64);
        const uint64_t rows_first = cap & ~63u;  // a chunk of at most `cap` rows cannot overflow a query's list: the first chunk (no thresholds yet) and the fallback
        // (chunks four times the heap path's: every chunk costs a query a pass over its whole pool; measured at k = 1 000: 32 K rows 1.98 s, 64 K 1.86 s, 128 K 1.89 s)
        const uint64_t max_chunk = std::min<uint64_t>(4ull * (uint64_t)g_knob_knn_chunk.load(std::memory_order_relaxed), std::max<uint64_t>(64, (n / 16 + 63) & ~(uint64_t)63));
        const uint32_t slab = knn_slab(nq, k, 4);  // queries in slabs whose candidate lists take at most 4 GiB
        DevBuf bpack, bnorm, qpack, qnorm, rhs, cand, count, flag, pool, root;
        struct Release3 {
            DevBuf* b[10];
            ~Release3() { for (DevBuf* x : b) x->release(); }
        } release3{{&bpack, &bnorm, &qpack, &qnorm, &rhs, &cand, &count, &flag, &pool, &root}};
        if ((rc = bpack.ensure((size_t)n * dp * 4))) return rc;
        if ((rc = bnorm.ensure(((size_t)n + 64) * 4))) return rc;
        if ((rc = qpack.ensure((size_t)slab * dp * 4))) return rc;
        if ((rc = qnorm.ensure((size_t)slab * 4))) return rc;
        if ((rc = rhs.ensure((size_t)slab * 4))) return rc;
        if ((rc = cand.ensure((size_t)slab * cap * 4))) return rc;
        if ((rc = count.ensure((size_t)slab * 4))) return rc;
        if ((rc = flag.ensure(4))) return rc;
        if ((rc = pool.ensure((size_t)slab * (size_t)k * 8))) return rc;
        if ((rc = root.ensure((size_t)slab * 8))) return rc;
        HIP_TRY(launch_fill_u32(bnorm.as<uint32_t>() + n, 0x7F800000u, 64, s));
        HIP_TRY(launch_knn_pack(p.base, p.bstride, d, n, bpack.as<uint16_t>(), bnorm.as<float>(), s));
        for (uint32_t q0 = 0; q0 < nq; q0 += slab) {
            const uint32_t qn = std::min(slab, nq - q0);
            KnnPoolParams pp{};
            pp.k = p;
            pp.k.q = p.q + (size_t)q0 * d; pp.k.nq = qn; pp.k.out_ids = p.out_ids + (size_t)q0 * k;
            pp.k.out_dist = p.out_dist ? p.out_dist + (size_t)q0 * k : nullptr;
            pp.k.self_offset = self_offset >= 0 ? self_offset + (int64_t)q0 : -1;
            if (qtags) pp.k.query_tags = qtags + q0;
            pp.pool = pool.as<uint64_t>(); pp.root = root.as<uint64_t>(); pp.cand = cand.as<uint32_t>(); pp.count = count.as<uint32_t>();
            pp.cap = cap; pp.qnorm = qnorm.as<float>(); pp.rhs = rhs.as<float>();
            HIP_TRY(launch_knn_pack(pp.k.q, d, d, qn, qpack.as<uint16_t>(), qnorm.as<float>(), s));
            HIP_TRY(hipMemsetAsync(pool.p, 0xFF, (size_t)qn * (size_t)k * 8, s));
            HIP_TRY(hipMemsetAsync(root.p, 0xFF, (size_t)qn * 8, s));
            HIP_TRY(launch_fill_u32(rhs.as<uint32_t>(), 0xFF800000u, qn, s));  // -inf: every row passes
            uint32_t h_flag = 0;
            auto filter_rows = [&](uint64_t r0, uint32_t rows) -> int {
                HIP_TRY(hipMemsetAsync(count.p, 0, (size_t)qn * 4, s));
                HIP_TRY(hipMemsetAsync(flag.p, 0, 4, s));
                KnnFilterParams f{};
                f.qpack = qpack.as<uint16_t>(); f.bpack = bpack.as<uint16_t>() + (size_t)r0 * dp * 2; f.bnorm = bnorm.as<float>() + r0;
                f.rhs = rhs.as<float>(); f.nq = qn; f.dp = dp; f.rows = rows; f.row0 = (uint32_t)r0; f.cap = cap;
                f.cand = cand.as<uint32_t>(); f.count = count.as<uint32_t>(); f.overflow = flag.as<uint32_t>();
                if (qtags) { f.btag = tags + r0; f.qtag = qtags + q0; }
                HIP_TRY(launch_knn_filter(f, s));
                return GBNNS_OK;
            };
            for (uint64_t r0 = 0, chunk = 0; r0 < n; r0 += chunk) {
                chunk = r0 == 0 ? std::min<uint64_t>(n, rows_first) : std::min<uint64_t>(max_chunk, r0);
                const uint32_t rows = (uint32_t)std::min<uint64_t>(chunk, n - r0);
                if ((rc = filter_rows(r0, rows))) return rc;
                HIP_TRY(hipMemcpyAsync(&h_flag, flag.p, 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                if (!h_flag) {
                    HIP_TRY(launch_knn_pool_update(pp, s));
                    continue;
                }
                // some query kept more rows of this chunk than its list holds: the chunk again in pieces that cannot overflow
                for (uint64_t r1 = r0; r1 < r0 + rows; r1 += rows_first) {
                    if ((rc = filter_rows(r1, (uint32_t)std::min<uint64_t>(rows_first, r0 + rows - r1)))) return rc;
                    HIP_TRY(launch_knn_pool_update(pp, s));
                }
            }
            HIP_TRY(launch_knn_pool_finalize(pp, s));
        }
    } else if (filter) {
        const uint32_t dp = (d + 15u) & ~15u;
        const uint32_t cap = (uint32_t)std::max(256, 4 * k + 64);
        // The first rows are scanned exactly (they fill the heaps: thresholds exist afterwards); then filtered chunks, each
        // at most as long as everything before it -- a query is then expected to keep about k rows of a chunk, whatever
        // the chunk -- and at most 32 K rows (4 MB of packed rows at d = 32: L2 / Infinity-Cache resident while swept).
        // Chunks start on multiples of 64 rows (the filter reads the norms in aligned groups of four).
        const uint64_t max_chunk = std::min<uint64_t>((uint64_t)g_knob_knn_chunk.load(std::memory_order_relaxed), std::max<uint64_t>(64, (n / 16 + 63) & ~(uint64_t)63));  // (small sets, tests: a sixteenth)
        const uint64_t first = std::min<uint64_t>(n, (std::max<uint64_t>(std::min<uint64_t>(max_chunk, 8192), 4ull * (uint64_t)k) + 63) & ~(uint64_t)63);
        DevBuf bpack, bnorm, qpack, qnorm, rhs, cand, count, flag;
        struct Release2 {
            DevBuf* b[8];
            ~Release2() { for (DevBuf* x : b) x->release(); }
        } release2{{&bpack, &bnorm, &qpack, &qnorm, &rhs, &cand, &count, &flag}};
        if ((rc = bpack.ensure((size_t)n * dp * 4))) return rc;       // 2 dp bf16 per row
        if ((rc = bnorm.ensure(((size_t)n + 64) * 4))) return rc;  // (+inf behind the last row: the filter reads whole blocks of 32)
        if ((rc = qpack.ensure((size_t)nq * dp * 4))) return rc;
        if ((rc = qnorm.ensure((size_t)nq * 4))) return rc;
        if ((rc = rhs.ensure((size_t)nq * 4))) return rc;
        if ((rc = cand.ensure((size_t)nq * cap * 4))) return rc;
        if ((rc = count.ensure((size_t)nq * 4))) return rc;
        if ((rc = flag.ensure(4))) return rc;
        HIP_TRY(launch_fill_u32(bnorm.as<uint32_t>() + n, 0x7F800000u, 64, s));
        HIP_TRY(launch_knn_pack(p.base, p.bstride, d, n, bpack.as<uint16_t>(), bnorm.as<float>(), s));
        HIP_TRY(launch_knn_pack(p.q, d, d, nq, qpack.as<uint16_t>(), qnorm.as<float>(), s));
        KnnParams ps = p;          // the first rows: the exact scan, heaps kept
        ps.n = first; ps.row0 = 0; ps.keep_heap = 1;
        HIP_TRY(launch_knn_scan(ps, metric, s));
        HIP_TRY(launch_knn_thresholds(p.heap, p.heap_stride, k, qnorm.as<float>(), nq, rhs.as<float>(), s));
        uint32_t h_flag = 0;
        for (uint64_t r0 = first, chunk = 0; r0 < n; r0 += chunk) {
            chunk = std::min<uint64_t>(max_chunk, r0);
            const uint32_t rows = (uint32_t)std::min<uint64_t>(chunk, n - r0);
            HIP_TRY(hipMemsetAsync(count.p, 0, (size_t)nq * 4, s));
            HIP_TRY(hipMemsetAsync(flag.p, 0, 4, s));
            KnnFilterParams f{};
            f.qpack = qpack.as<uint16_t>(); f.bpack = bpack.as<uint16_t>() + (size_t)r0 * dp * 2; f.bnorm = bnorm.as<float>() + r0;
            f.rhs = rhs.as<float>(); f.nq = nq; f.dp = dp; f.rows = rows; f.row0 = (uint32_t)r0; f.cap = cap;
            f.cand = cand.as<uint32_t>(); f.count = count.as<uint32_t>(); f.overflow = flag.as<uint32_t>();
            if (qtags) { f.btag = tags + r0; f.qtag = qtags; }
            HIP_TRY(launch_knn_filter(f, s));
            HIP_TRY(hipMemcpyAsync(&h_flag, flag.p, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (h_flag) {
                // some query kept more rows of this chunk than its list holds (adversarial order of the rows, or thresholds
                // not yet tight): the chunk is scanned exactly for everyone instead -- same heaps, nothing offered twice
                KnnParams pc = p;
                pc.base = p.base + (size_t)r0 * p.bstride; pc.n = rows; pc.row0 = r0; pc.keep_heap = 1;
                HIP_TRY(launch_knn_scan(pc, metric, s));
                HIP_TRY(launch_knn_thresholds(p.heap, p.heap_stride, k, qnorm.as<float>(), nq, rhs.as<float>(), s));
            } else {
                KnnRescoreParams rp{};
                rp.k = p; rp.cand = cand.as<uint32_t>(); rp.count = count.as<uint32_t>(); rp.cap = cap;
                rp.qnorm = qnorm.as<float>(); rp.rhs = rhs.as<float>();
                HIP_TRY(launch_knn_rescore(rp, s));
            }
        }
        HIP_TRY(launch_knn_finalize(p, s));
    } else {
        HIP_TRY(launch_knn_scan(p, metric, s));
    }
    if (host) {
        HIP_TRY(hipMemcpyAsync(out_ids, p.out_ids, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
        if (out_dist) HIP_TRY(hipMemcpyAsync(out_dist, p.out_dist, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    }
    // the temporaries are released below: wait for the work that uses them
    HIP_TRY(hipStreamSynchronize(s));
    return GBNNS_OK;
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
    pl.slab = knn_slab(nq, k, 8);
    return pl;
}

int knn_bytes_call(const KnnCall<uint8_t>& c) {
    const int device = c.device, k = c.k, metric = c.metric, mem_kind = c.mem_kind;
    const uint8_t* const base = c.base;
    const uint8_t* const queries = c.queries;
    const uint64_t n = c.n, n_q = c.n_q;
    const uint32_t d = c.d;
    const int64_t self_offset = c.self_offset;
    uint32_t* const out_ids = c.out_ids;
    float* const out_dist = c.out_dist;
    void* const stream = c.stream;
    if (!base || !queries || !out_ids || (c.tagged && (!c.row_tags || !c.query_tags))) return fail(GBNNS_ERR_INVALID, "null argument");
    if (n == 0 || n >= (1ull << 32) - 1) return fail(GBNNS_ERR_INVALID, "n must be in [1, 2^32 - 1)");
    if (n_q >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "n_q too large");
    if (k < 1 || k > (1 << 20)) return fail(GBNNS_ERR_INVALID, "k must be in [1, 2^20]");
    if (d == 0) return fail(GBNNS_ERR_INVALID, "d must be >= 1");
    if (metric != GBNNS_METRIC_L2 && metric != GBNNS_METRIC_NEG_DOT) return fail(GBNNS_ERR_INVALID, "unknown metric %d", metric);
    if (mem_kind != GBNNS_MEM_HOST && mem_kind != GBNNS_MEM_DEVICE) return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", mem_kind);
    if (d > 256)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn_bytes: d <= 256 (every sum of the distance must stay an integer below 2^24 to be exact "
                    "in float32 and on the int8 matrix cores; got %u): widen the rows and call gbnns_exact_knn", d);
    if (k > 4096) return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn_bytes: k <= 4096 (got %d): widen the rows and call gbnns_exact_knn", k);
    if (metric == GBNNS_METRIC_NEG_DOT && d % 8 != 0)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_exact_knn_bytes: the negative-dot form needs d %% 8 == 0 (got %u)", d);
    if (self_offset < -1) return fail(GBNNS_ERR_INVALID, "self_offset must be >= -1");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(GBNNS_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(GBNNS_ERR_NO_DEVICE, "device %d out of range (%d devices)", device, count);
    if (n_q == 0) return GBNNS_OK;
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool host = mem_kind == GBNNS_MEM_HOST;
    const uint32_t nq = (uint32_t)n_q;
    const KnnBytesPlan pl = knn_bytes_plan(n, n_q, d, k);
    const uint32_t dp = pl.dp, cap = pl.cap, slab = pl.slab;
    DevBuf b_dev, q_dev, ids_dev, dist_dev, bpack, bterm, qpack, qterm, thr, cand, cnt, flag, keys, root, tag_dev, qtag_dev;
    struct Release {  // DevBuf has no destructor (index members are released by gbnns_index_destroy)
        DevBuf* b[16];
        ~Release() { for (DevBuf* x : b) x->release(); }
    } release{{&b_dev, &q_dev, &ids_dev, &dist_dev, &bpack, &bterm, &qpack, &qterm, &thr, &cand, &cnt, &flag, &keys, &root, &tag_dev, &qtag_dev}};
    int rc;
    const uint8_t* base_d = base;
    const uint8_t* q_d = queries;
    uint32_t* ids_d = out_ids;
    float* dist_d = out_dist;
    if (host) {  // uploaded as bytes: a quarter of the float call's traffic, and no float copy anywhere
        if (!c.resident) {
            if ((rc = b_dev.ensure((size_t)n * d))) return rc;
            HIP_TRY(hipMemcpyAsync(b_dev.p, base, (size_t)n * d, hipMemcpyHostToDevice, s));
            base_d = b_dev.as<uint8_t>();
        }
        if ((rc = q_dev.ensure((size_t)nq * d))) return rc;
        if ((rc = ids_dev.ensure((size_t)nq * k * 4))) return rc;
        if (out_dist && (rc = dist_dev.ensure((size_t)nq * k * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(q_dev.p, queries, (size_t)nq * d, hipMemcpyHostToDevice, s));
        q_d = q_dev.as<uint8_t>(); ids_d = ids_dev.as<uint32_t>();
        dist_d = out_dist ? dist_dev.as<float>() : nullptr;
    }
    const uint32_t* qtags = nullptr;  // tagged: the device copies of the tag words; a sweep with null tags is the untagged instance
    if (c.tagged && (rc = knn_stage_tags(c, tag_dev, qtag_dev, qtags, s))) return rc;
    const uint32_t* const tags = tag_dev.as<uint32_t>();
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
    HIP_TRY(launch_knn_bytes_pack(base_d, c.bstride, d, dp, metric, 0, n, bpack.as<int8_t>(), bterm.as<int32_t>(), s));
    for (uint32_t q0 = 0; q0 < nq; q0 += slab) {
        const uint32_t qn = std::min(slab, nq - q0);
        KnnBytesOfferParams op{};
        op.cand = cand.as<uint64_t>(); op.count = cnt.as<uint32_t>(); op.cap = cap; op.nq = qn; op.k = k;
        op.self_offset = self_offset >= 0 ? self_offset + (int64_t)q0 : -1;
        op.qterm = qterm.as<int32_t>(); op.thr = thr.as<int32_t>();
        if (pl.pool) { op.pool = keys.as<uint64_t>(); op.root = root.as<uint64_t>(); }
        else { op.heap = keys.as<uint64_t>(); op.heap_stride = heap_stride; }
        HIP_TRY(launch_knn_bytes_pack(q_d + (size_t)q0 * d, d, d, dp, metric, 1, qn, qpack.as<int8_t>(), qterm.as<int32_t>(), s));
        HIP_TRY(hipMemsetAsync(keys.p, 0xFF, pl.pool ? (size_t)qn * (size_t)k * 8 : heap_stride * (size_t)k * 8, s));
        if (pl.pool) HIP_TRY(hipMemsetAsync(root.p, 0xFF, (size_t)qn * 8, s));
        HIP_TRY(launch_fill_u32(thr.as<uint32_t>(), 0x80000000u, qn, s));  // INT32_MIN: every row passes
        uint32_t h_flag = 0;
        auto sweep_rows = [&](uint64_t r0, uint32_t rows) -> int {
            HIP_TRY(hipMemsetAsync(cnt.p, 0, (size_t)qn * 4, s));
            HIP_TRY(hipMemsetAsync(flag.p, 0, 4, s));
            KnnBytesSweepParams f{};
            f.qpack = qpack.as<int8_t>(); f.bpack = bpack.as<int8_t>() + (size_t)r0 * dp; f.bterm = bterm.as<int32_t>() + r0;
            f.qterm = qterm.as<int32_t>(); f.thr = thr.as<int32_t>(); f.nq = qn; f.dp = dp; f.rows = rows; f.row0 = (uint32_t)r0; f.cap = cap;
            f.shift = metric == GBNNS_METRIC_L2 ? 1 : 0;
            f.cand = cand.as<uint64_t>(); f.count = cnt.as<uint32_t>(); f.overflow = flag.as<uint32_t>();
            if (qtags) { f.btag = tags + r0; f.qtag = qtags + q0; }
            HIP_TRY(launch_knn_bytes_sweep(f, s));
            return GBNNS_OK;
        };
        // the first chunk cannot overflow a list; a later one is at most as long as everything before it -- a query is then
        // expected to keep about k rows of it, whatever the chunk -- and at most max_chunk rows
        for (uint64_t r0 = 0, chunk = 0; r0 < n; r0 += chunk) {
            chunk = r0 == 0 ? pl.first_rows : std::min<uint64_t>(pl.max_chunk, r0);
            const uint32_t rows = (uint32_t)std::min<uint64_t>(chunk, n - r0);
            if ((rc = sweep_rows(r0, rows))) return rc;
            if (r0 != 0) {
                HIP_TRY(hipMemcpyAsync(&h_flag, flag.p, 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
            }
            if (r0 == 0 || !h_flag) {
                HIP_TRY(launch_knn_bytes_offer(op, s));
                continue;
            }
            // some query kept more rows of this chunk than its list holds (rows in an adversarial order, a mass of ties at the
            // threshold): nothing of the chunk has been offered yet; the chunk again in pieces that cannot overflow
            for (uint64_t r1 = r0; r1 < r0 + rows; r1 += pl.first_rows) {
                if ((rc = sweep_rows(r1, (uint32_t)std::min<uint64_t>(pl.first_rows, r0 + rows - r1)))) return rc;
                HIP_TRY(launch_knn_bytes_offer(op, s));
            }
        }
        if (pl.pool) {
            KnnPoolParams pp{};
            pp.k.nq = qn; pp.k.k = k; pp.k.out_ids = ids_d + (size_t)q0 * k; pp.k.out_dist = dist_d ? dist_d + (size_t)q0 * k : nullptr;
            pp.pool = keys.as<uint64_t>();
            HIP_TRY(launch_knn_pool_finalize(pp, s));
        } else {
            KnnParams kp{};
            kp.nq = qn; kp.k = k; kp.heap = keys.as<uint64_t>(); kp.heap_stride = heap_stride;
            kp.out_ids = ids_d + (size_t)q0 * k; kp.out_dist = dist_d ? dist_d + (size_t)q0 * k : nullptr;
            HIP_TRY(launch_knn_finalize(kp, s));
        }
    }
    if (host) {
        HIP_TRY(hipMemcpyAsync(out_ids, ids_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
        if (out_dist) HIP_TRY(hipMemcpyAsync(out_dist, dist_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    }
    // the temporaries are released below: wait for the work that uses them
    HIP_TRY(hipStreamSynchronize(s));
    return GBNNS_OK;
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
}  // namespace

extern "C" {

int gbnns_exact_knn(int device, const float* base, uint64_t n, const float* queries, uint64_t n_q,
                    uint32_t d, int k, int metric, int64_t self_offset, uint32_t* out_ids, float* out_dist,
                    int mem_kind, void* stream) {
    return knn_float_call(knn_free_call(device, base, n, queries, n_q, d, k, metric, self_offset, false, nullptr, nullptr, out_ids, out_dist, mem_kind, stream));
}

int gbnns_exact_knn_tagged(int device, const float* base, uint64_t n, const float* queries, uint64_t n_q, uint32_t d, int k, int metric,
                           int64_t self_offset, const uint32_t* row_tags, const uint32_t* query_tags, uint32_t* out_ids, float* out_dist,
                           int mem_kind, void* stream) {
    return knn_float_call(knn_free_call(device, base, n, queries, n_q, d, k, metric, self_offset, true, row_tags, query_tags, out_ids, out_dist, mem_kind, stream));
}

int gbnns_exact_knn_bytes(int device, const uint8_t* base, uint64_t n, const uint8_t* queries, uint64_t n_q,
                          uint32_t d, int k, int metric, int64_t self_offset, uint32_t* out_ids, float* out_dist,
                          int mem_kind, void* stream) {
    return knn_bytes_call(knn_free_call(device, base, n, queries, n_q, d, k, metric, self_offset, false, nullptr, nullptr, out_ids, out_dist, mem_kind, stream));
}

int gbnns_exact_knn_bytes_tagged(int device, const uint8_t* base, uint64_t n, const uint8_t* queries, uint64_t n_q, uint32_t d, int k, int metric,
                                 int64_t self_offset, const uint32_t* row_tags, const uint32_t* query_tags, uint32_t* out_ids, float* out_dist,
                                 int mem_kind, void* stream) {
    return knn_bytes_call(knn_free_call(device, base, n, queries, n_q, d, k, metric, self_offset, true, row_tags, query_tags, out_ids, out_dist, mem_kind, stream));
}

// The same computation over the handle's own table, read in place at its device row stride (d_pad floats / bytes); the row tags are the
// handle's.  The packed workspace is the call's own: none of the lanes' workspaces is touched.
int gbnns_index_exact_knn(gbnns_index* ix, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags, int k,
                          int64_t self_offset, uint32_t* out_ids, float* out_dist, int mem_kind, void* stream) {
    if ((queries != nullptr) == (queries_u8 != nullptr))
        return fail(GBNNS_ERR_INVALID, "gbnns_index_exact_knn: exactly one of queries / queries_u8");
    if (!ix) return fail(GBNNS_ERR_INVALID, "null argument");
    if (queries_u8 && !ix->db_b) return fail(GBNNS_ERR_INVALID, "gbnns_index_exact_knn: queries_u8 needs a byte handle (gbnns_index_create_bytes)");
    if (queries && ix->db_b)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_index_exact_knn: float queries on a byte handle: there is no mixed-pair scan (uint8 rows against "
                    "float queries); pass queries_u8, or widen the table and call gbnns_exact_knn");
    if (query_tags && !ix->tags.p) return fail(GBNNS_ERR_INVALID, "gbnns_index_exact_knn with query_tags but without gbnns_index_set_tags");
    const bool tagged = query_tags != nullptr;
    int rc;
    if (queries) {
        if (!ix->db) return fail(GBNNS_ERR_INVALID, "gbnns_index_exact_knn: the handle has no original-space table");
        KnnCall<float> c = knn_free_call(ix->device, ix->db, ix->n, queries, n_q, ix->d, k, ix->metric, self_offset, tagged, ix->tags.as<uint32_t>(),
                                         query_tags, out_ids, out_dist, mem_kind, stream);
        c.bstride = ix->d_pad; c.resident = true;
        // (enter_stream: the deferred calls still owed are joined, as by any call without GBNNS_FLAG_DEFER_JOIN, and `stream` waits for the
        // handle's work in flight on another stream -- a gbnns_index_set_tags among it)
        HIP_TRY(hipSetDevice(ix->device));
        if ((rc = enter_stream(ix, static_cast<hipStream_t>(stream)))) return rc;
        rc = knn_float_call(c);
    } else {
        KnnCall<uint8_t> c = knn_free_call(ix->device, ix->db_b, ix->n, queries_u8, n_q, ix->d, k, ix->metric, self_offset, tagged,
                                           ix->tags.as<uint32_t>(), query_tags, out_ids, out_dist, mem_kind, stream);
        c.bstride = ix->d_pad; c.resident = true;
        HIP_TRY(hipSetDevice(ix->device));
        if ((rc = enter_stream(ix, static_cast<hipStream_t>(stream)))) return rc;
        rc = knn_bytes_call(c);
    }
    if (rc == GBNNS_OK && n_q) ix->in_flight = false;  // (the call returned behind a synchronisation of its stream)
    return rc;
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
    *slab = knn_slab(n_q, k, bytes ? 8 : 4);
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
        DevBuf ds_dev, off_dev, nbr_dev, adj_dev, deg_dev;
        struct Release {
            DevBuf* b[5];
            ~Release() { for (DevBuf* x : b) x->release(); }
        } release{{&ds_dev, &off_dev, &nbr_dev, &adj_dev, &deg_dev}};
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
        HIP_TRY(hipMemcpy(adj.data(), adj_dev.p, (size_t)n * cap * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(deg.data(), deg_dev.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    const int rc = gbnns_internal_gd_finish(knn_offsets, knn_nbrs, ds, n, d, M, metric, reverse, threads, adj.data(),
                                            deg.data(), out_host_nodes, out_offsets, out_nbrs);
    if (rc == GBNNS_ERR_INVALID) return fail(rc, "gbnns_build_graph_gd_device: neighbour id out of range");
    if (rc) return fail(rc, "gbnns_build_graph_gd_device: host allocation failed");
    return GBNNS_OK;
}

}  // extern "C"
