// knn_scan_kernels.h -- the exact-distance kernels of the brute-force kNN as templates over the base rows' element: float rows (knn.hip) and
// binary16 rows (knn_half.hip).  Device code shared by inclusion, so that the row kinds cannot drift apart: a binary16 row is widened where it
// is staged or loaded -- widening is exact -- and every operation behind that load, and its order, is the float kernels' (knn_scan_row.inc for
// the narrow scan).  The float instances are the kernels knn.hip held before the row kind became a parameter: B is the LAST template
// argument and defaults to float.
//   knn_scan_kernel / knn_scan_wide_kernel   the scan: every row against every query (the filter's first rows, its overflowed chunks, the dot
//                                            form, d % 4 != 0, d > 128)
//   knn_rescore_kernel                       the rows the matrix-core filter kept, offered to the heaps
//   knn_pool_update_kernel                   ... or to the pools of long lists
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "knn_select.h"     // the distance keys, the heap, the radix select
#include "knn_scan_dist.h"  // f32x2, the tile and workgroup sizes

namespace gbnns {

namespace {

// The table of a launch by its element: KnnParams::base (float rows) / KnnParams::base_h (binary16 bit patterns).
template <class B>
__device__ __forceinline__ const B* knn_rows(const KnnParams& p);
template <>
__device__ __forceinline__ const float* knn_rows<float>(const KnnParams& p) { return p.base; }
template <>
__device__ __forceinline__ const uint16_t* knn_rows<uint16_t>(const KnnParams& p) { return p.base_h; }

__device__ __forceinline__ float knn_widen(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }  // exact, subnormals included

// Step c (elements 4 c .. 4 c + 3) of the row at bp as floats; vec: the step is one aligned load (16 bytes of floats, 8 of halves).
__device__ __forceinline__ float4 knn_row_step(const float* bp, uint32_t c, bool vec) {
    if (vec) return reinterpret_cast<const float4*>(bp)[c];
    return make_float4(bp[4 * c], bp[4 * c + 1], bp[4 * c + 2], bp[4 * c + 3]);
}
__device__ __forceinline__ float4 knn_row_step(const uint16_t* bp, uint32_t c, bool vec) {
    if (vec) {
        const uint2 w = reinterpret_cast<const uint2*>(bp)[c];
        return make_float4(knn_widen((uint16_t)w.x), knn_widen((uint16_t)(w.x >> 16)), knn_widen((uint16_t)w.y), knn_widen((uint16_t)(w.y >> 16)));
    }
    return make_float4(knn_widen(bp[4 * c]), knn_widen(bp[4 * c + 1]), knn_widen(bp[4 * c + 2]), knn_widen(bp[4 * c + 3]));
}

// S = 16-byte steps of a query held in registers (d <= 4 * S), QPT = queries per thread.
// TAG (gbnns_exact_knn_tagged): a row whose tag word shares no bit with the query's is not offered; the tile's tag words are staged in LDS
// with the tile, once for all its queries.  Same arithmetic; the untagged instances are the code they were.
template <int METRIC, int S, int QPT, bool TAG, class B = float>
__global__ __launch_bounds__(kKnnThreads) void knn_scan_kernel(KnnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* tile = reinterpret_cast<float4*>(smem);  // [kKnnTile][S]
    uint32_t* tile_tag = reinterpret_cast<uint32_t*>(tile + kKnnTile * S);  // [kKnnTile], TAG instances only
    const int t = threadIdx.x;
    // L2Metric::Dist uses the first 4 * floor(d / 4) dims only; the dot form is offered for d % 8 == 0
    const uint32_t steps = p.dim >> 2;
    const bool vec_ok = (p.bstride & 3u) == 0;   // rows 16-B aligned -> float4 loads (8-B aligned halves -> one load a step)
    const bool qvec_ok = (p.qstride & 3u) == 0;
    const B* const rows_base = knn_rows<B>(p);

    float4 q[QPT][S];
    uint32_t qi[QPT];
    bool live[QPT];
    uint64_t root[QPT];
    uint32_t qtag[QPT];
#pragma unroll
    for (int a = 0; a < QPT; ++a) {
        qi[a] = (blockIdx.x * QPT + a) * kKnnThreads + t;
        live[a] = qi[a] < p.nq;
        root[a] = live[a] ? p.heap[qi[a]] : ~0ull;  // (all-ones in a fresh heap; an earlier slice's root otherwise)
        if constexpr (TAG) qtag[a] = live[a] ? p.query_tags[qi[a]] : 0u;
        const float* qp = p.q + (size_t)(live[a] ? qi[a] : 0u) * p.qstride;
#pragma unroll
        for (int c = 0; c < S; ++c) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((uint32_t)c < steps) {
                if (qvec_ok) v = reinterpret_cast<const float4*>(qp)[c];
                else v = make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]);
            }
            q[a][c] = v;
        }
    }

    for (uint64_t base0 = 0; base0 < p.n; base0 += kKnnTile) {
        __syncthreads();  // everyone is done with the previous tile
        for (int e = t; e < kKnnTile * S; e += kKnnThreads) {
            const int r = e / S, c = e % S;
            const uint64_t row = base0 + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < p.n && (uint32_t)c < steps) v = knn_row_step(rows_base + (size_t)row * p.bstride, (uint32_t)c, vec_ok);
            tile[e] = v;
        }
        if constexpr (TAG) {
            if (t < kKnnTile) tile_tag[t] = base0 + t < p.n ? p.row_tags[p.row0 + base0 + t] : 0u;
        }
        __syncthreads();
        const int rows = (p.n - base0 < (uint64_t)kKnnTile) ? (int)(p.n - base0) : kKnnTile;
        for (int r = 0; r < rows; ++r) {
            float dist[QPT];
            const float4* trow = tile + r * S;
#include "knn_scan_row.inc"  // dist[] = the row's distances to q[] (shared with knn_gather_kernel)
            const uint64_t row = p.row0 + base0 + r;
            uint32_t rtag = 0;
            if constexpr (TAG) rtag = tile_tag[r];
#pragma unroll
            for (int a = 0; a < QPT; ++a) {
                const uint64_t key = ((uint64_t)knn_fkey(dist[a]) << 32) | (uint32_t)row;
                bool self = p.self_offset >= 0 && row == (uint64_t)qi[a] + (uint64_t)p.self_offset;
                if constexpr (TAG) self = self || (rtag & qtag[a]) == 0u;  // (a disallowed row is dropped where the query's own row is)
                if (live[a] && !self && key < root[a])
                    root[a] = heap_replace_root(p.heap + qi[a], p.heap_stride, p.k, key);
            }
        }
    }

    if (p.keep_heap) return;
    // heap sort in place (ascending), then the outputs; every lane runs the same trip counts
#pragma unroll
    for (int a = 0; a < QPT; ++a) {
        if (!live[a]) continue;
        uint64_t* h = p.heap + qi[a];
        const size_t st = p.heap_stride;
        for (int m = p.k - 1; m > 0; --m) {
            const uint64_t last = h[(size_t)m * st];
            h[(size_t)m * st] = h[0];
            heap_replace_root(h, st, m, last);
        }
        for (int e = 0; e < p.k; ++e) {
            const uint64_t kv = h[(size_t)e * st];
            const uint32_t id = (uint32_t)kv;
            p.out_ids[(size_t)qi[a] * p.k + e] = id;  // all-ones (never offered) -> 0xFFFFFFFF: fewer than k rows
            if (p.out_dist)
                p.out_dist[(size_t)qi[a] * p.k + e] = (kv == ~0ull) ? __builtin_inff() : knn_fkey_inv((uint32_t)(kv >> 32));
        }
    }
}

// Wide rows (d > 128): a query no longer fits a thread's registers next to its running sums, so the loops are
// turned around.  A thread still owns one query, but walks the base set in tiles of R rows whose running sums
// (R x 4 for L2, R x 8 for the dot form) it keeps in registers while it streams its own query through in chunks
// of eight 16-byte steps (read from global memory: its row is re-read once per tile and stays in the caches);
// the tile [R][steps rounded up to 8, zero filled] sits in LDS and is read by broadcast.  Per distance the
// operations and their order are exactly those of the narrow kernel (a zero-filled step adds +0 to sums that
// are never -0).  Offers to the heap happen in ascending row order, as before.
// TAG: as in knn_scan_kernel (the tile's R tag words behind the tile in LDS).
template <int METRIC, int R, bool TAG, class B = float>
__global__ __launch_bounds__(kKnnThreads) void knn_scan_wide_kernel(KnnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* tile = reinterpret_cast<float4*>(smem);  // [R][steps8]
    const int t = threadIdx.x;
    const uint32_t steps = p.dim >> 2;
    const uint32_t steps8 = (steps + 7u) & ~7u;
    uint32_t* tile_tag = reinterpret_cast<uint32_t*>(tile + (size_t)R * steps8);  // [R], TAG instances only
    const bool vec_ok = (p.bstride & 3u) == 0;
    const bool qvec_ok = (p.qstride & 3u) == 0;
    const B* const rows_base = knn_rows<B>(p);
    const uint32_t qi = blockIdx.x * kKnnThreads + t;
    const bool live = qi < p.nq;
    const float* qp = p.q + (size_t)(live ? qi : 0u) * p.qstride;
    uint64_t root = live ? p.heap[qi] : ~0ull;
    uint32_t qtag = 0;
    if constexpr (TAG) qtag = live ? p.query_tags[qi] : 0u;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (uint64_t base0 = 0; base0 < p.n; base0 += R) {
        __syncthreads();  // everyone is done with the previous tile
        for (uint32_t e = t; e < (uint32_t)R * steps8; e += kKnnThreads) {
            const uint32_t r = e / steps8, c = e % steps8;
            const uint64_t row = base0 + r;
            float4 v = zero4;
            if (row < p.n && c < steps) v = knn_row_step(rows_base + (size_t)row * p.bstride, c, vec_ok);
            tile[e] = v;
        }
        if constexpr (TAG) {
            if (t < R) tile_tag[t] = base0 + t < p.n ? p.row_tags[p.row0 + base0 + t] : 0u;
        }
        __syncthreads();
        float dist[R];
        if constexpr (METRIC == 0) {
            f32x2 s01[R], s23[R];
#pragma unroll
            for (int r = 0; r < R; ++r) s01[r] = s23[r] = f32x2{0.f, 0.f};
            for (uint32_t c0 = 0; c0 < steps8; c0 += 8) {
                float4 qv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t c = c0 + j;
                    qv[j] = zero4;
                    if (c < steps) {
                        if (qvec_ok) qv[j] = reinterpret_cast<const float4*>(qp)[c];
                        else qv[j] = make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const f32x2 q01{qv[j].x, qv[j].y}, q23{qv[j].z, qv[j].w};
#pragma unroll
                    for (int r = 0; r < R; ++r) {  // support_func.h:113-124: e = a - b; sum += e * e, four lanes
                        const float4 b = tile[r * steps8 + c0 + j];  // same address in every lane: LDS broadcast
                        const f32x2 e01 = f32x2{b.x, b.y} - q01;
                        const f32x2 e23 = f32x2{b.z, b.w} - q23;
                        s01[r] = s01[r] + e01 * e01;
                        s23[r] = s23[r] + e23 * e23;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) dist[r] = ((s01[r].x + s01[r].y) + s23[r].x) + s23[r].y;  // :125-126
        } else {
            f32x2 cs[R][4];  // eight running sums (k mod 8) as four pairs: {0,1} {2,3} {4,5} {6,7}
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) cs[r][j] = f32x2{0.f, 0.f};
            for (uint32_t c0 = 0; c0 < steps8; c0 += 8) {
                float4 qv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t c = c0 + j;
                    qv[j] = zero4;
                    if (c < steps) {
                        if (qvec_ok) qv[j] = reinterpret_cast<const float4*>(qp)[c];
                        else qv[j] = make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const f32x2 q01{qv[j].x, qv[j].y}, q23{qv[j].z, qv[j].w};
                    const int o = (j & 1) * 2;  // support_func.h:140-147 (c0 is a multiple of 8: c & 1 == j & 1)
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float4 b = tile[r * steps8 + c0 + j];
                        cs[r][o + 0] = cs[r][o + 0] + f32x2{b.x, b.y} * q01;
                        cs[r][o + 1] = cs[r][o + 1] + f32x2{b.z, b.w} * q23;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const f32x2 m01 = cs[r][2] + cs[r][0], m23 = cs[r][3] + cs[r][1];  // :148 hi half onto lo half
                dist[r] = -((m01.x + m01.y) + (m23.x + m23.y));                     // :160-162
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t row = p.row0 + base0 + r;
            const uint64_t key = ((uint64_t)knn_fkey(dist[r]) << 32) | (uint32_t)row;
            bool self = p.self_offset >= 0 && row == (uint64_t)qi + (uint64_t)p.self_offset;
            if constexpr (TAG) self = self || (tile_tag[r] & qtag) == 0u;
            if (live && base0 + r < p.n && !self && key < root)
                root = heap_replace_root(p.heap + qi, p.heap_stride, p.k, key);
        }
    }
    if (!live || p.keep_heap) return;
    uint64_t* h = p.heap + qi;
    const size_t st = p.heap_stride;
    for (int m = p.k - 1; m > 0; --m) {  // heap sort in place (ascending)
        const uint64_t last = h[(size_t)m * st];
        h[(size_t)m * st] = h[0];
        heap_replace_root(h, st, m, last);
    }
    for (int e = 0; e < p.k; ++e) {
        const uint64_t kv = h[(size_t)e * st];
        p.out_ids[(size_t)qi * p.k + e] = (uint32_t)kv;
        if (p.out_dist)
            p.out_dist[(size_t)qi * p.k + e] = (kv == ~0ull) ? __builtin_inff() : knn_fkey_inv((uint32_t)(kv >> 32));
    }
}

template <int METRIC, int R, bool TAG, class B>
hipError_t launch_knn_wide(const KnnParams& p, hipStream_t s) {
    const uint32_t steps8 = ((p.dim >> 2) + 7u) & ~7u;
    const size_t lds = (size_t)R * steps8 * 16 + (TAG ? R * 4 : 0);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_scan_wide_kernel<METRIC, R, TAG, B>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const unsigned grid = (unsigned)((p.nq + (uint64_t)kKnnThreads - 1) / (uint64_t)kKnnThreads);
    hipLaunchKernelGGL((knn_scan_wide_kernel<METRIC, R, TAG, B>), dim3(grid), dim3(kKnnThreads), lds, s, p);
    return hipGetLastError();
}

template <int METRIC, int S, int QPT, bool TAG, class B>
hipError_t launch_knn_t(const KnnParams& p, hipStream_t s) {
    const size_t lds = (size_t)kKnnTile * S * 16 + (TAG ? kKnnTile * 4 : 0);
    const unsigned grid = (unsigned)((p.nq + (uint64_t)kKnnThreads * QPT - 1) / ((uint64_t)kKnnThreads * QPT));
    hipLaunchKernelGGL((knn_scan_kernel<METRIC, S, QPT, TAG, B>), dim3(grid), dim3(kKnnThreads), lds, s, p);
    return hipGetLastError();
}

// The scan instance of a shape: its launch and its name from one place (launch_knn_scan starts what gbnns_debug_knn_plan names).  A
// binary16 instance carries its row kind as the name's last argument: "knn_scan_kernel<0, 8, 2, false, half>".
struct KnnScanPick {
    hipError_t (*launch)(const KnnParams&, hipStream_t);
    const char* name;
};
template <class B>
constexpr bool kKnnHalfRows = sizeof(B) == 2;
#define KNN_SCAN(M, S, QPT, TAG)                                                                                      \
    KnnScanPick{&launch_knn_t<M, S, QPT, TAG, B>, kKnnHalfRows<B> ? "knn_scan_kernel<" #M ", " #S ", " #QPT ", " #TAG ", half>" \
                                                                   : "knn_scan_kernel<" #M ", " #S ", " #QPT ", " #TAG ">"}
#define KNN_WIDE(M, R, TAG)                                                                                       \
    KnnScanPick{&launch_knn_wide<M, R, TAG, B>, kKnnHalfRows<B> ? "knn_scan_wide_kernel<" #M ", " #R ", " #TAG ", half>" \
                                                                 : "knn_scan_wide_kernel<" #M ", " #R ", " #TAG ">"}
// X(metric, ..., tagged) at the call's metric and tag form
#define KNN_BY_METRIC_TAG(X, ...) \
    (metric == 1 ? (tagged ? X(1, __VA_ARGS__, true) : X(1, __VA_ARGS__, false)) : (tagged ? X(0, __VA_ARGS__, true) : X(0, __VA_ARGS__, false)))
template <class B>
KnnScanPick knn_scan_pick(int metric, uint32_t dim, bool tagged) {
    if (dim <= 32) return KNN_BY_METRIC_TAG(KNN_SCAN, 8, 2);
    if (dim <= 64) return KNN_BY_METRIC_TAG(KNN_SCAN, 16, 2);
    if (dim <= 128) return KNN_BY_METRIC_TAG(KNN_SCAN, 32, 1);
    // wide rows: tiles of 16 (L2) / 8 (dot) rows with their running sums in registers; the [R][d] tile must fit the
    // 160 KB of LDS (64 d bytes at R = 16), so very wide rows take fewer rows per tile: d <= 2560 / 5120 / 8192
    // (a tagged instance's R tag words behind the tile: d = 8192 at R = 4 is 128 KB + 16 bytes)
    const size_t row_bytes = (size_t)(((dim >> 2) + 7u) & ~7u) * 16;
    const size_t room = 160 * 1024 - (tagged ? 64 : 0);
    if (metric != 1 && 16 * row_bytes <= room) return tagged ? KNN_WIDE(0, 16, true) : KNN_WIDE(0, 16, false);
    if (8 * row_bytes <= room) return KNN_BY_METRIC_TAG(KNN_WIDE, 8);
    if (4 * row_bytes <= room) return KNN_BY_METRIC_TAG(KNN_WIDE, 4);
    return KnnScanPick{nullptr, nullptr};  // d > 10240: refused by gbnns_exact_knn (d <= 8192) before it gets here
}
#undef KNN_BY_METRIC_TAG
#undef KNN_WIDE
#undef KNN_SCAN

// One thread per query: the exact distance (L2Metric::Dist, support_func.h:107-128, the scan kernels' operations and order)
// of every candidate the filter kept, offered to the query's heap; then the query's new threshold.  d <= 128, query in
// registers, candidate rows straight from global memory.
template <int S, class B = float>
__global__ __launch_bounds__(128) void knn_rescore_kernel(KnnRescoreParams p) {
    const KnnParams& kp = p.k;
    const uint32_t qi = blockIdx.x * 128u + threadIdx.x;
    if (qi >= kp.nq) return;
    const uint32_t steps = kp.dim >> 2;
    const float* qp = kp.q + (size_t)qi * kp.qstride;
    float4 q[S];
#pragma unroll
    for (int c = 0; c < S; ++c)
        q[c] = (uint32_t)c < steps ? make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    uint64_t root = kp.heap[qi];
    const uint32_t cnt = min(p.count[qi], p.cap);
    for (uint32_t e = 0; e < cnt; ++e) {
        const uint32_t row = p.cand[(size_t)qi * p.cap + e];
        const B* bp = knn_rows<B>(kp) + (size_t)row * kp.bstride;
        f32x2 s01{0.f, 0.f}, s23{0.f, 0.f};
#pragma unroll
        for (int c = 0; c < S; ++c) {
            if ((uint32_t)c < steps) {
                const float4 b4 = knn_row_step(bp, (uint32_t)c, kKnnHalfRows<B>);  // (the filter's shapes: d % 4 == 0, a half step is one aligned load)
                const f32x2 b01{b4.x, b4.y}, b23{b4.z, b4.w};
                const f32x2 e01 = b01 - f32x2{q[c].x, q[c].y};
                const f32x2 e23 = b23 - f32x2{q[c].z, q[c].w};
                s01 = s01 + e01 * e01;
                s23 = s23 + e23 * e23;
            }
        }
        const float dist = ((s01.x + s01.y) + s23.x) + s23.y;
        const uint64_t key = ((uint64_t)knn_fkey(dist) << 32) | row;
        const bool self = kp.self_offset >= 0 && (uint64_t)row == (uint64_t)qi + (uint64_t)kp.self_offset;
        if (!self && key < root) root = heap_replace_root(kp.heap + qi, kp.heap_stride, kp.k, key);
    }
    p.rhs[qi] = root == ~0ull ? -__builtin_inff()
                              : 0.5f * ((1.0f - kKnnFilterSlack) * p.qnorm[qi] - knn_fkey_inv((uint32_t)(root >> 32)));
}

// ------------------------------------------------------------------------------------------
// Long lists (k >= 64; the reference's graph builder reads 1 000-NN lists, dim_red/support_func.py:374-384 ->
// prepare_graph.cpp:66).  A binary heap per query in global memory costs ~3 log2 k scattered accesses per entrant and a
// query sees about k ln(n / k) entrants (7 000 at k = 1 000, n = 10^6): 20 TB of 64-byte lines for 10^6 queries, seven
// seconds.  Here a query's current k smallest keys are an UNORDERED pool [k] in global memory and one wavefront serves
// one query per chunk: it reads the pool into LDS (coalesced), computes the exact distances (the reference's operations
// and order, one candidate per lane) of the rows the filter kept, appends the keys below the pool's largest, and when
// the appended keys fill their buffer -- or the chunk ends -- keeps the k smallest of the union with a radix select on the
// 64-bit (distance, id) keys: a 256-bin histogram per digit from the top, until the bin that holds the k-th key holds
// nothing else.  Same set of keys as the heaps would hold, whatever the order; knn_pool_finalize_kernel sorts it.
// ------------------------------------------------------------------------------------------
// (kPoolNew appended keys per selection round, pool_select: knn_select.h)
template <int S, class B = float>
__global__ __launch_bounds__(64) void knn_pool_update_kernel(KnnPoolParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_pool_smem[];
    const KnnParams& kp = p.k;
    const uint32_t qi = blockIdx.x;
    const int lane = threadIdx.x;
    const int k = kp.k;
    const uint32_t cnt = min(p.count[qi], p.cap);
    if (cnt == 0) return;  // (threshold unchanged)
    uint64_t* keys = reinterpret_cast<uint64_t*>(knn_pool_smem);
    uint32_t* hist = reinterpret_cast<uint32_t*>(keys + k + kPoolNew);
    uint64_t* pool = p.pool + (size_t)qi * (size_t)k;
    for (int i = lane; i < k; i += 64) keys[i] = pool[i];
    uint64_t root = p.root[qi];
    const uint32_t steps = kp.dim >> 2;
    const float* qp = kp.q + (size_t)qi * kp.qstride;
    float4 q[S];
#pragma unroll
    for (int c = 0; c < S; ++c)
        q[c] = (uint32_t)c < steps ? make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    int nnew = 0;
    for (uint32_t e0 = 0; e0 < cnt; e0 += 64) {
        const uint32_t e = e0 + (uint32_t)lane;
        const bool valid = e < cnt;
        const uint32_t row = valid ? p.cand[(size_t)qi * p.cap + e] : 0u;
        const B* bp = knn_rows<B>(kp) + (size_t)row * kp.bstride;
        f32x2 s01{0.f, 0.f}, s23{0.f, 0.f};  // L2Metric::Dist, the scan kernels' operations and order
#pragma unroll
        for (int c = 0; c < S; ++c) {
            if ((uint32_t)c < steps) {
                const float4 b4 = knn_row_step(bp, (uint32_t)c, true);
                const f32x2 e01 = f32x2{b4.x, b4.y} - f32x2{q[c].x, q[c].y};
                const f32x2 e23 = f32x2{b4.z, b4.w} - f32x2{q[c].z, q[c].w};
                s01 = s01 + e01 * e01;
                s23 = s23 + e23 * e23;
            }
        }
        const float dist = ((s01.x + s01.y) + s23.x) + s23.y;
        const uint64_t key = ((uint64_t)knn_fkey(dist) << 32) | row;
        const bool self = kp.self_offset >= 0 && (uint64_t)row == (uint64_t)qi + (uint64_t)kp.self_offset;
        const bool keep = valid && !self && key < root;
        const uint64_t m = __ballot(keep);
        if (keep) keys[k + nnew + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = key;
        nnew += __popcll(m);
        if (nnew > kPoolNew - 64) {
            __syncthreads();
            root = pool_select(keys, k, k + nnew, hist, lane);
            nnew = 0;
        }
    }
    __syncthreads();
    if (nnew) root = pool_select(keys, k, k + nnew, hist, lane);
    for (int i = lane; i < k; i += 64) pool[i] = keys[i];
    if (lane == 0) {
        p.root[qi] = root;
        p.rhs[qi] = root == ~0ull ? -__builtin_inff()
                                  : 0.5f * ((1.0f - kKnnFilterSlack) * p.qnorm[qi] - knn_fkey_inv((uint32_t)(root >> 32)));
    }
}

template <class B>
hipError_t launch_knn_rescore_rows(const KnnRescoreParams& p, hipStream_t s) {
    if (p.k.nq == 0) return hipSuccess;
    const dim3 grid((p.k.nq + 127u) / 128u), block(128);
    if (p.k.dim <= 32) hipLaunchKernelGGL((knn_rescore_kernel<8, B>), grid, block, 0, s, p);
    else if (p.k.dim <= 64) hipLaunchKernelGGL((knn_rescore_kernel<16, B>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((knn_rescore_kernel<32, B>), grid, block, 0, s, p);
    return hipGetLastError();
}

template <class B>
hipError_t launch_knn_pool_update_rows(const KnnPoolParams& p, hipStream_t s) {
    if (p.k.nq == 0) return hipSuccess;
    const size_t lds = ((size_t)p.k.k + kPoolNew) * 8 + 256 * 4;
    const dim3 grid(p.k.nq), block(64);
    auto go = [&](auto kernel) {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kernel, grid, block, lds, s, p);
        return hipGetLastError();
    };
    if (p.k.dim <= 32) return go(knn_pool_update_kernel<8, B>);
    if (p.k.dim <= 64) return go(knn_pool_update_kernel<16, B>);
    return go(knn_pool_update_kernel<32, B>);
}

}  // namespace

}  // namespace gbnns
