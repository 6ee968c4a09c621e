// knn.hip -- exact brute-force k-nearest-neighbour scan for gfx950 (MI355X).
//
// What it replaces in the reference: the brute-force ground truth getTruth (search/support_func.h:270-290,
// k = 1, strict `<` over ascending ids) and the exact kNN lists that feed the graph builder
// (dim_red/support_func.py:374-384 get_nearestneighbors_partly -> `<name>_knn_1k_<style>.ivecs`, read by
// search/prepare_graph.cpp:66).  Result of query i: the k smallest (Dist(base_j, q_i), j) pairs in ascending
// pair order -- distances in the reference's own arithmetic (L2Metric::Dist / Angular::Dist, support_func.h:
// 107-163: same running sums, same order, one rounding per operation), ties broken towards the lower id,
// which is what getTruth's strict `<` over ascending j does.
//
// Shape of the work: n_q x n distances of d dims, every one in a fixed summation order, so this is VALU work
// (sub / mul / add, packed two wide), not an MFMA GEMM: a matrix-core product would round differently.
// One thread owns QPT queries held in registers (d <= 128; wider rows: knn_scan_wide_kernel; both in knn_scan_kernels.h, templates over the rows' element); a workgroup of 128 threads streams the base set
// through LDS in tiles of 64 rows, every thread reading the same row (LDS broadcast reads, one row serves
// QPT x 128 queries).  Selection: a max-heap of k (distance key, id) pairs per query in global memory
// ([k][n_q] so that lanes touching the same heap level coalesce); a row is offered only when it beats the
// heap's root (kept in a register), which after the first few thousand rows is rare
// (about k * ln(n / k) times per query), then the heap is sorted in place.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "knn_select.h"  // the distance keys, the heap, the radix select (shared with knn_bytes.hip)
#include "knn_scan_dist.h"  // f32x2, the tile and workgroup sizes (shared with knn_gather.hip)
#include "knn_sweep.h"  // the matrix-core sweep's skeleton (shared with knn_bytes.hip and knn_half.hip)
#include "knn_scan_kernels.h"  // the scan, rescore and pool kernels, templates over the rows' element (shared with knn_half.hip): the float instances

namespace gbnns {

namespace {

// (f32x2, kKnnThreads = 128 and kKnnTile = 64 base rows per LDS tile: knn_scan_dist.h)

// ------------------------------------------------------------------------------------------
// Matrix-core filter (round 4).  The kNN lists that feed the graph builder are the one stage of this path where
// the reference has no arithmetic of its own to match: they come from faiss / torch.mm (dim_red/support_func.py:20-74,
// 374-384).  What gbnns_exact_knn promises is the k smallest (L2Metric::Dist, id) pairs -- so an approximate distance
// with a KNOWN error bound may decide which rows are worth an exact distance, as long as no row that belongs to the
// answer can be dropped:
//   a(q, x) = |q|^2 + |x|^2 - 2 q.x  with q.x on the matrix cores (v_mfma_f32_32x32x16_bf16, every float split into
//   bf16 hi + lo: q.x ~ qh.xh + qh.xl + ql.xh), |a - Dist| <= eps(q, x) := c (|q|^2 + |x|^2), c = 2^-12 (bound below);
//   a row is kept when a <= T_q + eps, T_q = the query's current exact k-th distance (its heap's root).  A dropped row has
//   Dist >= a - eps > T_q >= the final k-th distance: it is not among the k smallest (distance, id) pairs, ties included.
//   Kept rows get their exact distance in the reference's order (knn_rescore_kernel) and are offered to the same heap
//   as before: the heap ends up holding the same k keys as the full scan's, whatever the order of the offers.
// Error bound: x = xh + xl + r with |xl| <= 2^-8 |x|, |r| <= 2^-16 |x| (two round-to-nearest bf16 steps); the three
// products kept are exact in f32, the three dropped ones sum to <= 3 * 2^-16 |q_k x_k| per dimension; f32 accumulation of
// 3 d products <= 3 d 2^-24 sum |q_k x_k|; sum |q_k x_k| <= |q||x| <= (|q|^2 + |x|^2) / 2.  For d <= 128 the dot
// product is off by <= 3.8e-5 (|q|^2 + |x|^2), a by twice that plus the norms' own rounding (d 2^-24 each) plus the
// reference distance's rounding against the real value (<= (d / 4 + 3) 2^-23 Dist): < 9e-5 (|q|^2 + |x|^2) so far.
// (Round-4 review: one term was missing here.)  The accumulator does not start at zero but at -0.5 (1 - c) |x|^2, so every
// one of the <= 3 d / 16 accumulate steps of the matrix pipe rounds against |x|^2 / 2 + sum |q_k x_k| <= |q|^2 + |x|^2, not
// against sum |q_k x_k| alone -- and its internal adds may truncate (2^-23) instead of rounding to nearest: with 24 steps at
// d = 128 that adds <= 24 * 2^-23 (|q|^2 + |x|^2) = 2.9e-6 on the dot product's scale, 5.7e-6 on a's ... taken with the
// worst case of every other term on top of each other the error on a stays < 1.6e-4 (|q|^2 + |x|^2): c = 2^-12 = 2.44e-4
// leaves a factor 1.5, not the 2.7 claimed before -- and none to spare for longer rows: the shape guard below (dp <= 128)
// and the host's (d <= 128, gbnns_exact_knn) are what the bound rests on.
// ------------------------------------------------------------------------------------------
// the slack c must cover 4 dp 2^-23 (accumulation on the scale |q|^2 + |x|^2, truncating adds) + 2^-14 (the dropped
// lo x lo products and the norms' and the reference distance's own roundings) at the longest row the filter takes
constexpr uint32_t kKnnFilterMaxDim = 128;
static_assert(kKnnFilterSlack >= 4.0f * kKnnFilterMaxDim / 8388608.0f + 1.0f / 16384.0f, "kKnnFilterSlack no longer covers the filter's error bound at its longest row");
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint16_t bf16_rne(float x) {  // round to nearest even (finite inputs)
    const uint32_t u = __float_as_uint(x);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_val(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// one thread per (row, group of 8 dims): writes the 8 hi and 8 lo parts (32 contiguous bytes); thread of group 0 also the norm
__global__ __launch_bounds__(256) void knn_pack_kernel(const float* x, uint32_t stride, uint32_t dim, uint64_t rows, uint32_t groups,
                                                       uint16_t* packed, float* norms) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = e / groups;
    const uint32_t g = (uint32_t)(e % groups);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * stride;
    uint16_t hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t dcol = g * 8u + j;
        const float v = dcol < dim ? xr[dcol] : 0.f;
        hi[j] = bf16_rne(v);
        lo[j] = bf16_rne(v - bf16_val(hi[j]));
    }
    uint4 a, b;
    a.x = hi[0] | (uint32_t)hi[1] << 16; a.y = hi[2] | (uint32_t)hi[3] << 16; a.z = hi[4] | (uint32_t)hi[5] << 16; a.w = hi[6] | (uint32_t)hi[7] << 16;
    b.x = lo[0] | (uint32_t)lo[1] << 16; b.y = lo[2] | (uint32_t)lo[3] << 16; b.z = lo[4] | (uint32_t)lo[5] << 16; b.w = lo[6] | (uint32_t)lo[7] << 16;
    uint4* out = reinterpret_cast<uint4*>(packed + ((size_t)row * groups + g) * 16);
    out[0] = a;
    out[1] = b;
    if (g == 0) {
        float n2 = 0.f;
        for (uint32_t c = 0; c < dim; ++c) n2 += xr[c] * xr[c];
        norms[row] = n2;
    }
}

// The sweep (knn_sweep.h has the division of work, the hand-issued loads and the hit path): rows and queries as packed bf16 hi / lo pairs,
// three products per K step -- xh.qh + xl.qh + xh.ql -- on accumulators that start at -0.5 (1 - c) |x|^2 of their rows, so a value is
// q.x - 0.5 (1 - c) |x|^2 and a pair is kept when it is >= rhs[query]; the kept id goes to the rescore.
struct KnnFilterOps {
    typedef KnnFilterParams Params;
    typedef float Val;
    typedef f32x16 Vals;
    struct Q { float thr; };
    static constexpr int kQFrags = 2, kRowFrags = 2;  // hi, and lo 16 bytes further
    static constexpr bool kKeepsValue = false;
    static __device__ __forceinline__ Q load_q(const Params& p, uint32_t qi, bool ok) { return Q{ok ? p.rhs[qi] : __builtin_inff()}; }
    static __device__ __forceinline__ void use_q(const Q& q) { asm volatile("" ::"v"(q.thr)); }
    // fragments of K step s = group 2 s + h of 8 dims: hi at halfword 16 (2 s + h) of the packed row, lo 8 further; 64 bytes per K step
    static __device__ __forceinline__ const uint4* q_ptr(const Params& p, uint32_t qi) {
        return reinterpret_cast<const uint4*>(p.qpack + (size_t)qi * (p.dp >> 3) * 16);
    }
    static __device__ __forceinline__ const char* row_ptr(const Params& p, uint32_t j, uint32_t h) {
        return reinterpret_cast<const char*>(p.bpack + ((size_t)j * (p.dp >> 3) + h) * 16);
    }
    static __device__ __forceinline__ uint32_t row_off(const Params&, int s, uint32_t) { return 64u * (uint32_t)s; }
    static __device__ __forceinline__ const uint32_t* side(const Params& p) { return reinterpret_cast<const uint32_t*>(p.bnorm); }
    static __device__ __forceinline__ Vals rows_init(const knn_u32x4 (&nx)[4]) {
        const float scale = -0.5f * (1.0f - kKnnFilterSlack);
        Vals c;
#pragma unroll
        for (int v = 0; v < 16; ++v) c[v] = scale * __uint_as_float(nx[v >> 2][v & 3]);
        return c;
    }
    template <int KSTEPS>
    static __device__ __forceinline__ Vals tile(const Params&, const knn_u32x4 (&x)[2 * KSTEPS], Vals acc, const knn_u32x4 (&qf)[2 * KSTEPS], const Q&) {
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const bf16x8 xh = __builtin_bit_cast(bf16x8, x[2 * s]), xl = __builtin_bit_cast(bf16x8, x[2 * s + 1]);
            const bf16x8 qh = __builtin_bit_cast(bf16x8, qf[2 * s]), ql = __builtin_bit_cast(bf16x8, qf[2 * s + 1]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, qh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl, qh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, ql, acc, 0, 0, 0);
        }
        return acc;
    }
    static __device__ __forceinline__ uint32_t kept(const Q&, uint32_t id, float) { return id; }
};
template <int KSTEPS, int QB, bool TAG>
__global__ __launch_bounds__(256) void knn_filter_kernel(KnnFilterParams p) {
    knn_sweep_body<KnnFilterOps, KSTEPS, QB, TAG>(p);
}

// (slack: the calling filter's c -- kKnnFilterSlack, or kKnnWideSlack for knn_wide.hip; 1 - c is exact for either)
__global__ __launch_bounds__(256) void knn_thresholds_kernel(const uint64_t* heap, int k, const float* qnorm, uint32_t nq, float* rhs, float slack) {
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    if (qi >= nq) return;
    const uint64_t root = heap[qi];
    // heap not full yet (an all-ones key at the root): every row passes
    rhs[qi] = root == ~0ull ? -__builtin_inff()
                            : 0.5f * ((1.0f - slack) * qnorm[qi] - knn_fkey_inv((uint32_t)(root >> 32)));
    (void)k;
}

__global__ __launch_bounds__(128) void knn_finalize_kernel(KnnParams p) {
    const uint32_t qi = blockIdx.x * 128u + threadIdx.x;
    if (qi >= p.nq) return;
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

// ascending (distance, id) order of a query's pool and the outputs: one wavefront per query, bitonic network in LDS
__global__ __launch_bounds__(64) void knn_pool_finalize_kernel(KnnPoolParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_pool_smem[];
    const KnnParams& kp = p.k;
    const uint32_t qi = blockIdx.x;
    const int lane = threadIdx.x;
    const int k = kp.k;
    int N = 64;
    while (N < k) N <<= 1;
    uint64_t* keys = reinterpret_cast<uint64_t*>(knn_pool_smem);
    const uint64_t* pool = p.pool + (size_t)qi * (size_t)k;
    for (int i = lane; i < N; i += 64) keys[i] = i < k ? pool[i] : ~0ull;
    __syncthreads();
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (N >> 1); t += 64) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const uint64_t a = keys[i], b = keys[j];
                if ((a > b) == up) { keys[i] = b; keys[j] = a; }
            }
            __syncthreads();
        }
    }
    for (int e = lane; e < k; e += 64) {
        const uint64_t kv = keys[e];
        kp.out_ids[(size_t)qi * k + e] = (uint32_t)kv;
        if (kp.out_dist) kp.out_dist[(size_t)qi * k + e] = (kv == ~0ull) ? __builtin_inff() : knn_fkey_inv((uint32_t)(kv >> 32));
    }
}

// K steps of 16 dims
KNN_SWEEP_PICK_FN(knn_filter_pick, knn_filter_kernel, KnnFilterParams, 16, KNN_SWEEP_QB_TWO_PART)
#undef KNN_SWEEP_PICK_FN
#undef KNN_SWEEP_PICK_FN_
#undef KNN_SWEEP_CASE_
#undef KNN_SWEEP_INSTANCE_
#undef KNN_SWEEP_QB_TWO_PART
}  // namespace

hipError_t launch_knn_scan(const KnnParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (p.row_tags && !p.query_tags) return hipErrorInvalidValue;
    const KnnScanPick k = knn_scan_pick<float>(metric, p.dim, p.row_tags != nullptr);
    return k.launch ? k.launch(p, s) : hipErrorInvalidValue;
}
const char* knn_scan_kernel_name(int metric, uint32_t dim, bool tagged) { return knn_scan_pick<float>(metric, dim, tagged).name; }

hipError_t launch_knn_pack(const float* x, uint32_t stride, uint32_t dim, uint64_t rows, uint16_t* packed, float* norms, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    const uint32_t groups = ((dim + 15u) & ~15u) >> 3;
    const uint64_t threads = rows * groups;
    hipLaunchKernelGGL(knn_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, x, stride, dim, rows, groups, packed, norms);
    return hipGetLastError();
}

hipError_t launch_knn_filter(const KnnFilterParams& p, hipStream_t s) {
    if (p.nq == 0 || p.rows == 0) return hipSuccess;
    if (p.btag && !p.qtag) return hipErrorInvalidValue;
    const auto k = knn_filter_pick(p.dp, p.btag != nullptr);
    return k.launch ? k.launch(p, s) : hipErrorInvalidValue;
}
const char* knn_filter_kernel_name(uint32_t dp, bool tagged) { return knn_filter_pick(dp, tagged).name; }

hipError_t launch_knn_thresholds(const uint64_t* heap, size_t heap_stride, int k, const float* qnorm, uint32_t nq, float* rhs, hipStream_t s, float slack) {
    (void)heap_stride;
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(knn_thresholds_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, s, heap, k, qnorm, nq, rhs, slack);
    return hipGetLastError();
}

hipError_t launch_knn_rescore(const KnnRescoreParams& p, hipStream_t s) { return launch_knn_rescore_rows<float>(p, s); }

hipError_t launch_knn_pool_update(const KnnPoolParams& p, hipStream_t s) { return launch_knn_pool_update_rows<float>(p, s); }

hipError_t launch_knn_pool_finalize(const KnnPoolParams& p, hipStream_t s) {
    if (p.k.nq == 0) return hipSuccess;
    size_t N = 64;
    while (N < (size_t)p.k.k) N <<= 1;
    hipLaunchKernelGGL(knn_pool_finalize_kernel, dim3(p.k.nq), dim3(64), N * 8, s, p);
    return hipGetLastError();
}

hipError_t launch_knn_finalize(const KnnParams& p, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(knn_finalize_kernel, dim3((p.nq + 127u) / 128u), dim3(128), 0, s, p);
    return hipGetLastError();
}

}  // namespace gbnns
