// knn_half.hip -- exact brute-force kNN over binary16 rows against float32 queries for gfx950 (MI355X): gbnns_exact_knn_half and
// gbnns_index_exact_knn_half.  Every output byte is gbnns_exact_knn's over the widened rows.
//
// The scheme is knn.hip's: an approximate distance with a KNOWN error bound decides which rows are worth an exact distance, the exact
// distance is the reference's own arithmetic (the half-row instances of knn_scan_kernels.h: a row is widened while it is staged or loaded,
// which is exact).  What differs is the matrix-core product.  A binary16 row IS an exact operand of v_mfma_f32_32x32x16_f16 and lies in
// memory as the A fragment wants it -- lane (r, h) of K step s needs halves 16 s + 8 h .. + 7 of row r, one 16-byte chunk -- so the table
// is swept in place, at its own stride, with nothing packed and nothing split.  Only the float32 query is split:
//   q s = hi + lo + r     hi = f16(q s), lo = f16(q s - hi), s = 2^t per query with max_k |q_k s| in [2^12, 2^13)
// so that hi never overflows binary16 (max 65 504) and the large coordinates' lo parts stay normal, whatever the query's magnitude.  Two
// products per K step (x.hi, x.lo; the float filter needs three), every product exact in f32 (11 x 11 significand bits).  The scale is
// undone per lane and register: t = fma(acc, 1 / s, -0.5 (1 - c) |x|^2) -- one rounding -- and a pair is kept when t >= rhs[query], the
// float filter's test (knn.hip).  A lane whose chunk 2 s + h lies beyond a row's last chunk of dimensions reads that last chunk again:
// the query's halves are zero there, so nothing is read past a row and the table needs no tail padding.
//
// Error bound, on the scale |q|^2 + |x|^2 as in knn.hip (a = |q|^2 + |x|^2 - 2 q.x against the reference's Dist):
//   rows          none: x is the operand.
//   dropped r     |r_k| <= 2^-22 |q_k s| (two round-to-nearest binary16 steps of 11 bits), plus an absolute 2^-25 where lo is subnormal
//                 (|q_k s| < 2^-3 or so): sum |x_k r_k| / s <= 2^-22 sum |x_k q_k| + 2^-25 sum |x_k| / s; with 1 / s <= 2^-12 max |q_k| the
//                 second term is <= 2^-37 sqrt(d) |x| |q|.  On a (twice the dot product's error, sum |x_k q_k| <= (|q|^2 + |x|^2) / 2):
//                 < 2^-21 (|q|^2 + |x|^2).
//   accumulation  2 dp / 16 matrix instructions of 16 products each; taken as one add per product that may truncate (2^-23) against a
//                 partial sum <= (1 + 2^-10) sum |x_k q_k s|: <= 2 dp 2^-23 on the dot product's scale, 2 dp 2^-23 (|q|^2 + |x|^2) on a's.
//                 The accumulators start at ZERO here (|x|^2 enters in the final fma), so no step rounds against |x|^2.
//   the fma       one rounding of q.x - 0.5 (1 - c) |x|^2: 2^-24 (|q|^2 + |x|^2).
//   norms, Dist   |q|^2 and |x|^2 summed in float32 (d 2^-24 each) and the reference distance's own rounding against the real value
//                 (<= (d / 4 + 3) 2^-23 Dist, Dist <= 2 (|q|^2 + |x|^2)): < 2^-16 at d = 128.
// The static_assert below pins  c >= 4 dp 2^-23 + 2^-15  at the longest row -- twice the accumulation term above and twice the rest.
// The bound assumes what the instruction set documents for gfx942 and later: the matrix pipe keeps subnormal binary16 operands (rows
// scaled by 2^-20 are mostly subnormal halves; tests/test_gpu_knn_half.py runs that class against the plain reference).  It also assumes
// |q|^2 + |x|^2 in normal float32 range: a query with |q|^2 not finite or outside 2^-96 .. 2^96 raises a flag in the query-side kernel and
// the whole call takes the exact scan, which serves any finite input.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "knn_sweep.h"
#include "knn_scan_kernels.h"  // the scan, rescore and pool kernels: the binary16 instances

namespace gbnns {

namespace {

constexpr uint32_t kKnnHalfMaxDim = 128;  // (the bound would allow 256; the rescore kernel holds the query in registers: d <= 128)
static_assert(kKnnFilterSlack >= 4.0f * kKnnHalfMaxDim / 8388608.0f + 1.0f / 32768.0f, "kKnnFilterSlack no longer covers the half-row sweep's error bound at its longest row");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// one thread per row: |x|^2 in float32 (the widened squares are exact; the sum rounds, within the bound's d 2^-24)
__global__ __launch_bounds__(256) void knn_half_norm_kernel(const uint16_t* x, uint32_t stride, uint32_t dim, uint64_t rows, float* norms) {
    const uint64_t row = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (row >= rows) return;
    const uint16_t* xr = x + (size_t)row * stride;
    float n2 = 0.f;
    for (uint32_t c = 0; c < dim; ++c) {
        const float v = knn_widen(xr[c]);
        n2 += v * v;
    }
    norms[row] = n2;
}

// one thread per (row, chunk of 8 halves) of the copy: rows of dp halves, zero from column dim on
__global__ __launch_bounds__(256) void knn_half_pack_kernel(const uint16_t* x, uint32_t stride, uint32_t dim, uint32_t dp, uint64_t rows, uint16_t* packed) {
    const uint32_t chunks = dp >> 3;
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = e / chunks;
    const uint32_t g = (uint32_t)(e % chunks);
    if (row >= rows) return;
    const uint16_t* xr = x + (size_t)row * stride;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t col = g * 8u + j;
        w[j >> 1] |= (col < dim ? (uint32_t)xr[col] : 0u) << (16 * (j & 1));
    }
    *reinterpret_cast<uint4*>(packed + (size_t)row * dp + g * 8u) = make_uint4(w[0], w[1], w[2], w[3]);
}

// one thread per (query, group of 8 dims): the query's scale from its largest coordinate, the group's 8 hi and 8 lo halves (32 contiguous
// bytes, knn_pack_kernel's layout); the thread of group 0 also 1 / s, |q|^2 and the test of the bound's range
__global__ __launch_bounds__(256) void knn_half_qsplit_kernel(const float* q, uint32_t stride, uint32_t dim, uint64_t rows, uint32_t groups, uint16_t* packed,
                                                              float* inv, float* norms, uint32_t* uncovered) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = e / groups;
    const uint32_t g = (uint32_t)(e % groups);
    if (row >= rows) return;
    const float* qr = q + (size_t)row * stride;
    float m = 0.f, n2 = 0.f;
    for (uint32_t c = 0; c < dim; ++c) {
        m = fmaxf(m, fabsf(qr[c]));
        n2 += qr[c] * qr[c];
    }
    if (g == 0) {
        // 2^-96 <= |q|^2 <= 2^96, or the zero query (its distances are the row norms, which the sweep holds exactly as rounded)
        const bool covered = n2 == 0.f || (n2 >= 0x1p-96f && n2 <= 0x1p96f);
        if (!covered) *uncovered = 1u;
        if (packed) { norms[row] = n2; }
    }
    if (!packed) return;
    // m = 1.f x 2^(eb - 127): s = 2^(139 - eb) puts m s into [2^12, 2^13); clamped so that s and 1 / s stay normal (a query that small is
    // flagged above, its operands are then never used)
    const int eb = (int)((__float_as_uint(m) >> 23) & 255u);
    int t = m == 0.f ? 0 : 139 - eb;
    t = t > 126 ? 126 : (t < -126 ? -126 : t);
    const float sc = __uint_as_float((uint32_t)(127 + t) << 23);
    if (g == 0) inv[row] = __uint_as_float((uint32_t)(127 - t) << 23);
    uint16_t hi[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t dcol = g * 8u + j;
        const float v = dcol < dim ? qr[dcol] * sc : 0.f;  // (a power of two: exact)
        const _Float16 h = (_Float16)v;                    // round to nearest even
        const _Float16 l = (_Float16)(v - (float)h);       // (the difference is exact in float32)
        hi[j] = __builtin_bit_cast(uint16_t, h);
        lo[j] = __builtin_bit_cast(uint16_t, l);
    }
    uint4 a, b;
    a.x = hi[0] | (uint32_t)hi[1] << 16; a.y = hi[2] | (uint32_t)hi[3] << 16; a.z = hi[4] | (uint32_t)hi[5] << 16; a.w = hi[6] | (uint32_t)hi[7] << 16;
    b.x = lo[0] | (uint32_t)lo[1] << 16; b.y = lo[2] | (uint32_t)lo[3] << 16; b.z = lo[4] | (uint32_t)lo[5] << 16; b.w = lo[6] | (uint32_t)lo[7] << 16;
    uint4* out = reinterpret_cast<uint4*>(packed + ((size_t)row * groups + g) * 16);
    out[0] = a;
    out[1] = b;
}

// The sweep (knn_sweep.h has the division of work, the hand-issued loads and the hit path).  Operand A: one 16-byte load per K step and lane
// straight from the table (half the float filter's requests, a quarter of its bytes per row); operand B: hi and lo of the scaled query, two
// products per K step on accumulators that start at zero.  A value is fma(acc, 1 / s, -0.5 (1 - c) |x|^2), kept when >= rhs[query]; the
// kept id goes to the rescore.
struct KnnHalfOps {
    typedef KnnHalfSweepParams Params;
    typedef float Val;
    typedef f32x16 Vals;
    struct Q { float thr, qinv; };
    static constexpr int kQFrags = 2, kRowFrags = 1;
    static constexpr bool kKeepsValue = false;
    static __device__ __forceinline__ Q load_q(const Params& p, uint32_t qi, bool ok) { return Q{ok ? p.rhs[qi] : __builtin_inff(), ok ? p.qinv[qi] : 0.f}; }
    static __device__ __forceinline__ void use_q(const Q& q) { asm volatile("" ::"v"(q.thr), "v"(q.qinv)); }
    // knn_pack_kernel's layout: group 2 s + h of 8 dims, hi then lo
    static __device__ __forceinline__ const uint4* q_ptr(const Params& p, uint32_t qi) {
        return reinterpret_cast<const uint4*>(p.qsplit + (size_t)qi * (p.dp >> 3) * 16);
    }
    static __device__ __forceinline__ const char* row_ptr(const Params& p, uint32_t j, uint32_t) {
        return reinterpret_cast<const char*>(p.base + (size_t)j * p.stride);
    }
    // the lane's chunk of K step s: 2 s + h, or the row's last chunk where that lies beyond it
    static __device__ __forceinline__ uint32_t row_off(const Params& p, int s, uint32_t h) { return 16u * min(2u * (uint32_t)s + h, p.last_chunk); }
    static __device__ __forceinline__ const uint32_t* side(const Params& p) { return reinterpret_cast<const uint32_t*>(p.bnorm); }
    static __device__ __forceinline__ Vals rows_init(const knn_u32x4 (&nx)[4]) {
        const float scale = -0.5f * (1.0f - kKnnFilterSlack);
        Vals c;
#pragma unroll
        for (int v = 0; v < 16; ++v) c[v] = scale * __uint_as_float(nx[v >> 2][v & 3]);
        return c;
    }
    template <int KSTEPS>
    static __device__ __forceinline__ Vals tile(const Params&, const knn_u32x4 (&xa)[KSTEPS], const Vals& cinit, const knn_u32x4 (&qf)[2 * KSTEPS], const Q& q) {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const f16x8 x = __builtin_bit_cast(f16x8, xa[s]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, __builtin_bit_cast(f16x8, qf[2 * s]), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, __builtin_bit_cast(f16x8, qf[2 * s + 1]), acc, 0, 0, 0);
        }
        Vals t;  // q.x - 0.5 (1 - c) |x|^2: the scale undone and the norm added in one rounding
#pragma unroll
        for (int v = 0; v < 16; ++v) t[v] = __builtin_fmaf(acc[v], q.qinv, cinit[v]);
        return t;
    }
    static __device__ __forceinline__ uint32_t kept(const Q&, uint32_t id, float) { return id; }
};
template <int KSTEPS, int QB, bool TAG>
__global__ __launch_bounds__(256) void knn_half_sweep_kernel(KnnHalfSweepParams p) {
    knn_sweep_body<KnnHalfOps, KSTEPS, QB, TAG>(p);
}

// K steps of 16 dims; knn_filter_pick's table: the B operands are as many registers, the A sets half as many
KNN_SWEEP_PICK_FN(knn_half_sweep_pick, knn_half_sweep_kernel, KnnHalfSweepParams, 16, KNN_SWEEP_QB_TWO_PART)
#undef KNN_SWEEP_PICK_FN
#undef KNN_SWEEP_PICK_FN_
#undef KNN_SWEEP_CASE_
#undef KNN_SWEEP_INSTANCE_
#undef KNN_SWEEP_QB_TWO_PART
}  // namespace

hipError_t launch_knn_half_norms(const uint16_t* x, uint32_t stride, uint32_t dim, uint64_t rows, float* norms, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    if (stride < dim) return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_half_norm_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, x, stride, dim, rows, norms);
    return hipGetLastError();
}

hipError_t launch_knn_half_pack(const uint16_t* x, uint32_t stride, uint32_t dim, uint32_t dp, uint64_t rows, uint16_t* packed, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    if (stride < dim || dp < dim || (dp & 15u)) return hipErrorInvalidValue;
    const uint64_t threads = rows * (dp >> 3);
    hipLaunchKernelGGL(knn_half_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, x, stride, dim, dp, rows, packed);
    return hipGetLastError();
}

hipError_t launch_knn_half_qsplit(const float* q, uint32_t stride, uint32_t dim, uint32_t dp, uint64_t rows, uint16_t* packed, float* inv, float* norms,
                                  uint32_t* uncovered, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    if (stride < dim || dp < dim || (dp & 15u) || !uncovered || (packed && (!inv || !norms))) return hipErrorInvalidValue;
    const uint32_t groups = packed ? dp >> 3 : 1u;  // (the test alone: one thread a query)
    const uint64_t threads = rows * groups;
    hipLaunchKernelGGL(knn_half_qsplit_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, q, stride, dim, rows, groups, packed, inv, norms, uncovered);
    return hipGetLastError();
}

hipError_t launch_knn_half_sweep(const KnnHalfSweepParams& p, hipStream_t s) {
    if (p.nq == 0 || p.rows == 0) return hipSuccess;
    if (p.btag && !p.qtag) return hipErrorInvalidValue;
    // what keeps every 16-byte request inside its row: an aligned table at a stride of whole chunks that holds the last chunk read
    if ((p.stride & 7u) || (reinterpret_cast<uintptr_t>(p.base) & 15u) || 8u * (p.last_chunk + 1u) > p.stride || 8u * (p.last_chunk + 1u) > p.dp)
        return hipErrorInvalidValue;
    const auto k = knn_half_sweep_pick(p.dp, p.btag != nullptr);
    return k.launch ? k.launch(p, s) : hipErrorInvalidValue;
}
const char* knn_half_sweep_kernel_name(uint32_t dp, bool tagged) { return knn_half_sweep_pick(dp, tagged).name; }

hipError_t launch_knn_half_scan(const KnnParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (!p.base_h || (p.row_tags && !p.query_tags)) return hipErrorInvalidValue;
    const KnnScanPick k = knn_scan_pick<uint16_t>(metric, p.dim, p.row_tags != nullptr);
    return k.launch ? k.launch(p, s) : hipErrorInvalidValue;
}
const char* knn_half_scan_kernel_name(int metric, uint32_t dim, bool tagged) { return knn_scan_pick<uint16_t>(metric, dim, tagged).name; }

hipError_t launch_knn_half_rescore(const KnnRescoreParams& p, hipStream_t s) {
    if (!p.k.base_h || (p.k.bstride & 3u)) return hipErrorInvalidValue;
    return launch_knn_rescore_rows<uint16_t>(p, s);
}

hipError_t launch_knn_half_pool_update(const KnnPoolParams& p, hipStream_t s) {
    if (!p.k.base_h || (p.k.bstride & 3u)) return hipErrorInvalidValue;
    return launch_knn_pool_update_rows<uint16_t>(p, s);
}

}  // namespace gbnns
