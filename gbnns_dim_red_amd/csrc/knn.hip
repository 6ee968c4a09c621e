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

// A workgroup = 4 wavefronts x QB blocks of 32 queries (operand B of the product, in registers for the whole launch: the
// lane's column of every 32 x 32 tile is ITS query, so one threshold per lane and block); blockIdx.y picks a slab of the
// chunk's rows, walked in blocks of 32 (operand A straight from global memory, the next block's fragments requested
// before the current block's products: a 32 K-row chunk of packed rows is 4 MB at d = 32, L2 / Infinity-Cache resident
// while every workgroup sweeps it).  The accumulators start at -0.5 (1 - c) |x|^2 of their rows (16 rows of the block
// per lane: four float4 loads of the norms), so a kept pair is  max over the lane's 16 rows >= rhs[query]  -- eight
// v_max3 and one compare per tile beside its six matrix instructions.
// TAG (gbnns_exact_knn_tagged): a pair whose row is not allowed for its query is not a hit -- neither counted nor stored.  The tag words of
// a lane's 16 rows travel with the block's norms (four more 16-byte requests, the same address pattern; the array is padded like bnorm)
// and are looked at where hits are counted: under a selective filter a query's threshold is its k-th ALLOWED distance, rows of every
// tile pass it, and a fetch in the hit path was a dependent load in most tiles (DESIGN.md 5.1 has both measurements).
template <int KSTEPS, int QB, bool TAG>
__global__ __launch_bounds__(256) void knn_filter_kernel(KnnFilterParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint32_t q0 = (blockIdx.x * 4u + wave) * (QB * 32u);
    if (q0 >= p.nq) return;
    const uint32_t groups = p.dp >> 3;  // 8-dim groups per row = 2 KSTEPS
    // B fragments: query q0 + 32 b + r, k = 16 s + 8 h .. + 7 -> group 2 s + h: hi at halfword 16 (2 s + h), lo 8 further
    bf16x8 qh[QB][KSTEPS], ql[QB][KSTEPS];
    float rhs[QB];
    uint32_t qtag[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        const uint32_t qi = q0 + 32u * b + r;
        const bool ok = qi < p.nq;
        if constexpr (TAG) qtag[b] = ok ? p.qtag[qi] : 0u;
        const uint16_t* qp = p.qpack + (size_t)(ok ? qi : 0u) * groups * 16;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const uint4* src = reinterpret_cast<const uint4*>(qp + (size_t)(2 * s + h) * 16);
            qh[b][s] = __builtin_bit_cast(bf16x8, src[0]);
            ql[b][s] = __builtin_bit_cast(bf16x8, src[1]);
        }
        rhs[b] = ok ? p.rhs[qi] : __builtin_inff();  // (a query beyond the batch keeps nothing)
    }
    // (every compiler-issued load is used here, once: its waits then sit in this prologue and not inside the sweep)
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        asm volatile("" ::"v"(rhs[b]));
        if constexpr (TAG) asm volatile("" ::"v"(qtag[b]));
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) asm volatile("" ::"v"(qh[b][s]), "v"(ql[b][s]));
    }
    const uint32_t blocks = (p.rows + 31u) >> 5;
    const uint32_t per = (blocks + gridDim.y - 1) / gridDim.y;
    const uint32_t b_lo = blockIdx.y * per, b_hi = min(blocks, b_lo + per);
    if (b_lo >= b_hi) return;
    const float scale = -0.5f * (1.0f - kKnnFilterSlack);
    // Fragments and norms of one block of 32 rows (rows beyond the chunk read row 0), requested by hand-written loads: the
    // compiler's own bookkeeping put a full wait (vmcnt(0)) BEHIND the next block's requests -- no overlap at all --
    // whatever the order in the source; these requests are invisible to it, and `landed` below is the one wait, placed in
    // front of the next requests.  (No branch here: the norms' array is readable 64 entries beyond the set and +inf
    // there, and the chunk starts on a multiple of 64 rows; a row of the NEXT chunk that slips through the test is
    // refused where the hits are stored.)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    auto request_block = [&](uint32_t rb, u32x4 (&xh)[KSTEPS], u32x4 (&xl)[KSTEPS], f32x4v (&nx)[4], u32x4 (&tg)[4]) {
        const uint32_t j = rb * 32u + r;
        const uint16_t* bp = p.bpack + ((size_t)(j < p.rows ? j : 0u) * groups + h) * 16;
        const float* np = p.bnorm + rb * 32u + 4u * h;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {  // group 2 s + h: 64 bytes per K step further on
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xh[s]) : "v"(bp + 32 * s));
            asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(xl[s]) : "v"(bp + 32 * s));
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)  // accumulator registers 4 g .. 4 g + 3 = rows 8 g + 4 h + 0 .. 3 of the block
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(nx[g]) : "v"(np + 8 * g));
        if constexpr (TAG) {
            const uint32_t* tp = p.btag + rb * 32u + 4u * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(tg[g]) : "v"(tp + 8 * g));
        }
    };
    auto landed = [&](u32x4 (&xh)[KSTEPS], u32x4 (&xl)[KSTEPS], f32x4v (&nx)[4], u32x4 (&tg)[4]) {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(nx[0]));
#pragma unroll
        for (int g = 1; g < 4; ++g) asm volatile("" : "+v"(nx[g]));
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) asm volatile("" : "+v"(xh[s]), "+v"(xl[s]));
        if constexpr (TAG) {
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(tg[g]));
        }
    };
    // the products and the test of one block of rows against the QB query blocks
    auto sweep_block = [&](uint32_t rb, const u32x4 (&xhr)[KSTEPS], const u32x4 (&xlr)[KSTEPS], const f32x4v (&nx)[4], const u32x4 (&tg)[4]) {
        bf16x8 xh[KSTEPS], xl[KSTEPS];
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) { xh[s] = __builtin_bit_cast(bf16x8, xhr[s]); xl[s] = __builtin_bit_cast(bf16x8, xlr[s]); }
        f32x16 cinit;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            cinit[4 * g + 0] = scale * nx[g].x; cinit[4 * g + 1] = scale * nx[g].y;
            cinit[4 * g + 2] = scale * nx[g].z; cinit[4 * g + 3] = scale * nx[g].w;
        }
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[0], qh[b][0], cinit, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl[0], qh[b][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[0], ql[b][0], acc, 0, 0, 0);
#pragma unroll
            for (int s = 1; s < KSTEPS; ++s) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[s], qh[b][s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl[s], qh[b][s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[s], ql[b][s], acc, 0, 0, 0);
            }
            float m = fmaxf(fmaxf(acc[0], acc[1]), acc[2]);
#pragma unroll
            for (int v = 3; v < 15; v += 2) m = fmaxf(fmaxf(m, acc[v]), acc[v + 1]);
            m = fmaxf(m, acc[15]);
            if (__builtin_expect(__ballot(m >= rhs[b]) != 0ull, 0)) {
                // one returning atomic per lane with hits (its 16 rows of the tile): the places of all of them at once -- a
                // returning atomic per hit serialised up to sixteen memory round trips in every tile that had any, and in
                // the early chunks (thresholds still loose) that is most tiles
                const uint32_t qv = q0 + 32u * b + r;   // (rhs = +inf beyond the batch: never here with qv >= nq)
                uint32_t hits = 0;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const uint32_t j = rb * 32u + (uint32_t)((v & 3) + 8 * (v >> 2)) + 4u * h;
                    hits |= (acc[v] >= rhs[b] && j < p.rows) ? 1u << v : 0u;  // (a threshold of -inf -- list not full yet -- lets -inf through too)
                }
                if constexpr (TAG) {
                    uint32_t tm = 0;
#pragma unroll
                    for (int v = 0; v < 16; ++v) tm |= ((tg[v >> 2][v & 3] & qtag[b]) ? 1u : 0u) << v;
                    hits &= tm;
                }
                if (hits) {
                    uint32_t pos = atomicAdd(&p.count[qv], (uint32_t)__popc(hits));
                    do {
                        const uint32_t v = (uint32_t)__ffs((int)hits) - 1u;
                        hits &= hits - 1u;
                        if (pos < p.cap) p.cand[(size_t)qv * p.cap + pos] = p.row0 + rb * 32u + ((v & 3u) + 8u * (v >> 2)) + 4u * h;
                        else *p.overflow = 1u;
                        pos += 1u;
                    } while (hits);
                }
            }
        }
    };
    // two register sets in turn: wait for the set at hand, request the next block into the other one, sweep
    u32x4 xh0[KSTEPS], xl0[KSTEPS], xh1[KSTEPS], xl1[KSTEPS];
    f32x4v nx0[4], nx1[4];
    u32x4 tg0[4], tg1[4];
    request_block(b_lo, xh0, xl0, nx0, tg0);
    for (uint32_t rb = b_lo;;) {
        landed(xh0, xl0, nx0, tg0);
        if (rb + 1u < b_hi) request_block(rb + 1u, xh1, xl1, nx1, tg1);
        sweep_block(rb, xh0, xl0, nx0, tg0);
        if (++rb >= b_hi) break;
        landed(xh1, xl1, nx1, tg1);
        if (rb + 1u < b_hi) request_block(rb + 1u, xh0, xl0, nx0, tg0);
        sweep_block(rb, xh1, xl1, nx1, tg1);
        if (++rb >= b_hi) break;
    }
}

__global__ __launch_bounds__(256) void knn_thresholds_kernel(const uint64_t* heap, int k, const float* qnorm, uint32_t nq, float* rhs) {
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    if (qi >= nq) return;
    const uint64_t root = heap[qi];
    // heap not full yet (an all-ones key at the root): every row passes
    rhs[qi] = root == ~0ull ? -__builtin_inff()
                            : 0.5f * ((1.0f - kKnnFilterSlack) * qnorm[qi] - knn_fkey_inv((uint32_t)(root >> 32)));
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

template <int KSTEPS, int QB, bool TAG>
hipError_t launch_knn_filter_tt(const KnnFilterParams& p, hipStream_t s) {
    const unsigned gx = (p.nq + QB * 128u - 1) / (QB * 128u);
    const unsigned blocks = (p.rows + 31u) >> 5;
    static const unsigned simds = [] {  // 4 SIMDs per CU of the current device (the MI355X: 1 024)
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return 4u * (unsigned)cus;
    }();
    unsigned gy = gx >= simds ? 1u : (simds + gx - 1) / gx;   // enough workgroups for every SIMD
    if (gy > blocks) gy = blocks;
    if (gy < 1u) gy = 1u;
    hipLaunchKernelGGL((knn_filter_kernel<KSTEPS, QB, TAG>), dim3(gx, gy), dim3(256), 0, s, p);
    return hipGetLastError();
}

// The filter instance of a packed row length, launch and name from one place: K steps of 16; query blocks per wavefront by what the
// operands leave of the register file.
struct KnnFilterPick {
    hipError_t (*launch)(const KnnFilterParams&, hipStream_t);
    const char* name;
};
#define KNN_FILTER(K, QB)                                                                                                   \
    (tagged ? KnnFilterPick{&launch_knn_filter_tt<K, QB, true>, "knn_filter_kernel<" #K ", " #QB ", true>"} \
            : KnnFilterPick{&launch_knn_filter_tt<K, QB, false>, "knn_filter_kernel<" #K ", " #QB ", false>"})
KnnFilterPick knn_filter_pick(uint32_t dp, bool tagged) {
    switch (dp >> 4) {
        case 1: return KNN_FILTER(1, 4);
        case 2: return KNN_FILTER(2, 4);
        case 3: return KNN_FILTER(3, 2);
        case 4: return KNN_FILTER(4, 2);
        case 5: return KNN_FILTER(5, 1);
        case 6: return KNN_FILTER(6, 1);
        case 7: return KNN_FILTER(7, 1);
        case 8: return KNN_FILTER(8, 1);
        default: return KnnFilterPick{nullptr, nullptr};
    }
}
#undef KNN_FILTER
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
    const KnnFilterPick k = knn_filter_pick(p.dp, p.btag != nullptr);
    return k.launch ? k.launch(p, s) : hipErrorInvalidValue;
}
const char* knn_filter_kernel_name(uint32_t dp, bool tagged) { return knn_filter_pick(dp, tagged).name; }

hipError_t launch_knn_thresholds(const uint64_t* heap, size_t heap_stride, int k, const float* qnorm, uint32_t nq, float* rhs, hipStream_t s) {
    (void)heap_stride;
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(knn_thresholds_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, s, heap, k, qnorm, nq, rhs);
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
