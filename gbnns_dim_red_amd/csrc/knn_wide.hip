// knn_wide.hip -- the matrix-core filter of the exact kNN for float rows wider than 128 dims (gist: 960, glove: 300 / 200) on gfx950
// (MI355X): gbnns_exact_knn / gbnns_exact_knn_tagged with "knn_filter_wide" set, L2, 128 < d <= 1024, d % 4 == 0, k <= 512 (heaps).
//
// The scheme is knn.hip's: a(q, x) = |q|^2 + |x|^2 - 2 q.x with q.x on the matrix cores (v_mfma_f32_32x32x16_bf16, every float split into
// bf16 hi + lo, three products per K step: xh.qh + xl.qh + xh.ql) decides which rows are worth an exact distance; a row is kept when
// a <= T_q + c (|q|^2 + |x|^2), c = kKnnWideSlack, T_q the query's current exact k-th distance; kept rows get L2Metric::Dist in the scan's
// operations and order (knn_wide_rescore_kernel) and are offered to the scan's heaps.  Both operands are knn_pack_kernel's images.
//
// What differs from knn_sweep.h is the division of work.  There a query's packed operands stay in registers for the whole launch -- 2 x
// KSTEPS fragments, at most 8 K steps.  Here the K dimension is looped: a workgroup of 4 wavefronts owns a tile of 128 queries x 128 rows
// of the chunk, wavefront (wq, wr) the 64 x 64 sub-tile of query half wq and row half wr as four 32 x 32 accumulators (64 registers).
// blockIdx.x picks the 128 queries, blockIdx.y a slab of the chunk's blocks of 128 rows.  Per row block the K loop runs over dp =
// round_up(d, 16) in stages of KS K steps: both operands' stage -- 64 KS contiguous bytes of each of 128 packed rows, which is already
// fragment order -- goes global memory -> registers -> LDS, two LDS buffers in turn, the loads hand-issued (knn_sweep.h says why) and
// the next stage's requested right behind the barrier, in front of the current stage's products.  An LDS row is 64 KS + 16 bytes: an odd
// number of 16-byte slots, so the fragment reads of eight consecutive lanes (rows r .. r + 7, same K step half) cover all 32 banks.
// One barrier per stage is enough: stage g is written to buffer g & 1 behind the barrier of stage g - 1, which every wavefront reaches
// only behind its products of stage g - 2, the last readers of that buffer.  K steps beyond dp in the last stage are written as zeros.
// Accumulators start at ZERO; the row norm enters in one fma behind the K loop -- t = fma(-0.5 (1 - c), |x|^2, acc) -- so no accumulate
// step rounds against |x|^2.  Epilogue: knn_sweep.h's hit path (C layout: register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h,
// column r -- a lane's 16 values of a tile belong to ONE query): max over the 16 values, one compare, ballot; a returning atomicAdd per
// lane with hits, ids stored while pos < cap, the overflow flag otherwise; rows beyond the chunk refused by j < rows; TAG instances fetch
// the tag words with the norms (at the head of the row block) and test them where hits are counted.
//
// Error bound for dp <= 1024, on the scale S = |q|^2 + |x|^2 (|a - Dist| <= c S must hold; sum |q_k x_k| <= |q||x| <= S / 2):
//   dropped       x = xh + xl + r, |xl| <= 2^-8 |x|, |r| <= 2^-16 |x| (two round-to-nearest bf16 steps); the three products kept are exact in
//                 f32, the dropped ones (xl.ql, r.q, x.r) sum to <= 3 * 2^-16 |q_k x_k| per dimension, whatever d: on a (twice the dot
//                 product's error) <= 3 * 2^-16 S = 4.6e-5 S.
//   accumulation  3 dp / 16 matrix instructions of 16 products each, taken as one add per product that may truncate (2^-23) against a
//                 partial sum <= sum |q_k x_k|: <= 3 dp 2^-23 sum |q_k x_k| on the dot product, 3 dp 2^-23 S on a: 3.7e-4 S at dp = 1024.
//                 (The narrow filter's accumulators start at the norm term; these start at zero.)
//   the fma       one rounding of q.x - 0.5 (1 - c) |x|^2, a value of at most S / 2: 2^-24 S on a.
//   norms         |q|^2 and |x|^2 summed in float32, d products and d adds each: <= d 2^-23 of each norm, d 2^-23 S together: 1.2e-4 S.
//   Dist          the reference distance's own rounding against the real value, <= (d / 4 + 3) 2^-23 Dist with Dist <= 2 S:
//                 (d / 4 + 3) 2^-22 S = 6.2e-5 S.
//   threshold     rhs = 0.5 ((1 - c) |q|^2 - T) rounds twice against values <= S (the halving is exact): <= 2^-22 S on a.
// Sum at d = dp = 1024: 5.97e-4 S.  c = 2^-10 = 9.77e-4 leaves a factor 1.6; the static_assert pins that sum at kKnnWideMaxDim.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "knn_select.h"     // the distance keys, the heap
#include "knn_scan_dist.h"  // f32x2
#include "knn_scan_kernels.h"  // knn_rows, knn_widen, knn_row_step: the rescore's binary16 instance

namespace gbnns {

namespace {

constexpr float kKnnWideBound = 3.0f * kKnnWideMaxDim / 8388608.0f      // accumulation
                                + 1.0f * kKnnWideMaxDim / 8388608.0f    // both norms
                                + (kKnnWideMaxDim / 4 + 3) / 4194304.0f  // the reference distance
                                + 3.0f / 65536.0f                       // the dropped products
                                + 1.0f / 16777216.0f + 1.0f / 4194304.0f;  // the fma, the threshold
static_assert(kKnnWideSlack >= 1.5f * kKnnWideBound, "kKnnWideSlack no longer covers the wide filter's error bound at its longest row with a factor 1.5");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kWideTile = 128;  // queries, and rows, of a workgroup's tile

template <int KS>
constexpr uint32_t kWidePitch = 64u * KS + 16u;  // bytes of one packed row's stage in LDS
template <int KS>
constexpr uint32_t kWideLds = 4u * kWideTile * kWidePitch<KS>;  // two buffers of two operands

// KS = K steps of 16 dims per stage
template <int KS, bool TAG>
__global__ __launch_bounds__(256) void knn_wide_filter_kernel(KnnFilterParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wide_smem[];
    constexpr uint32_t PITCH = kWidePitch<KS>, OPER = kWideTile * PITCH;  // a buffer: the rows' stage, then the queries'
    constexpr int LD = 2 * KS;            // 16-byte requests per thread, operand and stage: 128 rows x 4 KS / 256 threads
    constexpr uint32_t UNITS = 4u * KS;   // 16-byte units of a row's stage
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint32_t wq = wave & 1u, wr = wave >> 1;
    const uint32_t q0 = blockIdx.x * kWideTile;
    const uint32_t ksteps = p.dp >> 4, stages = (ksteps + KS - 1) / KS;
    const size_t row_bytes = (size_t)p.dp * 4;  // 2 dp 16-bit parts
    const uint32_t blocks = (p.rows + kWideTile - 1) / kWideTile;
    const uint32_t per = (blocks + gridDim.y - 1) / gridDim.y;
    const uint32_t b_lo = blockIdx.y * per, b_hi = min(blocks, b_lo + per);
    if (b_lo >= b_hi) return;  // (the whole workgroup)

    // what this thread moves per stage: unit i = row lrow[i] of the tile, 16-byte unit cu[i] of its stage (consecutive threads: consecutive units of a row)
    uint32_t lrow[LD], cu[LD];
    const char* qsrc[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) {
        const uint32_t u = tid + 256u * i;
        lrow[i] = u / UNITS;
        cu[i] = u % UNITS;
        const uint32_t qi = q0 + lrow[i];
        qsrc[i] = reinterpret_cast<const char*>(p.qpack) + (size_t)(qi < p.nq ? qi : 0u) * row_bytes;  // (a query beyond the batch keeps nothing: its threshold)
    }
    // the thresholds and tag words of the lane's queries: one per 32 x 32 tile column block
    float thr[2];
    uint32_t qtag[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const uint32_t qv = q0 + 64u * wq + 32u * qt + r;
        thr[qt] = qv < p.nq ? p.rhs[qv] : __builtin_inff();
        qtag[qt] = 0u;
        if constexpr (TAG) qtag[qt] = qv < p.nq ? p.qtag[qv] : 0u;
    }

    // a stage's units on their way: rows' then queries'.  A unit of a K step beyond dp (the last stage) is requested at the row's first
    // 16 bytes instead -- readable -- and written as zeros.
    u32x4 stg[2 * LD];
    auto request = [&](uint32_t rb, uint32_t st) {
#pragma unroll
        for (int i = 0; i < LD; ++i) {
            const uint32_t j = rb * kWideTile + lrow[i];
            const bool live = st * KS + (cu[i] >> 2) < ksteps;
            const size_t off = live ? (size_t)st * (64u * KS) + 16u * cu[i] : 0u;
            const char* xp = reinterpret_cast<const char*>(p.bpack) + (size_t)(j < p.rows ? j : 0u) * row_bytes + off;  // (rows beyond the chunk read row 0; refused below)
            const char* qp = qsrc[i] + off;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(stg[i]) : "v"(xp));
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(stg[LD + i]) : "v"(qp));
        }
    };
    auto landed = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(stg[0]));
#pragma unroll
        for (int i = 1; i < 2 * LD; ++i) asm volatile("" : "+v"(stg[i]));
    };
    auto to_lds = [&](uint32_t buf, uint32_t st) {
        unsigned char* xb = wide_smem + buf * 2u * OPER;
#pragma unroll
        for (int i = 0; i < LD; ++i) {
            const bool live = st * KS + (cu[i] >> 2) < ksteps;
            const u32x4 zero = {0u, 0u, 0u, 0u};
            const uint32_t at = lrow[i] * PITCH + 16u * cu[i];
            *reinterpret_cast<u32x4*>(xb + at) = live ? stg[i] : zero;
            *reinterpret_cast<u32x4*>(xb + OPER + at) = live ? stg[LD + i] : zero;
        }
    };

    f32x16 acc[2][2];  // [query block][row block] of the wavefront's 64 x 64
    auto products = [&](uint32_t buf) {
        const unsigned char* xb = wide_smem + buf * 2u * OPER + (64u * wr + r) * PITCH + 32u * h;
        const unsigned char* qb = wide_smem + buf * 2u * OPER + OPER + (64u * wq + r) * PITCH + 32u * h;
#pragma unroll
        for (int s = 0; s < KS; ++s) {  // fragments of K step s: group 2 s + h of 8 dims, hi then lo
            bf16x8 xh[2], xl[2], qh[2], ql[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                xh[b] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(xb + 32u * b * PITCH + 64u * s));
                xl[b] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(xb + 32u * b * PITCH + 64u * s + 16u));
                qh[b] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(qb + 32u * b * PITCH + 64u * s));
                ql[b] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(qb + 32u * b * PITCH + 64u * s + 16u));
            }
            // (four accumulators in turn: no product waits for the one before it)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) acc[qt][rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[rt], qh[qt], acc[qt][rt], 0, 0, 0);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) acc[qt][rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl[rt], qh[qt], acc[qt][rt], 0, 0, 0);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) acc[qt][rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[rt], ql[qt], acc[qt][rt], 0, 0, 0);
        }
    };

    uint32_t buf = 0;
    request(b_lo, 0);
    for (uint32_t rb = b_lo; rb < b_hi; ++rb) {
        // Norms (and tag words) of the lane's rows, register group g of row block rt = rows 8 g + 4 h + 0 .. 3: aligned groups of four,
        // asked for here so that they have landed behind the K loop.  A group that starts beyond the chunk is not read (a block of 128
        // may end further behind the set than the arrays' padding of 64): +inf keeps its rows out, as does j < rows.
        u32x4 nx[2][4], tg[2][4];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t jg = rb * kWideTile + 64u * wr + 32u * rt + 8u * g + 4u * h;
                const u32x4 inf4 = {0x7F800000u, 0x7F800000u, 0x7F800000u, 0x7F800000u}, zero4 = {0u, 0u, 0u, 0u};
                nx[rt][g] = jg < p.rows ? *reinterpret_cast<const u32x4*>(p.bnorm + jg) : inf4;
                tg[rt][g] = zero4;
                if constexpr (TAG) tg[rt][g] = jg < p.rows ? *reinterpret_cast<const u32x4*>(p.btag + jg) : zero4;
            }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[qt][rt][v] = 0.f;
        for (uint32_t st = 0; st < stages; ++st) {
            landed();
            to_lds(buf, st);
            __syncthreads();
            if (st + 1u < stages) request(rb, st + 1u);
            else if (rb + 1u < b_hi) request(rb + 1u, 0u);
            products(buf);
            buf ^= 1u;
        }
        const float scale = -0.5f * (1.0f - kKnnWideSlack);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                f32x16 t;  // q.x - 0.5 (1 - c) |x|^2, the norm in one rounding
#pragma unroll
                for (int v = 0; v < 16; ++v) t[v] = __builtin_fmaf(scale, __uint_as_float(nx[rt][v >> 2][v & 3]), acc[qt][rt][v]);
                float m = fmaxf(fmaxf(t[0], t[1]), t[2]);
#pragma unroll
                for (int v = 3; v < 15; v += 2) m = fmaxf(fmaxf(m, t[v]), t[v + 1]);
                m = fmaxf(m, t[15]);
                if (__builtin_expect(__ballot(m >= thr[qt]) != 0ull, 0)) {
                    const uint32_t qv = q0 + 64u * wq + 32u * qt + r;  // (nothing passes beyond the batch: never here with qv >= nq)
                    const uint32_t j0 = rb * kWideTile + 64u * wr + 32u * rt + 4u * h;
                    uint32_t hits = 0;
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const uint32_t j = j0 + (uint32_t)((v & 3) + 8 * (v >> 2));
                        hits |= (t[v] >= thr[qt] && j < p.rows) ? 1u << v : 0u;  // (a pass-all threshold lets -inf through too)
                    }
                    if constexpr (TAG) {
                        uint32_t tm = 0;
#pragma unroll
                        for (int v = 0; v < 16; ++v) tm |= ((tg[rt][v >> 2][v & 3] & qtag[qt]) ? 1u : 0u) << v;
                        hits &= tm;
                    }
                    if (hits && qv < p.nq) {  // one returning atomic per lane with hits: the places of all of them at once (qv: an overflowed +inf value passes +inf)
                        uint32_t pos = atomicAdd(&p.count[qv], (uint32_t)__popc(hits));
                        do {
                            const uint32_t v = (uint32_t)__ffs((int)hits) - 1u;
                            hits &= hits - 1u;
                            if (pos < p.cap) p.cand[(size_t)qv * p.cap + pos] = p.row0 + j0 + (v & 3u) + 8u * (v >> 2);
                            else *p.overflow = 1u;
                            pos += 1u;
                        } while (hits);
                    }
                }
            }
        }
    }
}

// The exact distances of the rows the wide filter kept: one wavefront per query.  The query is staged once in LDS and read by broadcast;
// every lane takes one candidate row straight from global memory and runs L2Metric::Dist (support_func.h:107-128) in the scan kernels'
// operations and order -- four running sums over ascending 16-byte steps, then ((s0 + s1) + s2) + s3 --; the keys below the heap's root
// are offered in list order by lane 0; then the query's new threshold, with the wide slack.
// B = uint16_t (knn_half_wide.hip's filter): the rows are binary16, widened as they are loaded -- exact --; vec: 16-byte chunks of eight
// halves, two steps each, and 8 bytes for the last step of an odd count.
template <class B>
__global__ __launch_bounds__(64) void knn_wide_rescore_kernel(KnnRescoreParams p, int vec) {
    __shared__ float4 qs[kKnnWideMaxDim / 4];
    __shared__ uint64_t keys[64];
    __shared__ uint64_t new_root;
    const KnnParams& kp = p.k;
    const uint32_t qi = blockIdx.x, lane = threadIdx.x;
    const uint32_t cnt = min(p.count[qi], p.cap);
    if (cnt == 0) return;  // (threshold unchanged)
    const uint32_t steps = kp.dim >> 2;
    const float* qp = kp.q + (size_t)qi * kp.qstride;
    for (uint32_t c = lane; c < steps; c += 64u)
        qs[c] = vec ? reinterpret_cast<const float4*>(qp)[c] : make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]);
    uint64_t root = kp.heap[qi];
    __syncthreads();
    for (uint32_t e0 = 0; e0 < cnt; e0 += 64u) {
        const uint32_t e = e0 + lane;
        const bool valid = e < cnt;
        const uint32_t row = valid ? p.cand[(size_t)qi * p.cap + e] : p.cand[(size_t)qi * p.cap];  // (an idle lane: the list's first row again)
        const B* bp = knn_rows<B>(kp) + (size_t)row * kp.bstride;
        f32x2 s01{0.f, 0.f}, s23{0.f, 0.f};
        auto step = [&](const float4 b4, const float4 q4) {
            const f32x2 e01 = f32x2{b4.x, b4.y} - f32x2{q4.x, q4.y};
            const f32x2 e23 = f32x2{b4.z, b4.w} - f32x2{q4.z, q4.w};
            s01 = s01 + e01 * e01;
            s23 = s23 + e23 * e23;
        };
        if constexpr (!kKnnHalfRows<B>) {
#pragma unroll 8
            for (uint32_t c = 0; c < steps; ++c)
                step(vec ? reinterpret_cast<const float4*>(bp)[c] : make_float4(bp[4 * c], bp[4 * c + 1], bp[4 * c + 2], bp[4 * c + 3]), qs[c]);
        } else if (vec) {
            auto widen4 = [](uint32_t a, uint32_t b) {
                return make_float4(knn_widen((uint16_t)a), knn_widen((uint16_t)(a >> 16)), knn_widen((uint16_t)b), knn_widen((uint16_t)(b >> 16)));
            };
#pragma unroll 4
            for (uint32_t c = 0; c + 1u < steps; c += 2u) {
                const uint4 w = reinterpret_cast<const uint4*>(bp)[c >> 1];
                step(widen4(w.x, w.y), qs[c]);
                step(widen4(w.z, w.w), qs[c + 1u]);
            }
            if (steps & 1u) {
                const uint2 w = reinterpret_cast<const uint2*>(bp)[steps - 1u];
                step(widen4(w.x, w.y), qs[steps - 1u]);
            }
        } else {
#pragma unroll 8
            for (uint32_t c = 0; c < steps; ++c) step(knn_row_step(bp, c, false), qs[c]);
        }
        const float dist = ((s01.x + s01.y) + s23.x) + s23.y;
        const uint64_t key = ((uint64_t)knn_fkey(dist) << 32) | row;
        const bool self = kp.self_offset >= 0 && (uint64_t)row == (uint64_t)qi + (uint64_t)kp.self_offset;
        uint64_t m = __ballot(valid && !self && key < root);
        if (m) {  // (the whole wavefront)
            keys[lane] = key;
            __syncthreads();
            if (lane == 0) {
                do {
                    const uint64_t kv = keys[__ffsll((unsigned long long)m) - 1];
                    m &= m - 1ull;
                    if (kv < root) root = heap_replace_root(kp.heap + qi, kp.heap_stride, kp.k, kv);
                } while (m);
                new_root = root;
            }
            __syncthreads();
            root = new_root;
        }
    }
    if (lane == 0)
        p.rhs[qi] = root == ~0ull ? -__builtin_inff() : 0.5f * ((1.0f - kKnnWideSlack) * p.qnorm[qi] - knn_fkey_inv((uint32_t)(root >> 32)));
}

constexpr int kWideStage = 2;  // K steps per stage: 72 KB of LDS, two workgroups a CU
static_assert(kWideStage == 2, "knn_wide_filter_kernel_name spells the stage out");

template <bool TAG>
hipError_t knn_wide_filter_launch(const KnnFilterParams& p, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_wide_filter_kernel<kWideStage, TAG>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kWideLds<kWideStage>);  // (more than the 64 KB a launch may ask for unannounced)
    if (e != hipSuccess) return e;
    // grid: x = blocks of 128 queries, y = slabs of the chunk's blocks of 128 rows -- two workgroups of 4 wavefronts for every CU
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const unsigned gx = (p.nq + kWideTile - 1) / kWideTile, blocks = (p.rows + kWideTile - 1) / kWideTile;
    const unsigned want = 2u * (unsigned)cus;
    unsigned gy = gx >= want ? 1u : (want + gx - 1) / gx;
    if (gy > blocks) gy = blocks;
    hipLaunchKernelGGL((knn_wide_filter_kernel<kWideStage, TAG>), dim3(gx, gy), dim3(256), kWideLds<kWideStage>, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_knn_wide_filter(const KnnFilterParams& p, hipStream_t s) {
    if (p.nq == 0 || p.rows == 0) return hipSuccess;
    if (p.dp == 0 || (p.dp & 15u) || p.dp > kKnnWideMaxDim || (p.btag && !p.qtag)) return hipErrorInvalidValue;
    // the norms and tag words are read in aligned groups of four
    if ((reinterpret_cast<uintptr_t>(p.bnorm) & 15u) || (reinterpret_cast<uintptr_t>(p.btag) & 15u)) return hipErrorInvalidValue;
    return p.btag ? knn_wide_filter_launch<true>(p, s) : knn_wide_filter_launch<false>(p, s);
}
const char* knn_wide_filter_kernel_name(uint32_t dp, bool tagged) {
    if (dp == 0 || (dp & 15u) || dp > kKnnWideMaxDim) return nullptr;
    return tagged ? "knn_wide_filter_kernel<2, true>" : "knn_wide_filter_kernel<2, false>";
}

hipError_t launch_knn_wide_rescore(const KnnRescoreParams& p, hipStream_t s) {
    if (p.k.nq == 0) return hipSuccess;
    if (p.k.dim > kKnnWideMaxDim || (p.k.dim & 3u)) return hipErrorInvalidValue;
    const int vec = !(p.k.bstride & 3u) && !(p.k.qstride & 3u) && !(reinterpret_cast<uintptr_t>(p.k.base) & 15u) && !(reinterpret_cast<uintptr_t>(p.k.q) & 15u);
    hipLaunchKernelGGL(knn_wide_rescore_kernel<float>, dim3(p.k.nq), dim3(64), 0, s, p, vec);
    return hipGetLastError();
}

hipError_t launch_knn_half_wide_rescore(const KnnRescoreParams& p, hipStream_t s) {
    if (p.k.nq == 0) return hipSuccess;
    if (!p.k.base_h || p.k.dim > kKnnWideMaxDim || (p.k.dim & 3u)) return hipErrorInvalidValue;
    // (16-byte chunks of eight halves: a table at a stride of whole chunks; the query's float4 steps as above)
    const int vec = !(p.k.bstride & 7u) && !(p.k.qstride & 3u) && !(reinterpret_cast<uintptr_t>(p.k.base_h) & 15u) && !(reinterpret_cast<uintptr_t>(p.k.q) & 15u);
    hipLaunchKernelGGL(knn_wide_rescore_kernel<uint16_t>, dim3(p.k.nq), dim3(64), 0, s, p, vec);
    return hipGetLastError();
}

}  // namespace gbnns
