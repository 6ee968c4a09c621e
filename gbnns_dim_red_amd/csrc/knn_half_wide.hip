// knn_half_wide.hip -- the matrix-core filter of the exact kNN for binary16 rows wider than 128 dims (gist kept as halves: 960, glove: 300 /
// 200) on gfx950 (MI355X): gbnns_exact_knn_half / gbnns_index_exact_knn_half with "knn_half_wide" set, L2, 128 < d <= 1024, d % 4 == 0,
// k <= 512 (heaps).
//
// knn_half.hip's arithmetic on knn_wide.hip's division of work.  The arithmetic: a binary16 row IS an exact operand of
// v_mfma_f32_32x32x16_f16 and lies in memory in A-fragment order, so the table is swept in place, at its own stride, nothing packed; the
// float32 query is launch_knn_half_qsplit's image, q s = hi + lo + r with s = 2^t per query; two products per K step (x.hi, x.lo), each
// exact in f32; the scale is undone and the norm added behind the K loop, t = fma(acc, 1 / s, -0.5 (1 - c) |x|^2), and a pair is kept when
// t >= rhs[query] = 0.5 ((1 - c) |q|^2 - T_q), c = kKnnWideSlack.  Kept rows get L2Metric::Dist in the scan's operations and order
// (knn_wide.hip's rescore, its binary16 instance) and are offered to the scan's heaps.
//
// The division of work: a workgroup of 4 wavefronts owns a tile of 128 queries x 128 rows of the chunk, wavefront (wq, wr) the 64 x 64
// sub-tile of query half wq and row half wr as four 32 x 32 accumulators that start at zero.  blockIdx.x picks the 128 queries, blockIdx.y
// a slab of the chunk's blocks of 128 rows.  Per row block K is looped over dp = round_up(d, 16) in stages of KS K steps.  A row's stage
// is 32 KS contiguous bytes of the table (2 KS chunks of eight halves), a query's 64 KS contiguous bytes of the split image (per group of
// 8 dims 16 bytes of hi, then 16 of lo): both go global memory -> registers -> LDS, two LDS buffers in turn, the loads hand-issued
// (knn_sweep.h says why) and the next stage's requested right behind the barrier, in front of the current stage's products.  One barrier
// per stage is enough, as in knn_wide.hip: stage g is written to buffer g & 1 behind the barrier of stage g - 1, which every wavefront
// reaches only behind its products of stage g - 2, the last readers of that buffer.  The LDS pitches are odd multiples of 16 bytes,
// 32 KS + 16 for rows and 64 KS + 16 for queries, so the fragment reads of eight consecutive lanes cover all 32 banks; two buffers take
// 256 (96 KS + 32) bytes: 56 KB at KS = 2 (two workgroups a CU), 104 KB at KS = 4 (one).
// No byte beyond a row's last 16-byte chunk of dimensions (last_chunk) is requested -- the table has no tail padding and its last row ends
// the allocation: a unit beyond it asks for the row's first chunk instead and is written to LDS as zeros.  (Columns d .. 8 (last_chunk + 1)
// - 1 inside the last chunk -- d % 8 == 4, a stride of whole chunks: a handle's padded rows -- meet zero query halves.)
// Epilogue: knn_wide.hip's hit path (C layout: register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h, column r -- a lane's 16 values
// of a tile belong to ONE query, so 1 / s is one register per query block): max over the 16 values, one compare, ballot; a returning
// atomicAdd per lane with hits, ids stored while pos < cap, the overflow flag otherwise; rows beyond the chunk refused by j < rows; TAG
// instances fetch the tag words with the norms, in aligned groups of four guarded by jg < rows, and test them where hits are counted.
//
// Error bound for dp <= 1024, on the scale S = |q|^2 + |x|^2 (|a - Dist| <= c S must hold for a = |q|^2 + |x|^2 - 2 q.x as computed;
// sum |q_k x_k| <= |q||x| <= S / 2):
//   rows          none: x is the operand.
//   dropped r     |r_k| <= 2^-22 |q_k s| (two round-to-nearest binary16 steps of 11 bits): 2^-22 sum |x_k q_k| on the dot product, 2^-21 S on
//                 a = 4.8e-7 S; plus an absolute 2^-25 where lo is subnormal: sum |x_k| 2^-25 / s <= 2^-37 sqrt(d) |x||q| (knn_half.hip), on
//                 a <= 2^-37 sqrt(d) S = 2^-32 S at d = 1024.
//   accumulation  2 dp / 16 matrix instructions of 16 products each, taken as one add per product that may truncate (2^-23) against a
//                 partial sum <= sum |x_k q_k s|: 2 dp 2^-23 sum |x_k q_k| on the dot product, 2 dp 2^-23 S on a: 2.4e-4 S at dp = 1024.
//                 The accumulators start at zero, so no step rounds against |x|^2.
//   the fma       acc / s is exact (a power of two, normal range); one rounding of q.x - 0.5 (1 - c) |x|^2, a value of at most S / 2, and one of
//                 the product -0.5 (1 - c) |x|^2 that enters it: 2 * 2^-24 S on a.
//   norms         |q|^2 and |x|^2 summed in float32, d products and d adds each: <= d 2^-23 of each norm, d 2^-23 S together: 1.2e-4 S.
//   Dist          the reference distance's own rounding against the real value, <= (d / 4 + 3) 2^-23 Dist with Dist <= 2 S:
//                 (d / 4 + 3) 2^-22 S = 6.2e-5 S.
//   threshold     rhs = 0.5 ((1 - c) |q|^2 - T) rounds twice against values <= S (the halving is exact): <= 2^-22 S on a.
// Sum at d = dp = 1024: 4.29e-4 S.  c = 2^-10 = 9.77e-4 leaves a factor 2.2; the static_assert pins that sum at kKnnWideMaxDim with 1.5.
// knn_half.hip's assumptions stay: the matrix pipe keeps subnormal binary16 operands, and a query with |q|^2 outside 2^-96 .. 2^96 sends
// the whole call to the exact scan (queries_covered in graph_api.cpp) before this kernel is reached.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gbnns {

namespace {

constexpr float kKnnHalfWideBound = 2.0f * kKnnWideMaxDim / 8388608.0f      // accumulation
                                    + 1.0f * kKnnWideMaxDim / 8388608.0f    // both norms
                                    + (kKnnWideMaxDim / 4 + 3) / 4194304.0f  // the reference distance
                                    + 1.0f / 2097152.0f + 1.0f / 4294967296.0f  // the dropped query remainder, the subnormal lo parts
                                    + 2.0f / 16777216.0f + 1.0f / 4194304.0f;   // the fma and its norm product, the threshold
static_assert(kKnnWideSlack >= 1.5f * kKnnHalfWideBound, "kKnnWideSlack no longer covers the half-row wide filter's error bound at its longest row with a factor 1.5");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kTile = 128;  // queries, and rows, of a workgroup's tile

template <int KS>
constexpr uint32_t kRowPitch = 32u * KS + 16u;  // bytes of one row's stage in LDS
template <int KS>
constexpr uint32_t kQueryPitch = 64u * KS + 16u;  // ... of one split query's
template <int KS>
constexpr uint32_t kHalfWideLds = 2u * kTile * (kRowPitch<KS> + kQueryPitch<KS>);  // two buffers of two operands

// KS = K steps of 16 dims per stage
template <int KS, bool TAG>
__global__ __launch_bounds__(256) void knn_half_wide_filter_kernel(KnnHalfSweepParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char half_wide_smem[];
    constexpr uint32_t RP = kRowPitch<KS>, QP = kQueryPitch<KS>, ROWS = kTile * RP, BUF = kTile * (RP + QP);  // a buffer: the rows' stage, then the queries'
    constexpr int LR = KS, LQ = 2 * KS;                // 16-byte requests per thread and stage: 128 rows x 2 KS, 128 queries x 4 KS, over 256 threads
    constexpr uint32_t RU = 2u * KS, QU = 4u * KS;     // 16-byte units of a row's / a query's stage
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint32_t wq = wave & 1u, wr = wave >> 1;
    const uint32_t q0 = blockIdx.x * kTile;
    const uint32_t ksteps = p.dp >> 4, stages = (ksteps + KS - 1) / KS;
    const size_t qbytes = (size_t)p.dp * 4, rbytes = (size_t)p.stride * 2;
    const uint32_t blocks = (p.rows + kTile - 1) / kTile;
    const uint32_t per = (blocks + gridDim.y - 1) / gridDim.y;
    const uint32_t b_lo = blockIdx.y * per, b_hi = min(blocks, b_lo + per);
    if (b_lo >= b_hi) return;  // (the whole workgroup)

    // what this thread moves per stage: unit i = row / query l..[i] of the tile, 16-byte unit c..[i] of its stage (consecutive threads:
    // consecutive units of a row)
    uint32_t lrow[LR], cr[LR], lq[LQ], cq[LQ];
    const char* qsrc[LQ];
#pragma unroll
    for (int i = 0; i < LR; ++i) {
        const uint32_t u = tid + 256u * i;
        lrow[i] = u / RU;
        cr[i] = u % RU;
    }
#pragma unroll
    for (int i = 0; i < LQ; ++i) {
        const uint32_t u = tid + 256u * i;
        lq[i] = u / QU;
        cq[i] = u % QU;
        const uint32_t qi = q0 + lq[i];
        qsrc[i] = reinterpret_cast<const char*>(p.qsplit) + (size_t)(qi < p.nq ? qi : 0u) * qbytes;  // (a query beyond the batch keeps nothing: its threshold)
    }
    // the thresholds, 1 / s and tag words of the lane's queries: one per 32 x 32 tile column block
    float thr[2], qinv[2];
    uint32_t qtag[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const uint32_t qv = q0 + 64u * wq + 32u * qt + r;
        thr[qt] = qv < p.nq ? p.rhs[qv] : __builtin_inff();
        qinv[qt] = qv < p.nq ? p.qinv[qv] : 0.f;
        qtag[qt] = 0u;
        if constexpr (TAG) qtag[qt] = qv < p.nq ? p.qtag[qv] : 0u;
    }

    // a stage's units on their way: rows' then queries'.  A row's unit is chunk 2 KS st + cr of the row, live up to last_chunk; a query's
    // unit lies in K step KS st + cq / 4 of the split image, live below dp.  A unit that is not live is requested at the row's / query's
    // first 16 bytes instead -- readable -- and written as zeros.
    u32x4 stg[LR + LQ];
    auto request = [&](uint32_t rb, uint32_t st) {
#pragma unroll
        for (int i = 0; i < LR; ++i) {
            const uint32_t j = rb * kTile + lrow[i], c = st * RU + cr[i];
            const char* xp = reinterpret_cast<const char*>(p.base) + (size_t)(j < p.rows ? j : 0u) * rbytes + (c <= p.last_chunk ? 16u * c : 0u);  // (rows beyond the chunk read row 0; refused below)
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(stg[i]) : "v"(xp));
        }
#pragma unroll
        for (int i = 0; i < LQ; ++i) {
            const bool live = st * KS + (cq[i] >> 2) < ksteps;
            const char* qp = qsrc[i] + (live ? (size_t)st * (64u * KS) + 16u * cq[i] : 0u);
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(stg[LR + i]) : "v"(qp));
        }
    };
    auto landed = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(stg[0]));
#pragma unroll
        for (int i = 1; i < LR + LQ; ++i) asm volatile("" : "+v"(stg[i]));
    };
    auto to_lds = [&](uint32_t buf, uint32_t st) {
        unsigned char* xb = half_wide_smem + buf * BUF;
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < LR; ++i)
            *reinterpret_cast<u32x4*>(xb + lrow[i] * RP + 16u * cr[i]) = st * RU + cr[i] <= p.last_chunk ? stg[i] : zero;
#pragma unroll
        for (int i = 0; i < LQ; ++i)
            *reinterpret_cast<u32x4*>(xb + ROWS + lq[i] * QP + 16u * cq[i]) = st * KS + (cq[i] >> 2) < ksteps ? stg[LR + i] : zero;
    };

    f32x16 acc[2][2];  // [query block][row block] of the wavefront's 64 x 64
    auto products = [&](uint32_t buf) {
        const unsigned char* xb = half_wide_smem + buf * BUF + (64u * wr + r) * RP + 16u * h;
        const unsigned char* qb = half_wide_smem + buf * BUF + ROWS + (64u * wq + r) * QP + 32u * h;
#pragma unroll
        for (int s = 0; s < KS; ++s) {  // fragments of K step s: the row's chunk 2 s + h; the query's group 2 s + h of 8 dims, hi then lo
            f16x8 x[2], qh[2], ql[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                x[b] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(xb + 32u * b * RP + 32u * s));
                qh[b] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(qb + 32u * b * QP + 64u * s));
                ql[b] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(qb + 32u * b * QP + 64u * s + 16u));
            }
            // (four accumulators in turn: no product waits for the one before it)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) acc[qt][rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[rt], qh[qt], acc[qt][rt], 0, 0, 0);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) acc[qt][rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[rt], ql[qt], acc[qt][rt], 0, 0, 0);
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
                const uint32_t jg = rb * kTile + 64u * wr + 32u * rt + 8u * g + 4u * h;
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
        for (int rt = 0; rt < 2; ++rt) {
            f32x16 cx;  // -0.5 (1 - c) |x|^2 of the lane's 16 rows
#pragma unroll
            for (int v = 0; v < 16; ++v) cx[v] = scale * __uint_as_float(nx[rt][v >> 2][v & 3]);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                f32x16 t;  // q.x - 0.5 (1 - c) |x|^2: the scale undone and the norm added in one rounding
#pragma unroll
                for (int v = 0; v < 16; ++v) t[v] = __builtin_fmaf(acc[qt][rt][v], qinv[qt], cx[v]);
                float m = fmaxf(fmaxf(t[0], t[1]), t[2]);
#pragma unroll
                for (int v = 3; v < 15; v += 2) m = fmaxf(fmaxf(m, t[v]), t[v + 1]);
                m = fmaxf(m, t[15]);
                if (__builtin_expect(__ballot(m >= thr[qt]) != 0ull, 0)) {
                    const uint32_t qv = q0 + 64u * wq + 32u * qt + r;  // (nothing passes beyond the batch: never here with qv >= nq)
                    const uint32_t j0 = rb * kTile + 64u * wr + 32u * rt + 4u * h;
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
                    if (hits && qv < p.nq) {  // one returning atomic per lane with hits: the places of all of them at once
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

// K steps per stage: 2.  Measured on an MI355X by tools/knn_half_wide_timing.py against a build with -DGBNNS_HALF_WIDE_STAGE=4 in the same job
// (profiles/knn_half_wide_timing.txt has both runs): whole calls of 25.3 against 27.0 ms at 10^5 x 960 with 10 000 queries, 30.2 against
// 32.0 ms at 10^6 x 960 with 1 000, 42.2 against 48.0 ms at 10^6 x 300, 105 against 127 ms for the 48-NN self lists of 10^5 x 960.
#ifndef GBNNS_HALF_WIDE_STAGE
#define GBNNS_HALF_WIDE_STAGE 2
#endif
constexpr int kHalfWideStage = GBNNS_HALF_WIDE_STAGE;
static_assert(kHalfWideStage == 2 || kHalfWideStage == 4, "knn_half_wide_filter_kernel_name spells the stage out");

template <bool TAG>
hipError_t half_wide_launch(const KnnHalfSweepParams& p, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_half_wide_filter_kernel<kHalfWideStage, TAG>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kHalfWideLds<kHalfWideStage>);  // (KS = 4: more than the 64 KB a launch may ask for unannounced)
    if (e != hipSuccess) return e;
    // grid: x = blocks of 128 queries, y = slabs of the chunk's blocks of 128 rows -- two workgroups of 4 wavefronts for every CU
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const unsigned gx = (p.nq + kTile - 1) / kTile, blocks = (p.rows + kTile - 1) / kTile;
    const unsigned want = 2u * (unsigned)cus;
    unsigned gy = gx >= want ? 1u : (want + gx - 1) / gx;
    if (gy > blocks) gy = blocks;
    hipLaunchKernelGGL((knn_half_wide_filter_kernel<kHalfWideStage, TAG>), dim3(gx, gy), dim3(256), kHalfWideLds<kHalfWideStage>, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_knn_half_wide_filter(const KnnHalfSweepParams& p, hipStream_t s) {
    if (p.nq == 0 || p.rows == 0) return hipSuccess;
    if (p.dp == 0 || (p.dp & 15u) || p.dp > kKnnWideMaxDim || (p.btag && !p.qtag)) return hipErrorInvalidValue;
    // what keeps every 16-byte request inside its row: an aligned table at a stride of whole chunks that holds the last chunk read
    if ((p.stride & 7u) || (reinterpret_cast<uintptr_t>(p.base) & 15u) || 8u * (p.last_chunk + 1u) > p.stride || 8u * (p.last_chunk + 1u) > p.dp)
        return hipErrorInvalidValue;
    // the norms and tag words are read in aligned groups of four
    if ((reinterpret_cast<uintptr_t>(p.bnorm) & 15u) || (reinterpret_cast<uintptr_t>(p.btag) & 15u)) return hipErrorInvalidValue;
    return p.btag ? half_wide_launch<true>(p, s) : half_wide_launch<false>(p, s);
}
const char* knn_half_wide_filter_kernel_name(uint32_t dp, bool tagged) {
    if (dp == 0 || (dp & 15u) || dp > kKnnWideMaxDim) return nullptr;
    if (kHalfWideStage == 2) return tagged ? "knn_half_wide_filter_kernel<2, true>" : "knn_half_wide_filter_kernel<2, false>";
    return tagged ? "knn_half_wide_filter_kernel<4, true>" : "knn_half_wide_filter_kernel<4, false>";
}

}  // namespace gbnns
