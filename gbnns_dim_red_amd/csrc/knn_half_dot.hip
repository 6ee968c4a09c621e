// knn_half_dot.hip -- the matrix-core filter of the exact kNN under the negative dot (angular sets, MIPS) for binary16 rows on gfx950
// (MI355X): gbnns_exact_knn_half / gbnns_index_exact_knn_half with GBNNS_METRIC_NEG_DOT and "knn_half_dot" set, d % 8 == 0, 8 <= d <= 1024,
// k <= 512 (heaps), n > 4 k.  The last cell of the table: float rows have knn_dot.hip, binary16 rows under L2 knn_half.hip / knn_half_wide.hip.
//
// knn_half_wide.hip's operands under knn_dot.hip's pass rule.  The operands: a binary16 row IS an exact operand of
// v_mfma_f32_32x32x16_f16 and lies in memory in A-fragment order, so the table is swept in place, at its own stride, nothing packed; the
// float32 query is launch_knn_half_qsplit's image, q s = hi + lo + r with s = 2^t per query; two products per K step (x.hi, x.lo), each
// exact in f32 (knn_dot.hip's bf16 images need three).  The rule: Dist = -q.x has no norm to fold in, and the error of q.x on the matrix
// cores scales with P = |q||x|, whatever the distance.  A row is kept when
//     fma(cq, ux, acc * (1 / s)) >= thr     acc = s q.x on the matrix cores, accumulators from zero; the product by 1 / s is exact
//                                           ux  = an upper bound of |x|   (launch_knn_dot_bounds over launch_knn_half_norms' sums)
//                                           cq  = c * (an upper bound of |q|), c = kKnnWideSlack = 2^-10 (... over the qsplit kernel's sums)
//                                           thr = -T_q, T_q the query's current exact k-th distance, -inf while the heap is not full
// Kept rows get Angular::Dist on the widened row in the scan's operations and order (knn_dot.hip's rescore, its binary16 instance) and are
// offered to the scan's heaps.
// (The scale is NOT folded into per-query registers -- acc + (cq s) ux >= thr s would save the multiply, but thr = -T_q may be any float,
// near zero too, and thr s with s down to 2^-36 then leaves the normal range: the exact multiply by 1 / s stays.)
//
// Division of work: knn_half_wide.hip's.  A workgroup of 4 wavefronts owns a tile of 128 queries x 128 rows of the chunk, wavefront
// (wq, wr) the 64 x 64 sub-tile of query half wq and row half wr as four 32 x 32 accumulators that start at zero.  blockIdx.x picks the 128
// queries, blockIdx.y a slab of the chunk's blocks of 128 rows.  Per row block K is looped over dp = round_up(d, 16) in stages of KS K
// steps, down to one stage with one live K step at d = 8 .. 16.  A row's stage is 32 KS contiguous bytes of the table (2 KS chunks of
// eight halves), a query's 64 KS contiguous bytes of the split image (per group of 8 dims 16 bytes of hi, then 16 of lo): both go global
// memory -> registers -> LDS, two LDS buffers in turn, the loads hand-issued (knn_sweep.h says why) and the next stage's requested right
// behind the barrier, in front of the current stage's products.  One barrier per stage is enough: stage g is written to buffer g & 1 behind
// the barrier of stage g - 1, which every wavefront reaches only behind its products of stage g - 2, the last readers of that buffer.  The
// LDS pitches are odd multiples of 16 bytes, 32 KS + 16 for rows and 64 KS + 16 for queries, so the fragment reads of eight consecutive
// lanes cover all 32 banks; two buffers take 256 (96 KS + 32) bytes: 56 KB at KS = 2 (two workgroups a CU), 104 KB at KS = 4 (one).
// No byte beyond a row's last 16-byte chunk of dimensions (last_chunk) is requested -- the table has no tail padding and its last row ends
// the allocation: a unit beyond it asks for the row's first chunk instead and is written to LDS as zeros.  d % 8 == 0: a row's last chunk
// holds dimensions only.
// The staging code is a COPY of knn_half_wide_filter_kernel's, for the reason knn_dot.hip gives for its copy: it is a set of lambdas over
// the kernel's locals, and a shared form would put the measured kernels' register allocation behind a struct of references.
// The epilogue is knn_dot.hip's with the scale undone.  C layout: register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h, column r -- a
// lane's 16 values of a tile belong to ONE query, so 1 / s, cq and thr are per lane and ux varies with v: fetched, with the tag words, in
// aligned groups of four at the head of the row block.  A group that starts behind the chunk is not read and gets ux = -inf:
// fma(cq, -inf, .) = -inf fails every threshold but -inf, and a -inf threshold's rows are refused by j < rows (+inf, the L2 kernels' choice
// for their norms, would pass every threshold and send every partial block down the hit path); launch_knn_dot_bounds writes -inf behind
// the set's last row too.  cq = 0 and 1 / s = 0 -- a query beyond the batch -- give fma(0, -inf, 0) = NaN or 0 against thr = +inf: both
// compare false.  Then knn_sweep.h's hit path: max over the 16 values, one compare, ballot; a returning atomicAdd per lane with hits, ids
// stored while pos < cap, the overflow flag otherwise; TAG instances test the tag words where hits are counted.
//
// Error bound for dp <= 1024 on the scale P = |q||x| (|acc / s - q.x as Angular::Dist sums it| <= b P must hold with b < c;
// sum |q_k x_k| <= P):
//   rows          none: x is the operand.
//   dropped r     |r_k| <= 2^-22 |q_k s| (two round-to-nearest binary16 steps of 11 bits): 2^-22 sum |x_k q_k| <= 2^-22 P = 2.4e-7 P.
//   subnormal lo  an absolute 2^-25 per coordinate where lo is subnormal: sum |x_k| 2^-25 / s with 1 / s <= 2^-12 max |q_k| and
//                 sum |x_k| <= sqrt(d) |x| (knn_half.hip): <= 2^-37 sqrt(d) P = 2^-32 P at d = 1024.
//   products      exact: 11 x 11 significand bits; a nonzero product is at least 2^-24 2^-24, far inside the normal range.
//   accumulation  2 dp / 16 matrix instructions of 16 products each, taken as one add per product that may truncate (2^-23) against a
//                 partial sum <= sum |x_k q_k s|: 2 dp 2^-23 P = 2.44e-4 P at dp = 1024.  The accumulators start at zero.
//   the scale     acc / s is a product by a power of two: exact while the result is normal; a result below 2^-126 loses less than 2^-126
//                 against c P >= 2^-106 (the range below).
//   reference     Angular::Dist rounds each product once and adds it to one of eight running sums (d / 8 adds), then three levels of
//                 pairwise adds: <= (d / 8 + 3) roundings a path, taken at 2^-23 each: (d / 8 + 3) 2^-23 P = 1.56e-5 P.  The negation is exact.
//   the fma       one rounding of q.x + cq ux, a value of at most (1 + b + c) P: taken as 2^-23 P = 1.2e-7 P.
//   norm bounds   nothing on this side: ux >= |x| and cq >= c |q| by construction (below), so cq ux >= c P.
// Sum at d = dp = 1024: 2.60e-4 P.  c = 2^-10 = 9.77e-4 leaves a factor 3.7; the static_assert pins the sum at kKnnWideMaxDim with 1.5.
//
// The bounds ux, uq come from launch_knn_dot_bounds, sqrt(n2) kDotNormUp with kDotNormUp = 1 + 2^-12 (knn_dot.hip), over sums that are NOT
// knn_pack_kernel's: the rows' n2 is knn_half_norm_kernel's -- the same serial order, one thread a row, but the widened squares are exact
// (22 bits), so only the d adds round, all terms >= 0: n2 >= |x|^2 (1 - d 2^-24); the queries' n2 is knn_half_qsplit_kernel's -- serial
// again, d products and d adds that round once each, a product's rounding entering one term of the sum: n2 >= |q|^2 (1 - (d + 1) 2^-24).
// So |v| <= sqrt(n2) (1 + (d + 1) 2^-25) for both, to first order; the correctly rounded sqrt and the product by the factor round once
// each (2^-24).  knn_dot.hip pins kDotNormUp against four times that sum beside its own.
// Range: all terms are relative and assume normal float32 arithmetic.  A call is covered when every n2 (rows and queries) lies in
// [2^-96, 2^96] -- launch_knn_dot_bounds' flag, raised for a zero or non-finite norm too; the qsplit kernel's own test (queries_covered in
// graph_api.cpp) is asked before: q.x is then below 2^96, a query square lost to underflow is below 2^-126 against n2 >= 2^-96, and a row's
// squares (>= 2^-48 where nonzero) do not underflow.  A call that is not covered is served by the exact scan: for every finite input the
// answer is the scan's.  knn_half.hip's assumption stays: the matrix pipe keeps subnormal binary16 operands.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gbnns {

namespace {

constexpr float kKnnHalfDotBound = 2.0f * kKnnWideMaxDim / 8388608.0f        // accumulation
                                   + (kKnnWideMaxDim / 8 + 3) / 8388608.0f    // the reference dot
                                   + 1.0f / 4194304.0f + 1.0f / 4294967296.0f  // the dropped query remainder, the subnormal lo parts
                                   + 1.0f / 8388608.0f;                       // the fma
static_assert(kKnnWideSlack >= 1.5f * kKnnHalfDotBound, "kKnnWideSlack no longer covers the half-row dot filter's error bound at its longest row with a factor 1.5");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kTile = 128;  // queries, and rows, of a workgroup's tile

template <int KS>
constexpr uint32_t kRowPitch = 32u * KS + 16u;  // bytes of one row's stage in LDS
template <int KS>
constexpr uint32_t kQueryPitch = 64u * KS + 16u;  // ... of one split query's
template <int KS>
constexpr uint32_t kHalfDotLds = 2u * kTile * (kRowPitch<KS> + kQueryPitch<KS>);  // two buffers of two operands

// KS = K steps of 16 dims per stage
template <int KS, bool TAG>
__global__ __launch_bounds__(256) void knn_half_dot_filter_kernel(KnnHalfSweepParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char half_dot_smem[];
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

    // what this thread moves per stage: unit i = row lrow[i] / query lq[i] of the tile, 16-byte unit ur[i] / uq[i] of its stage
    // (consecutive threads: consecutive units of a row)
    uint32_t lrow[LR], ur[LR], lq[LQ], uq[LQ];
    const char* qsrc[LQ];
#pragma unroll
    for (int i = 0; i < LR; ++i) {
        const uint32_t u = tid + 256u * i;
        lrow[i] = u / RU;
        ur[i] = u % RU;
    }
#pragma unroll
    for (int i = 0; i < LQ; ++i) {
        const uint32_t u = tid + 256u * i;
        lq[i] = u / QU;
        uq[i] = u % QU;
        const uint32_t qi = q0 + lq[i];
        qsrc[i] = reinterpret_cast<const char*>(p.qsplit) + (size_t)(qi < p.nq ? qi : 0u) * qbytes;  // (a query beyond the batch keeps nothing: its threshold)
    }
    // the thresholds -T, 1 / s, slack factors c |q| and tag words of the lane's queries: one per 32 x 32 tile column block
    float thr[2], qinv[2], cq[2];
    uint32_t qtag[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const uint32_t qv = q0 + 64u * wq + 32u * qt + r;
        thr[qt] = qv < p.nq ? p.rhs[qv] : __builtin_inff();
        qinv[qt] = qv < p.nq ? p.qinv[qv] : 0.f;
        cq[qt] = qv < p.nq ? p.cq[qv] : 0.f;
        qtag[qt] = 0u;
        if constexpr (TAG) qtag[qt] = qv < p.nq ? p.qtag[qv] : 0u;
    }

    // a stage's units on their way: rows' then queries'.  A row's unit is chunk 2 KS st + ur of the row, live up to last_chunk; a query's
    // unit lies in K step KS st + uq / 4 of the split image, live below dp.  A unit that is not live is requested at the row's / query's
    // first 16 bytes instead -- readable -- and written as zeros.
    u32x4 stg[LR + LQ];
    auto request = [&](uint32_t rb, uint32_t st) {
#pragma unroll
        for (int i = 0; i < LR; ++i) {
            const uint32_t j = rb * kTile + lrow[i], c = st * RU + ur[i];
            const char* xp = reinterpret_cast<const char*>(p.base) + (size_t)(j < p.rows ? j : 0u) * rbytes + (c <= p.last_chunk ? 16u * c : 0u);  // (rows beyond the chunk read row 0; refused below)
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(stg[i]) : "v"(xp));
        }
#pragma unroll
        for (int i = 0; i < LQ; ++i) {
            const bool live = st * KS + (uq[i] >> 2) < ksteps;
            const char* qp = qsrc[i] + (live ? (size_t)st * (64u * KS) + 16u * uq[i] : 0u);
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(stg[LR + i]) : "v"(qp));
        }
    };
    auto landed = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(stg[0]));
#pragma unroll
        for (int i = 1; i < LR + LQ; ++i) asm volatile("" : "+v"(stg[i]));
    };
    auto to_lds = [&](uint32_t buf, uint32_t st) {
        unsigned char* xb = half_dot_smem + buf * BUF;
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < LR; ++i)
            *reinterpret_cast<u32x4*>(xb + lrow[i] * RP + 16u * ur[i]) = st * RU + ur[i] <= p.last_chunk ? stg[i] : zero;
#pragma unroll
        for (int i = 0; i < LQ; ++i)
            *reinterpret_cast<u32x4*>(xb + ROWS + lq[i] * QP + 16u * uq[i]) = st * KS + (uq[i] >> 2) < ksteps ? stg[LR + i] : zero;
    };

    f32x16 acc[2][2];  // [query block][row block] of the wavefront's 64 x 64
    auto products = [&](uint32_t buf) {
        const unsigned char* xb = half_dot_smem + buf * BUF + (64u * wr + r) * RP + 16u * h;
        const unsigned char* qb = half_dot_smem + buf * BUF + ROWS + (64u * wq + r) * QP + 32u * h;
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
        // Norm bounds (and tag words) of the lane's rows, register group g of row block rt = rows 8 g + 4 h + 0 .. 3: aligned groups of
        // four, asked for here so that they have landed behind the K loop.  A group that starts beyond the chunk is not read (a block of
        // 128 may end further behind the set than the arrays' padding of 64): -inf.
        u32x4 ux[2][4], tg[2][4];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t jg = rb * kTile + 64u * wr + 32u * rt + 8u * g + 4u * h;
                const u32x4 ninf4 = {0xFF800000u, 0xFF800000u, 0xFF800000u, 0xFF800000u}, zero4 = {0u, 0u, 0u, 0u};
                ux[rt][g] = jg < p.rows ? *reinterpret_cast<const u32x4*>(p.bnorm + jg) : ninf4;
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
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                f32x16 t;  // q.x + c |q||x|: the scale undone (exact), then the slack in the fma's one rounding
#pragma unroll
                for (int v = 0; v < 16; ++v) t[v] = __builtin_fmaf(cq[qt], __uint_as_float(ux[rt][v >> 2][v & 3]), acc[qt][rt][v] * qinv[qt]);
                float m = fmaxf(fmaxf(t[0], t[1]), t[2]);  // (fmaxf drops a NaN: cq = 0 against -inf)
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

// K steps per stage: 2.  Measured on an MI355X by tools/knn_half_dot_timing.py against a build with -DGBNNS_HALF_DOT_STAGE=4 in the same job
// (profiles/knn_half_dot_timing.txt has both runs): whole calls of 24.6 against 26.4 ms at 10^5 x 960 with 10 000 queries, 32.8 against
// 34.6 ms at 10^6 x 960 with 1 000 (k = 100), 31.1 against 38.2 ms at 10^6 x 200, 21.0 against 27.0 ms at 10^6 x 96, 103 against 127 ms for
// the 48-NN self lists of 10^5 x 960.
#ifndef GBNNS_HALF_DOT_STAGE
#define GBNNS_HALF_DOT_STAGE 2
#endif
constexpr int kHalfDotStage = GBNNS_HALF_DOT_STAGE;
static_assert(kHalfDotStage == 2 || kHalfDotStage == 4, "knn_half_dot_filter_kernel_name spells the stage out");

template <bool TAG>
hipError_t half_dot_launch(const KnnHalfSweepParams& p, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_half_dot_filter_kernel<kHalfDotStage, TAG>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kHalfDotLds<kHalfDotStage>);  // (KS = 4: more than the 64 KB a launch may ask for unannounced)
    if (e != hipSuccess) return e;
    // grid: x = blocks of 128 queries, y = slabs of the chunk's blocks of 128 rows -- two workgroups of 4 wavefronts for every CU
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const unsigned gx = (p.nq + kTile - 1) / kTile, blocks = (p.rows + kTile - 1) / kTile;
    const unsigned want = 2u * (unsigned)cus;
    unsigned gy = gx >= want ? 1u : (want + gx - 1) / gx;
    if (gy > blocks) gy = blocks;
    hipLaunchKernelGGL((knn_half_dot_filter_kernel<kHalfDotStage, TAG>), dim3(gx, gy), dim3(256), kHalfDotLds<kHalfDotStage>, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_knn_half_dot_filter(const KnnHalfSweepParams& p, hipStream_t s) {
    if (p.nq == 0 || p.rows == 0) return hipSuccess;
    if (p.dp == 0 || (p.dp & 15u) || p.dp > kKnnWideMaxDim || !p.cq || (p.btag && !p.qtag)) return hipErrorInvalidValue;
    // what keeps every 16-byte request inside its row: an aligned table at a stride of whole chunks that holds the last chunk read
    if ((p.stride & 7u) || (reinterpret_cast<uintptr_t>(p.base) & 15u) || 8u * (p.last_chunk + 1u) > p.stride || 8u * (p.last_chunk + 1u) > p.dp)
        return hipErrorInvalidValue;
    // the norm bounds and tag words are read in aligned groups of four
    if ((reinterpret_cast<uintptr_t>(p.bnorm) & 15u) || (reinterpret_cast<uintptr_t>(p.btag) & 15u)) return hipErrorInvalidValue;
    return p.btag ? half_dot_launch<true>(p, s) : half_dot_launch<false>(p, s);
}
const char* knn_half_dot_filter_kernel_name(uint32_t dp, bool tagged) {
    if (dp == 0 || (dp & 15u) || dp > kKnnWideMaxDim) return nullptr;
    if (kHalfDotStage == 2) return tagged ? "knn_half_dot_filter_kernel<2, true>" : "knn_half_dot_filter_kernel<2, false>";
    return tagged ? "knn_half_dot_filter_kernel<4, true>" : "knn_half_dot_filter_kernel<4, false>";
}

}  // namespace gbnns
