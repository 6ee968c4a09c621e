// knn_dot.hip -- the matrix-core filter of the exact kNN under the negative dot (angular sets, MIPS) for float rows on gfx950 (MI355X):
// gbnns_exact_knn / gbnns_exact_knn_tagged / gbnns_index_exact_knn with GBNNS_METRIC_NEG_DOT and "knn_filter_dot" set, d % 8 == 0,
// 8 <= d <= 1024, k <= 512 (heaps), n > 4 k.  Byte rows, pools (k > 512) and d > 1024 keep the paths they have; binary16 rows have
// knn_half_dot.hip's filter under a knob of their own, which shares this file's norm bounds, thresholds and rescore.
//
// The distance is Dist = -q.x, so there is no norm to fold in and no |q|^2 + |x|^2 to scale an error with: the error of q.x on the matrix
// cores (v_mfma_f32_32x32x16_bf16 over knn_pack_kernel's hi / lo images, three products per K step: xh.qh + xl.qh + xh.ql) scales with
// P = |q||x|, whatever the distance.  A row is kept when
//     fma(cq, ux, acc) >= thr        acc = q.x on the matrix cores, accumulators from zero
//                                    ux  = an upper bound of |x|   (knn_dot_bounds_kernel: sqrt of the packed norm, scaled up)
//                                    cq  = c * (an upper bound of |q|), c = kKnnWideSlack = 2^-10 -- the product by a power of two is exact
//                                    thr = -T_q, T_q the query's current exact k-th distance -- exact --, -inf while the heap is not full
// one fma and one compare per pair.  Kept rows get Angular::Dist in the scan's operations and order (knn_dot_rescore_kernel) and are
// offered to the scan's heaps.
//
// Division of work: knn_wide.hip's.  A workgroup of 4 wavefronts owns a tile of 128 queries x 128 rows, wavefront (wq, wr) a 64 x 64
// sub-tile as four 32 x 32 accumulators; blockIdx.x picks the queries, blockIdx.y a slab of the chunk's blocks of 128 rows; the K loop runs
// over dp = round_up(d, 16) in stages of KS K steps (down to one stage of one live K step at d = 8 .. 16), both operands global memory ->
// registers -> LDS through two buffers by hand-issued loads, one barrier per stage, LDS pitch 64 KS + 16 bytes.  The staging code is a COPY
// of knn_wide_filter_kernel's, not a shared header: there it is a set of lambdas over the kernel's locals, and a shared form would have to
// become a struct of references or a functor-taking template whose register allocation the measured L2 kernel would then depend on.
// The epilogue is this file's.  C layout: register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h, column r -- a lane's 16 values of a
// tile belong to ONE query, so cq and thr are per lane and ux varies with v: fetched, with the tag words, in aligned groups of four at the
// head of the row block.  A group that starts behind the chunk is not read and gets ux = -inf: fma(cq, -inf, acc) = -inf fails every
// threshold but -inf, and a -inf threshold's rows are refused by j < rows; (+inf, the L2 kernel's choice for its norms, would here pass
// every threshold and send every partial block down the hit path).  cq = 0 -- a query beyond the batch -- gives NaN, which compares false.
// knn_dot_bounds_kernel writes -inf behind the set's last row too.  Then knn_sweep.h's hit path: max over the 16 values, one compare,
// ballot; a returning atomicAdd per lane with hits, ids stored while pos < cap, the overflow flag otherwise; tags tested where hits are
// counted.
//
// Error bound for dp <= 1024 on the scale P = |q||x| (|acc - Dist_ref| <= b P must hold with b < c; sum |q_k x_k| <= P):
//   dropped       x = xh + xl + r, |xl| <= 2^-8 |x|, |r| <= 2^-16 |x| (two round-to-nearest bf16 steps); the three products kept are exact in
//                 f32, the dropped ones (xl.ql, r.q, x.r) sum to <= 3 * 2^-16 |q_k x_k| per dimension: 3 * 2^-16 P = 4.58e-5 P.
//   accumulation  3 dp / 16 matrix instructions of 16 products each, taken as one add per product that may truncate (2^-23) against a
//                 partial sum <= sum |q_k x_k|: 3 dp 2^-23 P = 3.66e-4 P at dp = 1024.
//   reference     Angular::Dist rounds each product once and adds it to one of eight running sums (d / 8 adds), then three levels of
//                 pairwise adds: <= (d / 8 + 3) roundings a path, taken at 2^-23 each: (d / 8 + 3) 2^-23 P = 1.56e-5 P.  The negation is exact.
//   the fma       one rounding of acc + cq ux, a value of at most (1 + b + c) P: taken as 2^-23 P = 1.2e-7 P.
//   norm bounds   nothing on this side: ux >= |x| and cq >= c |q| by construction (below), so cq ux >= c P; what they cost is kept rows --
//                 the slack actually applied is up to (1 + 2^-12)^2 c.
// Sum at d = dp = 1024: 4.28e-4 P.  c = 2^-10 = 9.77e-4 leaves a factor 2.2; the static_assert pins the sum at kKnnWideMaxDim with 1.5.
//
// The bounds ux, uq: the packed norm n2 is d products and d adds in float32, all terms >= 0: n2 >= |x|^2 (1 - d 2^-24) to first order, so
// |x| <= sqrt(n2) (1 + d 2^-25) = sqrt(n2) (1 + 2^-15) at d = 1024; the correctly rounded sqrt and the product by the factor round once
// each (2^-24).  Factor kDotNormUp = 1 + 2^-12: more than four times the sum of the three.
// Range: all terms are relative and assume normal float32 arithmetic.  A call is covered when every n2 (rows and queries) lies in
// [2^-96, 2^96]: products q_k x_k are then below 2^96, and a product or a square lost to underflow is below 2^-126 against P >= 2^-96
// (3 dp of them: 2^-114 against c P >= 2^-106) or n2 >= 2^-96.  A zero, non-finite, tiny or huge norm sets the flag
// knn_dot_bounds_kernel returns, and the call is served by the exact scan: for every finite input the answer is the scan's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "knn_select.h"     // the distance keys, the heap
#include "knn_scan_dist.h"  // f32x2
#include "knn_scan_kernels.h"  // knn_rows, knn_widen, knn_row_step: the rescore's binary16 instance

namespace gbnns {

namespace {

constexpr float kKnnDotBound = 3.0f * kKnnWideMaxDim / 8388608.0f       // accumulation
                               + (kKnnWideMaxDim / 8 + 3) / 8388608.0f  // the reference dot
                               + 3.0f / 65536.0f                        // the dropped products
                               + 1.0f / 8388608.0f;                     // the fma
static_assert(kKnnWideSlack >= 1.5f * kKnnDotBound, "kKnnWideSlack no longer covers the dot filter's error bound at its longest row with a factor 1.5");
constexpr float kDotNormUp = 1.0f + 1.0f / 4096.0f;
static_assert(kDotNormUp - 1.0f >= 4.0f * (kKnnWideMaxDim / 33554432.0f + 2.0f / 16777216.0f), "kDotNormUp no longer covers the norm's summation and the sqrt");
// (knn_half_dot.hip's norms are knn_half_norm_kernel's and knn_half_qsplit_kernel's sums, not knn_pack_kernel's: serial too, at most d products
// and d adds that round, the product's rounding counted as a term of its own -- (d + 1) 2^-25 on the norm; the derivation is written out there)
static_assert(kDotNormUp - 1.0f >= 4.0f * ((kKnnWideMaxDim + 1) / 33554432.0f + 2.0f / 16777216.0f), "kDotNormUp no longer covers the half-row calls' norm sums and the sqrt");
constexpr float kDotNormLo = 0x1p-96f, kDotNormHi = 0x1p96f;  // the squared norms the bound's terms hold for

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kDotTile = 128;  // queries, and rows, of a workgroup's tile

template <int KS>
constexpr uint32_t kDotPitch = 64u * KS + 16u;  // bytes of one packed row's stage in LDS
template <int KS>
constexpr uint32_t kDotLds = 4u * kDotTile * kDotPitch<KS>;  // two buffers of two operands

// In place: squared norms -> upper bounds of the norms, times `scale` (rows: 1; queries: c); entries i >= live (the padding behind the
// set) -> -inf.  *uncovered is set where a live norm lies outside the range of the bound.
__global__ __launch_bounds__(256) void knn_dot_bounds_kernel(float* norms, uint64_t live, uint64_t count, float scale, uint32_t* uncovered) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    if (i >= live) {
        norms[i] = -__builtin_inff();
        return;
    }
    const float n2 = norms[i];
    if (!(n2 >= kDotNormLo && n2 <= kDotNormHi)) *uncovered = 1u;  // (NaN included)
    norms[i] = scale * (__builtin_sqrtf(n2) * kDotNormUp);
}

// KS = K steps of 16 dims per stage
template <int KS, bool TAG>
__global__ __launch_bounds__(256) void knn_dot_filter_kernel(KnnFilterParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dot_smem[];
    constexpr uint32_t PITCH = kDotPitch<KS>, OPER = kDotTile * PITCH;  // a buffer: the rows' stage, then the queries'
    constexpr int LD = 2 * KS;            // 16-byte requests per thread, operand and stage: 128 rows x 4 KS / 256 threads
    constexpr uint32_t UNITS = 4u * KS;   // 16-byte units of a row's stage
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint32_t wq = wave & 1u, wr = wave >> 1;
    const uint32_t q0 = blockIdx.x * kDotTile;
    const uint32_t ksteps = p.dp >> 4, stages = (ksteps + KS - 1) / KS;
    const size_t row_bytes = (size_t)p.dp * 4;  // 2 dp 16-bit parts
    const uint32_t blocks = (p.rows + kDotTile - 1) / kDotTile;
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
    // the thresholds -T, slack factors c |q| and tag words of the lane's queries: one per 32 x 32 tile column block
    float thr[2], cq[2];
    uint32_t qtag[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const uint32_t qv = q0 + 64u * wq + 32u * qt + r;
        thr[qt] = qv < p.nq ? p.rhs[qv] : __builtin_inff();
        cq[qt] = qv < p.nq ? p.cq[qv] : 0.f;
        qtag[qt] = 0u;
        if constexpr (TAG) qtag[qt] = qv < p.nq ? p.qtag[qv] : 0u;
    }

    // a stage's units on their way: rows' then queries'.  A unit of a K step beyond dp (the last stage) is requested at the row's first
    // 16 bytes instead -- readable -- and written as zeros.
    u32x4 stg[2 * LD];
    auto request = [&](uint32_t rb, uint32_t st) {
#pragma unroll
        for (int i = 0; i < LD; ++i) {
            const uint32_t j = rb * kDotTile + lrow[i];
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
        unsigned char* xb = dot_smem + buf * 2u * OPER;
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
        const unsigned char* xb = dot_smem + buf * 2u * OPER + (64u * wr + r) * PITCH + 32u * h;
        const unsigned char* qb = dot_smem + buf * 2u * OPER + OPER + (64u * wq + r) * PITCH + 32u * h;
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
        // Norm bounds (and tag words) of the lane's rows, register group g of row block rt = rows 8 g + 4 h + 0 .. 3: aligned groups of
        // four, asked for here so that they have landed behind the K loop.  A group that starts beyond the chunk is not read: -inf.
        u32x4 ux[2][4], tg[2][4];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t jg = rb * kDotTile + 64u * wr + 32u * rt + 8u * g + 4u * h;
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
                f32x16 t;  // q.x + c |q||x|: the slack in the fma's one rounding
#pragma unroll
                for (int v = 0; v < 16; ++v) t[v] = __builtin_fmaf(cq[qt], __uint_as_float(ux[rt][v >> 2][v & 3]), acc[qt][rt][v]);
                float m = fmaxf(fmaxf(t[0], t[1]), t[2]);  // (fmaxf drops a NaN: cq = 0 against -inf)
#pragma unroll
                for (int v = 3; v < 15; v += 2) m = fmaxf(fmaxf(m, t[v]), t[v + 1]);
                m = fmaxf(m, t[15]);
                if (__builtin_expect(__ballot(m >= thr[qt]) != 0ull, 0)) {
                    const uint32_t qv = q0 + 64u * wq + 32u * qt + r;
                    const uint32_t j0 = rb * kDotTile + 64u * wr + 32u * rt + 4u * h;
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

// The exact distances of the rows the dot filter kept: one wavefront per query.  The query is staged once in LDS and read by broadcast;
// every lane takes one candidate row straight from global memory and runs Angular::Dist (support_func.h:130-163) in the scan kernels'
// operations and order (knn_scan_row.inc's dot branch, which knn_scan_wide_kernel's repeats for d > 128): eight running sums by k mod 8 as
// four pairs -- an even 16-byte step adds to sums 0 .. 3, an odd one to 4 .. 7; d % 8 == 0: whole pairs of steps --, the high half added
// onto the low half, the pairwise adds, the negation.  The keys below the heap's root are offered in list order by lane 0; then the
// query's new threshold -T.
// B = uint16_t: binary16 rows (p.k.base_h, bstride in halves), widened as they are loaded -- exact --, then the same sums in the same order;
// VEC there: a table of whole 16-byte chunks, one load of eight halves for a pair of steps.
template <class B, bool VEC>  // rows and queries 16-byte aligned at strides of whole float4 steps: one load a step
__global__ __launch_bounds__(64) void knn_dot_rescore_kernel(KnnRescoreParams p) {
    __shared__ float4 qs[kKnnWideMaxDim / 4];
    __shared__ uint64_t keys[64];
    __shared__ uint64_t new_root;
    const KnnParams& kp = p.k;
    const uint32_t qi = blockIdx.x, lane = threadIdx.x;
    const uint32_t cnt = min(p.count[qi], p.cap);
    if (cnt == 0) return;  // (threshold unchanged)
    const uint32_t steps = kp.dim >> 2;  // even
    const float* qp = kp.q + (size_t)qi * kp.qstride;
    for (uint32_t c = lane; c < steps; c += 64u)
        qs[c] = VEC ? reinterpret_cast<const float4*>(qp)[c] : make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]);
    uint64_t root = kp.heap[qi];
    __syncthreads();
    for (uint32_t e0 = 0; e0 < cnt; e0 += 64u) {
        const uint32_t e = e0 + lane;
        const bool valid = e < cnt;
        const uint32_t row = valid ? p.cand[(size_t)qi * p.cap + e] : p.cand[(size_t)qi * p.cap];  // (an idle lane: the list's first row again)
        const B* bp = knn_rows<B>(kp) + (size_t)row * kp.bstride;
        f32x2 cs[4];  // {0,1} {2,3} {4,5} {6,7}
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] = f32x2{0.f, 0.f};
        // steps c and c + 1 of the row
        auto pair = [&](uint32_t c, float4& b0, float4& b1) {
            if constexpr (!kKnnHalfRows<B>) {
                b0 = VEC ? reinterpret_cast<const float4*>(bp)[c] : make_float4(bp[4 * c], bp[4 * c + 1], bp[4 * c + 2], bp[4 * c + 3]);
                b1 = VEC ? reinterpret_cast<const float4*>(bp)[c + 1u] : make_float4(bp[4 * c + 4], bp[4 * c + 5], bp[4 * c + 6], bp[4 * c + 7]);
            } else if constexpr (VEC) {
                const uint4 w = reinterpret_cast<const uint4*>(bp)[c >> 1];
                b0 = make_float4(knn_widen((uint16_t)w.x), knn_widen((uint16_t)(w.x >> 16)), knn_widen((uint16_t)w.y), knn_widen((uint16_t)(w.y >> 16)));
                b1 = make_float4(knn_widen((uint16_t)w.z), knn_widen((uint16_t)(w.z >> 16)), knn_widen((uint16_t)w.w), knn_widen((uint16_t)(w.w >> 16)));
            } else {
                b0 = knn_row_step(bp, c, false);
                b1 = knn_row_step(bp, c + 1u, false);
            }
        };
#pragma unroll 4
        for (uint32_t c = 0; c < steps; c += 2u) {
            float4 b0, b1;
            pair(c, b0, b1);
            const float4 q0 = qs[c], q1 = qs[c + 1u];
            cs[0] = cs[0] + f32x2{b0.x, b0.y} * f32x2{q0.x, q0.y};
            cs[1] = cs[1] + f32x2{b0.z, b0.w} * f32x2{q0.z, q0.w};
            cs[2] = cs[2] + f32x2{b1.x, b1.y} * f32x2{q1.x, q1.y};
            cs[3] = cs[3] + f32x2{b1.z, b1.w} * f32x2{q1.z, q1.w};
        }
        const f32x2 m01 = cs[2] + cs[0], m23 = cs[3] + cs[1];
        const float dist = -((m01.x + m01.y) + (m23.x + m23.y));
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
    if (lane == 0) p.rhs[qi] = root == ~0ull ? -__builtin_inff() : -knn_fkey_inv((uint32_t)(root >> 32));
}

// thresholds from the heaps: thr[q] = -d_k(q), -inf while the heap is not full (an all-ones key at the root)
__global__ __launch_bounds__(256) void knn_dot_thresholds_kernel(const uint64_t* heap, uint32_t nq, float* thr) {
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    if (qi >= nq) return;
    const uint64_t root = heap[qi];
    thr[qi] = root == ~0ull ? -__builtin_inff() : -knn_fkey_inv((uint32_t)(root >> 32));
}

constexpr int kDotStage = 2;  // K steps per stage: 72 KB of LDS, two workgroups a CU
static_assert(kDotStage == 2, "knn_dot_filter_kernel_name spells the stage out");

template <bool TAG>
hipError_t knn_dot_filter_launch(const KnnFilterParams& p, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_dot_filter_kernel<kDotStage, TAG>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kDotLds<kDotStage>);  // (more than the 64 KB a launch may ask for unannounced)
    if (e != hipSuccess) return e;
    // grid: x = blocks of 128 queries, y = slabs of the chunk's blocks of 128 rows -- two workgroups of 4 wavefronts for every CU
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const unsigned gx = (p.nq + kDotTile - 1) / kDotTile, blocks = (p.rows + kDotTile - 1) / kDotTile;
    const unsigned want = 2u * (unsigned)cus;
    unsigned gy = gx >= want ? 1u : (want + gx - 1) / gx;
    if (gy > blocks) gy = blocks;
    hipLaunchKernelGGL((knn_dot_filter_kernel<kDotStage, TAG>), dim3(gx, gy), dim3(256), kDotLds<kDotStage>, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_knn_dot_bounds(float* norms, uint64_t live, uint64_t count, float scale, uint32_t* uncovered, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (live > count || !uncovered) return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_dot_bounds_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, norms, live, count, scale, uncovered);
    return hipGetLastError();
}

hipError_t launch_knn_dot_filter(const KnnFilterParams& p, hipStream_t s) {
    if (p.nq == 0 || p.rows == 0) return hipSuccess;
    if (p.dp == 0 || (p.dp & 15u) || p.dp > kKnnWideMaxDim || !p.cq || (p.btag && !p.qtag)) return hipErrorInvalidValue;
    // the norm bounds and tag words are read in aligned groups of four
    if ((reinterpret_cast<uintptr_t>(p.bnorm) & 15u) || (reinterpret_cast<uintptr_t>(p.btag) & 15u)) return hipErrorInvalidValue;
    return p.btag ? knn_dot_filter_launch<true>(p, s) : knn_dot_filter_launch<false>(p, s);
}
const char* knn_dot_filter_kernel_name(uint32_t dp, bool tagged) {
    if (dp == 0 || (dp & 15u) || dp > kKnnWideMaxDim) return nullptr;
    return tagged ? "knn_dot_filter_kernel<2, true>" : "knn_dot_filter_kernel<2, false>";
}

hipError_t launch_knn_dot_rescore(const KnnRescoreParams& p, hipStream_t s) {
    if (p.k.nq == 0) return hipSuccess;
    if (!p.k.base || p.k.dim == 0 || p.k.dim > kKnnWideMaxDim || (p.k.dim & 7u)) return hipErrorInvalidValue;
    const bool vec = !(p.k.bstride & 3u) && !(p.k.qstride & 3u) && !(reinterpret_cast<uintptr_t>(p.k.base) & 15u) && !(reinterpret_cast<uintptr_t>(p.k.q) & 15u);
    if (vec) hipLaunchKernelGGL((knn_dot_rescore_kernel<float, true>), dim3(p.k.nq), dim3(64), 0, s, p);
    else hipLaunchKernelGGL((knn_dot_rescore_kernel<float, false>), dim3(p.k.nq), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_knn_half_dot_rescore(const KnnRescoreParams& p, hipStream_t s) {
    if (p.k.nq == 0) return hipSuccess;
    if (!p.k.base_h || p.k.dim == 0 || p.k.dim > kKnnWideMaxDim || (p.k.dim & 7u)) return hipErrorInvalidValue;
    // (16-byte chunks of eight halves: a table at a stride of whole chunks; the query's float4 steps as above)
    const bool vec = !(p.k.bstride & 7u) && !(p.k.qstride & 3u) && !(reinterpret_cast<uintptr_t>(p.k.base_h) & 15u) && !(reinterpret_cast<uintptr_t>(p.k.q) & 15u);
    if (vec) hipLaunchKernelGGL((knn_dot_rescore_kernel<uint16_t, true>), dim3(p.k.nq), dim3(64), 0, s, p);
    else hipLaunchKernelGGL((knn_dot_rescore_kernel<uint16_t, false>), dim3(p.k.nq), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_knn_dot_thresholds(const uint64_t* heap, uint32_t nq, float* thr, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(knn_dot_thresholds_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, s, heap, nq, thr);
    return hipGetLastError();
}

}  // namespace gbnns
