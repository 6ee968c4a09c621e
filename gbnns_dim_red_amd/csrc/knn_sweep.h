// knn_sweep.h -- the matrix-core sweep of the exact kNN, once: knn_filter_kernel (knn.hip: float rows as bf16 hi + lo), knn_bytes_sweep_kernel
// (knn_bytes.hip: int8 operands, the product is the distance) and knn_half_sweep_kernel (knn_half.hip: binary16 rows in place) are this body
// with an `Ops` each that states the sweep's arithmetic; their error bounds stay in their units.
//
// Division of work.  A workgroup = 4 wavefronts x QB blocks of 32 queries (operand B of the product, in registers for the whole launch: the
// lane's column of every 32 x 32 tile is ITS query, so one threshold per lane and block); blockIdx.y picks a slab of the chunk's rows, walked
// in blocks of 32 (operand A straight from global memory, the next block's fragments requested before the current block's products: a chunk
// is L2 / Infinity-Cache resident while every workgroup sweeps it).  Lane (r, h) holds row / query r and the h-th half of every K step of
// both operands.  C/D: register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h of the block, column r -- so a lane's 16 values of a tile
// belong to 16 rows and ONE query, their per-row side words (norms or terms) are four 16-byte loads, and a kept pair is
// max over the lane's 16 values >= threshold[query]: eight v_max3 and one compare per tile beside its matrix instructions.
// TAG (the tagged entry points): a pair whose row is not allowed for its query -- (btag[row] & qtag[query]) == 0 -- is not a hit, neither
// counted nor stored.  The tag words of a lane's 16 rows travel with the block's side words (four more 16-byte requests, the same address
// pattern; the array is padded like them) and are looked at where hits are counted: under a selective filter a query's threshold is its
// k-th ALLOWED distance, rows of every tile pass it, and a fetch in the hit path was a dependent load in most tiles (DESIGN.md 5.1 has both
// measurements).
//
// What an Ops states (knn.hip's KnnFilterOps is the one to read first):
//   Params                     the kernel's parameter struct; the body itself reads nq, rows, row0, cap, cand, count, overflow, btag, qtag
//   Val, Vals                  a comparable value (float / int32_t: LARGER = nearer) and a lane's 16 of them (ext vector)
//   Q, load_q, use_q           a query's threshold `thr` and its companions; the out-of-batch values (thr: nothing passes); an empty asm use
//   kQFrags, q_ptr             16-byte operand fragments per K step and lane, and the query's packed row: fragment f of lane half h at K step s
//                              is its 16-byte word kQFrags (2 s + h) + f
//   kRowFrags, row_ptr,        16-byte requests per K step and row (2: the second one at offset:16), the lane's first one of row j, and the
//   row_off                    byte offset of step s from it
//   side                       the per-row side words' array (32-bit words; readable 64 entries beyond the set)
//   rows_init, tile            a block's side words as the products want them; one tile's 16 values from the fragments
//   kKeepsValue, kept          what a kept pair stores: the id alone, or a key made from the value
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gbnns {

typedef uint32_t knn_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float knn_sweep_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int32_t knn_sweep_max(int32_t a, int32_t b) { return max(a, b); }

template <class Ops, int KSTEPS, int QB, bool TAG>
__device__ __forceinline__ void knn_sweep_body(const typename Ops::Params& p) {
    typedef knn_u32x4 u32x4;
    typedef typename Ops::Q Q;
    typedef typename Ops::Vals Vals;
    constexpr int QF = Ops::kQFrags * KSTEPS, RF = Ops::kRowFrags * KSTEPS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint32_t q0 = (blockIdx.x * 4u + wave) * (QB * 32u);
    if (q0 >= p.nq) return;
    u32x4 qf[QB][QF];
    Q q[QB];
    uint32_t qtag[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        const uint32_t qi = q0 + 32u * b + r;
        const bool ok = qi < p.nq;
        if constexpr (TAG) qtag[b] = ok ? p.qtag[qi] : 0u;
        const uint4* src = Ops::q_ptr(p, ok ? qi : 0u);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
            for (int f = 0; f < Ops::kQFrags; ++f) qf[b][Ops::kQFrags * s + f] = __builtin_bit_cast(u32x4, src[Ops::kQFrags * (2 * s + h) + f]);
        q[b] = Ops::load_q(p, qi, ok);  // (a query beyond the batch keeps nothing)
    }
    // (every compiler-issued load is used here, once: its waits then sit in this prologue and not inside the sweep)
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        Ops::use_q(q[b]);
        if constexpr (TAG) asm volatile("" ::"v"(qtag[b]));
#pragma unroll
        for (int s = 0; s < QF; ++s) asm volatile("" ::"v"(qf[b][s]));
    }
    const uint32_t blocks = (p.rows + 31u) >> 5;
    const uint32_t per = (blocks + gridDim.y - 1) / gridDim.y;
    const uint32_t b_lo = blockIdx.y * per, b_hi = min(blocks, b_lo + per);
    if (b_lo >= b_hi) return;
    uint32_t xoff[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) xoff[s] = Ops::row_off(p, s, h);
    // Fragments and side words of one block of 32 rows (rows beyond the chunk read row 0), requested by hand-written loads: the
    // compiler's own bookkeeping put a full wait (vmcnt(0)) BEHIND the next block's requests -- no overlap at all -- whatever the
    // order in the source; these requests are invisible to it, and `landed` below is the one wait, placed in front of the next
    // requests.  (No branch here: the side words' array is readable 64 entries beyond the set, and the chunk starts on a multiple
    // of 64 rows.  What lies there need not keep a row out: the norms' padding is +inf, the byte terms' and the tag words' is any
    // value, and a row beyond the chunk -- padding, or a row of the NEXT chunk -- is refused by `j < p.rows` where the hits are
    // counted.)
    auto request_block = [&](uint32_t rb, u32x4 (&x)[RF], u32x4 (&sd)[4], u32x4 (&tg)[4]) {
        const uint32_t j = rb * 32u + r;
        const char* bp = Ops::row_ptr(p, j < p.rows ? j : 0u, h);
        const uint32_t* np = Ops::side(p) + rb * 32u + 4u * h;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(x[Ops::kRowFrags * s]) : "v"(bp + xoff[s]));
            if constexpr (Ops::kRowFrags == 2) asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(x[2 * s + 1]) : "v"(bp + xoff[s]));
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)  // accumulator registers 4 g .. 4 g + 3 = rows 8 g + 4 h + 0 .. 3 of the block
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(sd[g]) : "v"(np + 8 * g));
        if constexpr (TAG) {
            const uint32_t* tp = p.btag + rb * 32u + 4u * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(tg[g]) : "v"(tp + 8 * g));
        }
    };
    auto landed = [&](u32x4 (&x)[RF], u32x4 (&sd)[4], u32x4 (&tg)[4]) {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(sd[0]));
#pragma unroll
        for (int g = 1; g < 4; ++g) asm volatile("" : "+v"(sd[g]));
#pragma unroll
        for (int s = 0; s < RF; ++s) asm volatile("" : "+v"(x[s]));
        if constexpr (TAG) {
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(tg[g]));
        }
    };
    // the products and the test of one block of rows against the QB query blocks
    auto sweep_block = [&](uint32_t rb, const u32x4 (&x)[RF], const u32x4 (&sd)[4], const u32x4 (&tg)[4]) {
        const Vals init = Ops::rows_init(sd);
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            const Vals t = Ops::template tile<KSTEPS>(p, x, init, qf[b], q[b]);
            typename Ops::Val m = knn_sweep_max(knn_sweep_max(t[0], t[1]), t[2]);
#pragma unroll
            for (int v = 3; v < 15; v += 2) m = knn_sweep_max(knn_sweep_max(m, t[v]), t[v + 1]);
            m = knn_sweep_max(m, t[15]);
            if (__builtin_expect(__ballot(m >= q[b].thr) != 0ull, 0)) {
                // one returning atomic per lane with hits (its 16 rows of the tile): the places of all of them at once -- a
                // returning atomic per hit serialised up to sixteen memory round trips in every tile that had any, and in
                // the early chunks (thresholds still loose) that is most tiles
                const uint32_t qv = q0 + 32u * b + r;  // (nothing passes beyond the batch: never here with qv >= nq)
                uint32_t hits = 0;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const uint32_t j = rb * 32u + (uint32_t)((v & 3) + 8 * (v >> 2)) + 4u * h;
                    hits |= (t[v] >= q[b].thr && j < p.rows) ? 1u << v : 0u;  // (a pass-all threshold -- list not full yet -- lets -inf through too)
                }
                if constexpr (TAG) {
                    uint32_t tm = 0;
#pragma unroll
                    for (int v = 0; v < 16; ++v) tm |= ((tg[v >> 2][v & 3] & qtag[b]) ? 1u : 0u) << v;
                    hits &= tm;
                }
                if (hits) {
                    uint32_t pos = atomicAdd(&p.count[qv], (uint32_t)__popc(hits));
                    auto store = [&](uint32_t v, typename Ops::Val tv) {
                        if (pos < p.cap) p.cand[(size_t)qv * p.cap + pos] = Ops::kept(q[b], p.row0 + rb * 32u + ((v & 3u) + 8u * (v >> 2)) + 4u * h, tv);
                        else *p.overflow = 1u;
                        pos += 1u;
                    };
                    // Two forms of the store loop.  A sweep that stores the value walks the registers: a register cannot be picked by a
                    // run-time v.  One that stores ids alone walks the set bits.  (The two were never measured against each other for
                    // the id-only kernels: each kernel keeps the form it had.)
                    if constexpr (Ops::kKeepsValue) {
#pragma unroll
                        for (int v = 0; v < 16; ++v)
                            if (hits & (1u << v)) store((uint32_t)v, t[v]);
                    } else {
                        do {
                            const uint32_t v = (uint32_t)__ffs((int)hits) - 1u;
                            hits &= hits - 1u;
                            store(v, typename Ops::Val());
                        } while (hits);
                    }
                }
            }
        }
    };
    // two register sets in turn: wait for the set at hand, request the next block into the other one, sweep
    u32x4 x0[RF], x1[RF], sd0[4], sd1[4], tg0[4], tg1[4];
    request_block(b_lo, x0, sd0, tg0);
    for (uint32_t rb = b_lo;;) {
        landed(x0, sd0, tg0);
        if (rb + 1u < b_hi) request_block(rb + 1u, x1, sd1, tg1);
        sweep_block(rb, x0, sd0, tg0);
        if (++rb >= b_hi) break;
        landed(x1, sd1, tg1);
        if (rb + 1u < b_hi) request_block(rb + 1u, x0, sd0, tg0);
        sweep_block(rb, x1, sd1, tg1);
        if (++rb >= b_hi) break;
    }
}

// 4 SIMDs per CU of the current device (the MI355X: 1 024)
inline unsigned knn_sweep_simds() {
    static const unsigned simds = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return 4u * (unsigned)cus;
    }();
    return simds;
}

// grid: x = the query blocks of 4 wavefronts, y = slabs of the chunk's row blocks -- enough workgroups for every SIMD
template <int QB, class Params>
hipError_t knn_sweep_launch(void (*kernel)(Params), const Params& p, hipStream_t s) {
    const unsigned gx = (p.nq + QB * 128u - 1) / (QB * 128u);
    const unsigned blocks = (p.rows + 31u) >> 5;
    const unsigned simds = knn_sweep_simds();
    unsigned gy = gx >= simds ? 1u : (simds + gx - 1) / gx;
    if (gy > blocks) gy = blocks;
    if (gy < 1u) gy = 1u;
    hipLaunchKernelGGL(kernel, dim3(gx, gy), dim3(256), 0, s, p);
    return hipGetLastError();
}

// The sweep instance of a packed row length, launch and name from one place.  KNN_SWEEP_PICK_FN(fn, kernel, Params, K step, <QB of 1 .. 8 K steps>)
// defines  KnnSweepPick<Params> fn(uint32_t dp, bool tagged)  -- no instance for a dp that is no multiple of the K step or longer than 8 of
// them; query blocks per wavefront by what the operands leave of the register file.  A unit #undef's the macros below behind
// its table, as it did its own.
template <class Params>
struct KnnSweepPick {
    hipError_t (*launch)(const Params&, hipStream_t);
    const char* name;
};
#define KNN_SWEEP_QB_TWO_PART 4, 4, 2, 2, 1, 1, 1, 1  // two 16-byte B fragments per K step of 16 (knn.hip, knn_half.hip)
#define KNN_SWEEP_PICK_FN(FN, KERNEL, PARAMS, STEP, ...) KNN_SWEEP_PICK_FN_(FN, KERNEL, PARAMS, STEP, __VA_ARGS__)
#define KNN_SWEEP_PICK_FN_(FN, KERNEL, PARAMS, STEP, Q1, Q2, Q3, Q4, Q5, Q6, Q7, Q8)                                                \
    KnnSweepPick<PARAMS> FN(uint32_t dp, bool tagged) {                                                                           \
        switch (dp % (STEP) ? 0u : dp / (STEP)) {                                                                                 \
            KNN_SWEEP_CASE_(KERNEL, PARAMS, 1, Q1) KNN_SWEEP_CASE_(KERNEL, PARAMS, 2, Q2) KNN_SWEEP_CASE_(KERNEL, PARAMS, 3, Q3)  \
            KNN_SWEEP_CASE_(KERNEL, PARAMS, 4, Q4) KNN_SWEEP_CASE_(KERNEL, PARAMS, 5, Q5) KNN_SWEEP_CASE_(KERNEL, PARAMS, 6, Q6)  \
            KNN_SWEEP_CASE_(KERNEL, PARAMS, 7, Q7) KNN_SWEEP_CASE_(KERNEL, PARAMS, 8, Q8)                                         \
            default: return KnnSweepPick<PARAMS>{nullptr, nullptr};                                                               \
        }                                                                                                                         \
    }
#define KNN_SWEEP_CASE_(KERNEL, PARAMS, K, QB) \
    case K: return tagged ? KNN_SWEEP_INSTANCE_(KERNEL, PARAMS, K, QB, true) : KNN_SWEEP_INSTANCE_(KERNEL, PARAMS, K, QB, false);
#define KNN_SWEEP_INSTANCE_(KERNEL, PARAMS, K, QB, TAG)                                                                           \
    KnnSweepPick<PARAMS> {                                                                                                        \
        [](const PARAMS& p, hipStream_t s) { return knn_sweep_launch<QB>(&KERNEL<K, QB, TAG>, p, s); }, #KERNEL "<" #K ", " #QB ", " #TAG ">" \
    }

}  // namespace gbnns
