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
#include "knn_scan_kernels.h"  // the scan, rescore and pool kernels: the binary16 instances

namespace gbnns {

namespace {

constexpr uint32_t kKnnHalfMaxDim = 128;  // (the bound would allow 256; the rescore kernel holds the query in registers: d <= 128)
static_assert(kKnnFilterSlack >= 4.0f * kKnnHalfMaxDim / 8388608.0f + 1.0f / 32768.0f, "kKnnFilterSlack no longer covers the half-row sweep's error bound at its longest row");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

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

// knn_filter_kernel's division of work (knn.hip): a workgroup = 4 wavefronts x QB blocks of 32 queries, operand B (hi and lo of the scaled
// query) in registers for the whole launch; blockIdx.y picks a slab of the chunk's rows, walked in blocks of 32 with two register sets in
// turn -- the next block's fragments requested before the current block's products; one returning atomic per lane with hits; ids to the
// per-query lists.  Operand A: KSTEPS 16-byte loads per lane straight from the table (half the float filter's requests, a quarter of its
// bytes per row).  C/D: register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h of the block, column r.
// TAG: as in knn_filter_kernel -- the tag words of a lane's 16 rows travel with the block's norms and are looked at where hits are counted.
template <int KSTEPS, int QB, bool TAG>
__global__ __launch_bounds__(256) void knn_half_sweep_kernel(KnnHalfSweepParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint32_t q0 = (blockIdx.x * 4u + wave) * (QB * 32u);
    if (q0 >= p.nq) return;
    const uint32_t groups = p.dp >> 3;  // 8-dim groups per query = 2 KSTEPS
    f16x8 qh[QB][KSTEPS], ql[QB][KSTEPS];
    float rhs[QB], qinv[QB];
    uint32_t qtag[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        const uint32_t qi = q0 + 32u * b + r;
        const bool ok = qi < p.nq;
        if constexpr (TAG) qtag[b] = ok ? p.qtag[qi] : 0u;
        const uint16_t* qp = p.qsplit + (size_t)(ok ? qi : 0u) * groups * 16;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const uint4* src = reinterpret_cast<const uint4*>(qp + (size_t)(2 * s + h) * 16);
            qh[b][s] = __builtin_bit_cast(f16x8, src[0]);
            ql[b][s] = __builtin_bit_cast(f16x8, src[1]);
        }
        rhs[b] = ok ? p.rhs[qi] : __builtin_inff();  // (a query beyond the batch keeps nothing)
        qinv[b] = ok ? p.qinv[qi] : 0.f;
    }
    // (every compiler-issued load is used here, once: its waits then sit in this prologue and not inside the sweep)
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        asm volatile("" ::"v"(rhs[b]), "v"(qinv[b]));
        if constexpr (TAG) asm volatile("" ::"v"(qtag[b]));
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) asm volatile("" ::"v"(qh[b][s]), "v"(ql[b][s]));
    }
    const uint32_t blocks = (p.rows + 31u) >> 5;
    const uint32_t per = (blocks + gridDim.y - 1) / gridDim.y;
    const uint32_t b_lo = blockIdx.y * per, b_hi = min(blocks, b_lo + per);
    if (b_lo >= b_hi) return;
    const float scale = -0.5f * (1.0f - kKnnFilterSlack);
    // the lane's chunk of every K step, in halves from the row's start: 2 s + h, or the row's last chunk where that lies beyond it
    uint32_t coff[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) coff[s] = 8u * min(2u * (uint32_t)s + h, p.last_chunk);
    // Fragments and norms of one block of 32 rows (rows beyond the chunk read row 0; the norms' array is readable 64 entries beyond the set
    // and +inf there; the chunk starts on a multiple of 64 rows), requested by hand-written loads as in knn_filter_kernel: `landed` is the
    // one wait, placed in front of the next requests.
    auto request_block = [&](uint32_t rb, u32x4 (&xa)[KSTEPS], f32x4v (&nx)[4], u32x4 (&tg)[4]) {
        const uint32_t j = rb * 32u + r;
        const uint16_t* bp = p.base + (size_t)(j < p.rows ? j : 0u) * p.stride;
        const float* np = p.bnorm + rb * 32u + 4u * h;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xa[s]) : "v"(bp + coff[s]));
#pragma unroll
        for (int g = 0; g < 4; ++g)  // accumulator registers 4 g .. 4 g + 3 = rows 8 g + 4 h + 0 .. 3 of the block
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(nx[g]) : "v"(np + 8 * g));
        if constexpr (TAG) {
            const uint32_t* tp = p.btag + rb * 32u + 4u * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(tg[g]) : "v"(tp + 8 * g));
        }
    };
    auto landed = [&](u32x4 (&xa)[KSTEPS], f32x4v (&nx)[4], u32x4 (&tg)[4]) {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(nx[0]));
#pragma unroll
        for (int g = 1; g < 4; ++g) asm volatile("" : "+v"(nx[g]));
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) asm volatile("" : "+v"(xa[s]));
        if constexpr (TAG) {
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(tg[g]));
        }
    };
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // the products and the test of one block of rows against the QB query blocks
    auto sweep_block = [&](uint32_t rb, const u32x4 (&xa)[KSTEPS], const f32x4v (&nx)[4], const u32x4 (&tg)[4]) {
        f16x8 x[KSTEPS];
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) x[s] = __builtin_bit_cast(f16x8, xa[s]);
        float cinit[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            cinit[4 * g + 0] = scale * nx[g].x; cinit[4 * g + 1] = scale * nx[g].y;
            cinit[4 * g + 2] = scale * nx[g].z; cinit[4 * g + 3] = scale * nx[g].w;
        }
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[0], qh[b][0], zero, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[0], ql[b][0], acc, 0, 0, 0);
#pragma unroll
            for (int s = 1; s < KSTEPS; ++s) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[s], qh[b][s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[s], ql[b][s], acc, 0, 0, 0);
            }
            float t[16];  // q.x - 0.5 (1 - c) |x|^2: the scale undone and the norm added in one rounding
#pragma unroll
            for (int v = 0; v < 16; ++v) t[v] = __builtin_fmaf(acc[v], qinv[b], cinit[v]);
            float m = fmaxf(fmaxf(t[0], t[1]), t[2]);
#pragma unroll
            for (int v = 3; v < 15; v += 2) m = fmaxf(fmaxf(m, t[v]), t[v + 1]);
            m = fmaxf(m, t[15]);
            if (__builtin_expect(__ballot(m >= rhs[b]) != 0ull, 0)) {
                const uint32_t qv = q0 + 32u * b + r;   // (rhs = +inf beyond the batch: never here with qv >= nq)
                uint32_t hits = 0;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const uint32_t j = rb * 32u + (uint32_t)((v & 3) + 8 * (v >> 2)) + 4u * h;
                    hits |= (t[v] >= rhs[b] && j < p.rows) ? 1u << v : 0u;  // (a threshold of -inf -- list not full yet -- lets -inf through too)
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
    u32x4 xa0[KSTEPS], xa1[KSTEPS];
    f32x4v nx0[4], nx1[4];
    u32x4 tg0[4], tg1[4];
    request_block(b_lo, xa0, nx0, tg0);
    for (uint32_t rb = b_lo;;) {
        landed(xa0, nx0, tg0);
        if (rb + 1u < b_hi) request_block(rb + 1u, xa1, nx1, tg1);
        sweep_block(rb, xa0, nx0, tg0);
        if (++rb >= b_hi) break;
        landed(xa1, nx1, tg1);
        if (rb + 1u < b_hi) request_block(rb + 1u, xa0, nx0, tg0);
        sweep_block(rb, xa1, nx1, tg1);
        if (++rb >= b_hi) break;
    }
}

template <int KSTEPS, int QB, bool TAG>
hipError_t launch_half_sweep_tt(const KnnHalfSweepParams& p, hipStream_t s) {
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
    hipLaunchKernelGGL((knn_half_sweep_kernel<KSTEPS, QB, TAG>), dim3(gx, gy), dim3(256), 0, s, p);
    return hipGetLastError();
}

// The sweep instance of a row length, launch and name from one place: K steps of 16; query blocks per wavefront by what the operands
// leave of the register file (knn_filter_pick's table: the B operands are as many registers, the A sets half as many).
struct KnnHalfSweepPick {
    hipError_t (*launch)(const KnnHalfSweepParams&, hipStream_t);
    const char* name;
};
#define KNN_HALF_SWEEP(K, QB)                                                                                          \
    (tagged ? KnnHalfSweepPick{&launch_half_sweep_tt<K, QB, true>, "knn_half_sweep_kernel<" #K ", " #QB ", true>"} \
            : KnnHalfSweepPick{&launch_half_sweep_tt<K, QB, false>, "knn_half_sweep_kernel<" #K ", " #QB ", false>"})
KnnHalfSweepPick knn_half_sweep_pick(uint32_t dp, bool tagged) {
    if (dp & 15u) return KnnHalfSweepPick{nullptr, nullptr};
    switch (dp >> 4) {
        case 1: return KNN_HALF_SWEEP(1, 4);
        case 2: return KNN_HALF_SWEEP(2, 4);
        case 3: return KNN_HALF_SWEEP(3, 2);
        case 4: return KNN_HALF_SWEEP(4, 2);
        case 5: return KNN_HALF_SWEEP(5, 1);
        case 6: return KNN_HALF_SWEEP(6, 1);
        case 7: return KNN_HALF_SWEEP(7, 1);
        case 8: return KNN_HALF_SWEEP(8, 1);
        default: return KnnHalfSweepPick{nullptr, nullptr};
    }
}
#undef KNN_HALF_SWEEP
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
    const KnnHalfSweepPick k = knn_half_sweep_pick(p.dp, p.btag != nullptr);
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
