// knn_bytes.hip -- exact brute-force kNN over uint8 rows on the int8 matrix cores of gfx950 (MI355X).
//
// Same answer as the float scan of knn.hip over the widened rows, bit for bit: for uint8 x, q and d <= 256 every
// intermediate of L2Metric::Dist / Angular::Dist (support_func.h:107-163) on float(x), float(q) is an integer below 2^24
// (differences <= 255, squares <= 65 025, every running sum and fold <= 256 * 65 025 = 16 646 400), so each float
// operation is exact and the result is the integer sum(x - q)^2 -- or -sum(x q) -- whatever the order of summation.
// v_mfma_i32_32x32x32_i8 computes such integers in int32.  So here the matrix-core product is not a filter in front of
// an exact distance: it is the distance.  Nothing is rescored; the keys the sweep writes are the keys the lists hold.
//
//   pack   uint8 -> signed x' = x - 128 (the instruction is signed; L2 does not see the common shift, the dot product
//          is put right with the row sums), K padded to 32 with signed zeros, one int32 term per row (kernels.h)
//   sweep  queries = operand B in registers, blocks of 32 base rows = operand A from global memory; the distance of
//          every pair in integer VALU; pairs with distance <= T_q (the query's k-th distance so far; `<=`: a tie with
//          a lower id still enters) appended as (knn_fkey(float(distance)) << 32 | id)
//   offer  the appended keys into the query's heap (short lists) or pool + radix select (long lists), new T_q
//   sort   knn_finalize_kernel / knn_pool_finalize_kernel of knn.hip, unchanged: they see the same keys
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "knn_select.h"

namespace gbnns {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int32_t kPassAll = INT32_MIN;   // threshold of a list that is not full yet
constexpr int32_t kPassNone = INT32_MAX;  // ... of a lane without a query

// G (a power of two >= dp / 16) neighbouring lanes per row, lane g packs columns 16 g .. 16 g + 15: one 16-byte store;
// the row's sum of squares and sum are folded over the G lanes.  `used` = columns that count (4 floor(d / 4) for L2).
template <int G>
__global__ __launch_bounds__(256) void knn_bytes_pack_kernel(const uint8_t* x, uint32_t stride, uint32_t dim, uint32_t used, uint32_t dp, uint64_t rows,
                                                             int neg_dot, int query_side, int8_t* packed, int32_t* term) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = e / G;
    const uint32_t g = (uint32_t)(e % G);
    const bool live = row < rows && g * 16u < dp;
    int32_t n2 = 0, sm = 0;
    if (live) {
        const uint8_t* xr = x + (size_t)row * stride;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t col = g * 16u + j;
            const int32_t v = col < used ? (int32_t)xr[col] - 128 : 0;  // (= the byte with its top bit flipped, read as signed)
            n2 += v * v;
            sm += v;
            w[j >> 2] |= ((uint32_t)v & 255u) << (8 * (j & 3));
        }
        *reinterpret_cast<uint4*>(packed + (size_t)row * dp + g * 16u) = make_uint4(w[0], w[1], w[2], w[3]);
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {  // (every lane of the wavefront takes part: idle lanes add zeros)
        n2 += __shfl_xor(n2, m);
        sm += __shfl_xor(sm, m);
    }
    if (live && g == 0) {
        int32_t t;
        if (!neg_dot) t = query_side ? n2 : -n2;
        else t = query_side ? -128 * sm - 16384 * (int32_t)dim : 128 * sm;
        term[row] = t;
    }
}

__device__ __forceinline__ int32_t knn_bytes_thr(uint64_t root, int32_t qterm) {
    // (the k-th distance is an integer of magnitude < 2^24: the conversion back is exact)
    return root == ~0ull ? kPassAll : qterm - (int32_t)knn_fkey_inv((uint32_t)(root >> 32));
}

// A workgroup = 4 wavefronts x QB blocks of 32 queries (operand B, in registers for the whole launch: the lane's column
// of every 32 x 32 tile is ITS query, so one threshold per lane and block); blockIdx.y picks a slab of the chunk's rows,
// walked in blocks of 32 (operand A straight from global memory, the next block requested before the current block's
// products).  Lane (r, h) holds row / query r and the 16 bytes 32 s + 16 h .. + 15 of K step s for both operands: whatever
// order the instruction gives those 16 + 16 columns, it is the same for A and B, and a dot product does not see it.
// C/D: register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h of the block, column r.
// TAG (gbnns_exact_knn_bytes_tagged): a pair whose row is not allowed for its query -- (btag[row] & qtag[query]) == 0 -- is not a hit.  The
// tag words of a lane's 16 rows travel with the block's terms (four more 16-byte requests, same address pattern, the array padded like
// bterm) and are looked at where hits are counted, as in knn_filter_kernel: DESIGN.md 5.1 has the measurement against a fetch there.
template <int KSTEPS, int QB, bool TAG>
__global__ __launch_bounds__(256) void knn_bytes_sweep_kernel(KnnBytesSweepParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint32_t q0 = (blockIdx.x * 4u + wave) * (QB * 32u);
    if (q0 >= p.nq) return;
    i32x4 qf[QB][KSTEPS];
    int32_t thr[QB], qterm[QB];
    uint32_t qtag[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        const uint32_t qi = q0 + 32u * b + r;
        const bool ok = qi < p.nq;
        const int8_t* qp = p.qpack + (size_t)(ok ? qi : 0u) * p.dp + 16u * h;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) qf[b][s] = *reinterpret_cast<const i32x4*>(qp + 32 * s);
        thr[b] = ok ? p.thr[qi] : kPassNone;  // (a query beyond the batch keeps nothing: s never reaches INT32_MAX)
        qterm[b] = ok ? p.qterm[qi] : 0;
        if constexpr (TAG) qtag[b] = ok ? p.qtag[qi] : 0u;
    }
    // (every compiler-issued load is used here, once: its waits then sit in this prologue and not inside the sweep)
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        asm volatile("" ::"v"(thr[b]), "v"(qterm[b]));
        if constexpr (TAG) asm volatile("" ::"v"(qtag[b]));
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) asm volatile("" ::"v"(qf[b][s]));
    }
    const uint32_t blocks = (p.rows + 31u) >> 5;
    const uint32_t per = (blocks + gridDim.y - 1) / gridDim.y;
    const uint32_t b_lo = blockIdx.y * per, b_hi = min(blocks, b_lo + per);
    if (b_lo >= b_hi) return;
    // Fragments and terms of one block of 32 rows (rows beyond the chunk read row 0; the terms' array is readable 64
    // entries beyond the set; such a row is refused where the hits are stored), requested by hand-written loads, as in
    // knn_filter_kernel (knn.hip): `landed` is the one wait, placed in front of the next requests.
    auto request_block = [&](uint32_t rb, i32x4 (&xa)[KSTEPS], i32x4 (&bt)[4], i32x4 (&tg)[4]) {
        const uint32_t j = rb * 32u + r;
        const int8_t* bp = p.bpack + (size_t)(j < p.rows ? j : 0u) * p.dp + 16u * h;
        const int32_t* np = p.bterm + rb * 32u + 4u * h;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xa[s]) : "v"(bp + 32 * s));
#pragma unroll
        for (int g = 0; g < 4; ++g)  // accumulator registers 4 g .. 4 g + 3 = rows 8 g + 4 h + 0 .. 3 of the block
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bt[g]) : "v"(np + 8 * g));
        if constexpr (TAG) {
            const uint32_t* tp = p.btag + rb * 32u + 4u * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(tg[g]) : "v"(tp + 8 * g));
        }
    };
    auto landed = [&](i32x4 (&xa)[KSTEPS], i32x4 (&bt)[4], i32x4 (&tg)[4]) {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(bt[0]));
#pragma unroll
        for (int g = 1; g < 4; ++g) asm volatile("" : "+v"(bt[g]));
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) asm volatile("" : "+v"(xa[s]));
        if constexpr (TAG) {
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(tg[g]));
        }
    };
    const i32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto sweep_block = [&](uint32_t rb, const i32x4 (&xa)[KSTEPS], const i32x4 (&bt)[4], const i32x4 (&tg)[4]) {
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            i32x16 acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa[0], qf[b][0], zero, 0, 0, 0);
#pragma unroll
            for (int s = 1; s < KSTEPS; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa[s], qf[b][s], acc, 0, 0, 0);
            int32_t sv[16];
#pragma unroll
            for (int v = 0; v < 16; ++v) sv[v] = (int32_t)((uint32_t)acc[v] << p.shift) + bt[v >> 2][v & 3];  // distance = qterm - sv
            int32_t m = max(max(sv[0], sv[1]), sv[2]);
#pragma unroll
            for (int v = 3; v < 15; v += 2) m = max(max(m, sv[v]), sv[v + 1]);
            m = max(m, sv[15]);
            if (__builtin_expect(__ballot(m >= thr[b]) != 0ull, 0)) {
                // one returning atomic per lane with hits (its 16 rows of the tile): the places of all of them at once
                const uint32_t qv = q0 + 32u * b + r;  // (thr = INT32_MAX beyond the batch: never here with qv >= nq)
                uint32_t hits = 0;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const uint32_t j = rb * 32u + (uint32_t)((v & 3) + 8 * (v >> 2)) + 4u * h;
                    hits |= (sv[v] >= thr[b] && j < p.rows) ? 1u << v : 0u;
                }
                if constexpr (TAG) {
                    uint32_t m = 0;
#pragma unroll
                    for (int v = 0; v < 16; ++v) m |= (((uint32_t)tg[v >> 2][v & 3] & qtag[b]) ? 1u : 0u) << v;
                    hits &= m;
                }
                if (hits) {
                    uint32_t pos = atomicAdd(&p.count[qv], (uint32_t)__popc(hits));
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        if (hits & (1u << v)) {
                            const uint32_t id = p.row0 + rb * 32u + (uint32_t)((v & 3) + 8 * (v >> 2)) + 4u * h;
                            const float dist = (float)(qterm[b] - sv[v]);  // exact: an integer of magnitude < 2^24
                            if (pos < p.cap) p.cand[(size_t)qv * p.cap + pos] = ((uint64_t)knn_fkey(dist) << 32) | id;
                            else *p.overflow = 1u;
                            pos += 1u;
                        }
                    }
                }
            }
        }
    };
    // two register sets in turn: wait for the set at hand, request the next block into the other one, sweep
    i32x4 xa0[KSTEPS], xa1[KSTEPS], bt0[4], bt1[4], tg0[4], tg1[4];
    request_block(b_lo, xa0, bt0, tg0);
    for (uint32_t rb = b_lo;;) {
        landed(xa0, bt0, tg0);
        if (rb + 1u < b_hi) request_block(rb + 1u, xa1, bt1, tg1);
        sweep_block(rb, xa0, bt0, tg0);
        if (++rb >= b_hi) break;
        landed(xa1, bt1, tg1);
        if (rb + 1u < b_hi) request_block(rb + 1u, xa0, bt0, tg0);
        sweep_block(rb, xa1, bt1, tg1);
        if (++rb >= b_hi) break;
    }
}

// One thread per query: the keys the sweep kept, offered to the query's heap (knn_rescore_kernel of knn.hip without the
// gather and the distance: the key is stored); then the query's new threshold.
__global__ __launch_bounds__(128) void knn_bytes_offer_heap_kernel(KnnBytesOfferParams p) {
    const uint32_t qi = blockIdx.x * 128u + threadIdx.x;
    if (qi >= p.nq) return;
    uint64_t root = p.heap[qi];
    const uint32_t cnt = min(p.count[qi], p.cap);
    for (uint32_t e = 0; e < cnt; ++e) {
        const uint64_t key = p.cand[(size_t)qi * p.cap + e];
        const bool self = p.self_offset >= 0 && (uint64_t)(uint32_t)key == (uint64_t)qi + (uint64_t)p.self_offset;
        if (!self && key < root) root = heap_replace_root(p.heap + qi, p.heap_stride, p.k, key);
    }
    p.thr[qi] = knn_bytes_thr(root, p.qterm[qi]);
}

// One wavefront per query: knn_pool_update_kernel of knn.hip on the stored keys.
__global__ __launch_bounds__(64) void knn_bytes_offer_pool_kernel(KnnBytesOfferParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_bytes_smem[];
    const uint32_t qi = blockIdx.x;
    const int lane = threadIdx.x;
    const int k = p.k;
    const uint32_t cnt = min(p.count[qi], p.cap);
    if (cnt == 0) return;  // (threshold unchanged)
    uint64_t* keys = reinterpret_cast<uint64_t*>(knn_bytes_smem);
    uint32_t* hist = reinterpret_cast<uint32_t*>(keys + k + kPoolNew);
    uint64_t* pool = p.pool + (size_t)qi * (size_t)k;
    for (int i = lane; i < k; i += 64) keys[i] = pool[i];
    uint64_t root = p.root[qi];
    __syncthreads();
    int nnew = 0;
    for (uint32_t e0 = 0; e0 < cnt; e0 += 64) {
        const uint32_t e = e0 + (uint32_t)lane;
        const bool valid = e < cnt;
        const uint64_t key = valid ? p.cand[(size_t)qi * p.cap + e] : ~0ull;
        const bool self = p.self_offset >= 0 && (uint64_t)(uint32_t)key == (uint64_t)qi + (uint64_t)p.self_offset;
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
        p.thr[qi] = knn_bytes_thr(root, p.qterm[qi]);
    }
}

template <int G>
hipError_t launch_pack_t(const uint8_t* x, uint32_t stride, uint32_t dim, uint32_t used, uint32_t dp, uint64_t rows, int neg_dot, int query_side, int8_t* packed,
                         int32_t* term, hipStream_t s) {
    const uint64_t threads = rows * G;
    hipLaunchKernelGGL(knn_bytes_pack_kernel<G>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, x, stride, dim, used, dp, rows, neg_dot,
                       query_side, packed, term);
    return hipGetLastError();
}

template <int KSTEPS, int QB, bool TAG>
hipError_t launch_sweep_tt(const KnnBytesSweepParams& p, hipStream_t s) {
    const unsigned gx = (p.nq + QB * 128u - 1) / (QB * 128u);
    const unsigned blocks = (p.rows + 31u) >> 5;
    static const unsigned simds = [] {  // 4 SIMDs per CU of the current device (the MI355X: 1 024)
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return 4u * (unsigned)cus;
    }();
    unsigned gy = gx >= simds ? 1u : (simds + gx - 1) / gx;  // enough workgroups for every SIMD
    if (gy > blocks) gy = blocks;
    if (gy < 1u) gy = 1u;
    hipLaunchKernelGGL((knn_bytes_sweep_kernel<KSTEPS, QB, TAG>), dim3(gx, gy), dim3(256), 0, s, p);
    return hipGetLastError();
}

// The sweep instance of a packed row length, launch and name from one place: K steps of 32; query blocks per wavefront by what the
// operands leave of the register file.
struct KnnBytesSweepPick {
    hipError_t (*launch)(const KnnBytesSweepParams&, hipStream_t);
    const char* name;
};
#define KNN_BYTES_SWEEP(K, QB)                                                                                              \
    (tagged ? KnnBytesSweepPick{&launch_sweep_tt<K, QB, true>, "knn_bytes_sweep_kernel<" #K ", " #QB ", true>"} \
            : KnnBytesSweepPick{&launch_sweep_tt<K, QB, false>, "knn_bytes_sweep_kernel<" #K ", " #QB ", false>"})
KnnBytesSweepPick knn_bytes_sweep_pick(uint32_t dp, bool tagged) {
    if (dp % kKnnBytesKStep) return KnnBytesSweepPick{nullptr, nullptr};
    switch (dp / kKnnBytesKStep) {
        case 1: return KNN_BYTES_SWEEP(1, 4);
        case 2: return KNN_BYTES_SWEEP(2, 4);
        case 3: return KNN_BYTES_SWEEP(3, 4);
        case 4: return KNN_BYTES_SWEEP(4, 4);
        case 5: return KNN_BYTES_SWEEP(5, 2);
        case 6: return KNN_BYTES_SWEEP(6, 2);
        case 7: return KNN_BYTES_SWEEP(7, 2);
        case 8: return KNN_BYTES_SWEEP(8, 2);
        default: return KnnBytesSweepPick{nullptr, nullptr};
    }
}
#undef KNN_BYTES_SWEEP
}  // namespace

hipError_t launch_knn_bytes_pack(const uint8_t* x, uint32_t stride, uint32_t dim, uint32_t dp, int metric, int query_side, uint64_t rows, int8_t* packed,
                                 int32_t* term, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    if (dim == 0 || dim > 256 || stride < dim || dp < dim || dp % kKnnBytesKStep || dp > 256) return hipErrorInvalidValue;
    const int neg_dot = metric == 1;
    const uint32_t used = neg_dot ? dim : dim & ~3u;  // L2Metric::Dist reads the first 4 floor(d / 4) dimensions
    const uint32_t groups = dp / 16u;
    if (groups <= 2) return launch_pack_t<2>(x, stride, dim, used, dp, rows, neg_dot, query_side, packed, term, s);
    if (groups <= 4) return launch_pack_t<4>(x, stride, dim, used, dp, rows, neg_dot, query_side, packed, term, s);
    if (groups <= 8) return launch_pack_t<8>(x, stride, dim, used, dp, rows, neg_dot, query_side, packed, term, s);
    return launch_pack_t<16>(x, stride, dim, used, dp, rows, neg_dot, query_side, packed, term, s);
}

hipError_t launch_knn_bytes_sweep(const KnnBytesSweepParams& p, hipStream_t s) {
    if (p.nq == 0 || p.rows == 0) return hipSuccess;
    if (p.btag && !p.qtag) return hipErrorInvalidValue;
    const KnnBytesSweepPick k = knn_bytes_sweep_pick(p.dp, p.btag != nullptr);
    return k.launch ? k.launch(p, s) : hipErrorInvalidValue;
}
const char* knn_bytes_sweep_kernel_name(uint32_t dp, bool tagged) { return knn_bytes_sweep_pick(dp, tagged).name; }

hipError_t launch_knn_bytes_offer(const KnnBytesOfferParams& p, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (!p.pool) {
        hipLaunchKernelGGL(knn_bytes_offer_heap_kernel, dim3((p.nq + 127u) / 128u), dim3(128), 0, s, p);
        return hipGetLastError();
    }
    const size_t lds = ((size_t)p.k + kPoolNew) * 8 + 256 * 4;  // k <= 4 096: 42 KB at the most
    hipLaunchKernelGGL(knn_bytes_offer_pool_kernel, dim3(p.nq), dim3(64), lds, s, p);
    return hipGetLastError();
}

}  // namespace gbnns
