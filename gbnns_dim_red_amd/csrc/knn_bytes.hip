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
#include "knn_sweep.h"

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

// The sweep (knn_sweep.h has the division of work, the hand-issued loads and the hit path): lane (r, h) holds the 16 bytes
// 32 s + 16 h .. + 15 of K step s for both operands -- whatever order the instruction gives those 16 + 16 columns, it is the same for A
// and B, and a dot product does not see it.  A value is s = (x'.q' << shift) + bterm, kept when s >= thr[query], i.e. distance <= T_q;
// the kept pair is stored as its key: the distance qterm - s is final.
struct KnnBytesOps {
    typedef KnnBytesSweepParams Params;
    typedef int32_t Val;
    typedef i32x16 Vals;
    struct Q { int32_t thr, qterm; };
    static constexpr int kQFrags = 1, kRowFrags = 1;
    static constexpr bool kKeepsValue = true;
    // (a query beyond the batch keeps nothing: s never reaches INT32_MAX)
    static __device__ __forceinline__ Q load_q(const Params& p, uint32_t qi, bool ok) { return Q{ok ? p.thr[qi] : kPassNone, ok ? p.qterm[qi] : 0}; }
    static __device__ __forceinline__ void use_q(const Q& q) { asm volatile("" ::"v"(q.thr), "v"(q.qterm)); }
    static __device__ __forceinline__ const uint4* q_ptr(const Params& p, uint32_t qi) {
        return reinterpret_cast<const uint4*>(p.qpack + (size_t)qi * p.dp);
    }
    static __device__ __forceinline__ const char* row_ptr(const Params& p, uint32_t j, uint32_t h) {
        return reinterpret_cast<const char*>(p.bpack + (size_t)j * p.dp + 16u * h);
    }
    static __device__ __forceinline__ uint32_t row_off(const Params&, int s, uint32_t) { return 32u * (uint32_t)s; }
    static __device__ __forceinline__ const uint32_t* side(const Params& p) { return reinterpret_cast<const uint32_t*>(p.bterm); }
    static __device__ __forceinline__ Vals rows_init(const knn_u32x4 (&bt)[4]) {
        Vals c;
#pragma unroll
        for (int v = 0; v < 16; ++v) c[v] = (int32_t)bt[v >> 2][v & 3];
        return c;
    }
    template <int KSTEPS>
    static __device__ __forceinline__ Vals tile(const Params& p, const knn_u32x4 (&x)[KSTEPS], const Vals& bterm, const knn_u32x4 (&qf)[KSTEPS], const Q&) {
        i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, x[s]), __builtin_bit_cast(i32x4, qf[s]), acc, 0, 0, 0);
        Vals sv;
#pragma unroll
        for (int v = 0; v < 16; ++v) sv[v] = (int32_t)((uint32_t)acc[v] << p.shift) + bterm[v];  // distance = qterm - sv
        return sv;
    }
    static __device__ __forceinline__ uint64_t kept(const Q& q, uint32_t id, int32_t sv) {
        const float dist = (float)(q.qterm - sv);  // exact: an integer of magnitude < 2^24
        return ((uint64_t)knn_fkey(dist) << 32) | id;
    }
};
template <int KSTEPS, int QB, bool TAG>
__global__ __launch_bounds__(256) void knn_bytes_sweep_kernel(KnnBytesSweepParams p) {
    knn_sweep_body<KnnBytesOps, KSTEPS, QB, TAG>(p);
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

// K steps of 32 bytes; one 16-byte B fragment per step: twice the query blocks of the two-part sweeps
KNN_SWEEP_PICK_FN(knn_bytes_sweep_pick, knn_bytes_sweep_kernel, KnnBytesSweepParams, kKnnBytesKStep, 4, 4, 4, 4, 2, 2, 2, 2)
#undef KNN_SWEEP_PICK_FN
#undef KNN_SWEEP_PICK_FN_
#undef KNN_SWEEP_CASE_
#undef KNN_SWEEP_INSTANCE_
#undef KNN_SWEEP_QB_TWO_PART
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
    const auto k = knn_bytes_sweep_pick(p.dp, p.btag != nullptr);
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
