// rerank_bytes.hip -- the stand-alone re-rank kernels of a byte handle (gbnns_index_create_bytes): rerank.hip's four kernels over rows of
// uint8 coordinates.  A byte is widened by one conversion (v_cvt_f32_ubyte0..3) and is exact in binary32, so every distance is the float
// kernels' distance on float32(db_bytes), bit for bit: the same operations in the same order (walk_common.h: l2_ordered / negdot_ordered
// through the ByteRow4 adapter, rerank_bytes_core for the chunk-pair form).  The query is staged as floats in LDS, the k-answer selection is
// rerank_topk.h's.
#include "launch_util.h"
#include "rerank_topk.h"

namespace gbnns {

namespace {

// (RerankBytesParams: dstride = bytes of a row = floats of the staged query, a multiple of 16; k == 0 in the one-answer launches)
__device__ __forceinline__ void bytes_keep(const RerankBytesParams& p, const TopkLds& t, int r, float dv) {
    t.keys[r] = ((uint64_t)fkey(dv) << 32) | (uint32_t)r;
    t.dist[r] = dv;
}

// a lane per row: the negative dot product, and L2 at d % 16 != 0 (the d % 4 tail ignored, as in the float kernel)
template <int METRIC, bool TOPK>
__global__ __launch_bounds__(64) void rerank_bytes_kernel(RerankBytesParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const uint32_t qi = blockIdx.x;
    float* qf = reinterpret_cast<float*>(smem);
    const float4* qs = reinterpret_cast<const float4*>(qf);
    for (uint32_t i = lane; i < p.dstride; i += 64)
        qf[i] = (i < p.dim) ? p.q[(size_t)qi * p.qstride + i] : 0.f;
    wave_sync();
    const int cnt = topk_count(p, qi);
    const uint32_t* cand = p.cand + (size_t)qi * p.cand_stride;
    TopkLds t{};
    if constexpr (TOPK) t = topk_lds(smem, p);
    uint64_t bestk = ~0ull;
    for (int base = 0; base < cnt; base += 64) {
        const int r = base + lane;
        if (r < cnt) {
            uint32_t id = cand[r];
            id = id < p.n ? id : 0u;  // (never dereference an id outside the table)
            const ByteRow4 row{reinterpret_cast<const uint32_t*>(p.db_b + (size_t)id * p.dstride)};
            const float dv = metric_dist<METRIC>(row, qs, p.dim);
            if constexpr (TOPK) {
                bytes_keep(p, t, r, dv);
            } else {
                const uint64_t kv = ((uint64_t)fkey(dv) << 32) | (uint32_t)r;
                bestk = kv < bestk ? kv : bestk;
            }
        }
    }
    if constexpr (TOPK) {
        topk_select(p, t, cand, qi, cnt, lane);
    } else {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = shfl_u64(bestk, lane ^ off);
            bestk = o < bestk ? o : bestk;
        }
        if (lane == 0) p.out[qi] = (cnt > 0) ? cand[(uint32_t)(bestk & 0xFFFFFFFFu)] : kInvalidId;
    }
}

// the chunk-pair form: L2, d % 16 == 0
template <bool TOPK>
__global__ __launch_bounds__(64) void rerank_bytes_pair_kernel(RerankBytesParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const uint32_t qi = blockIdx.x;
    const int cnt = topk_count(p, qi);
    const uint32_t* cand = p.cand + (size_t)qi * p.cand_stride;
    const RerankBytesSrc a{p.q, p.qstride, p.db_b, p.dstride, p.dim, p.n};
    auto id_at = [&](int r) { return cand[r]; };
    if constexpr (TOPK) {
        const TopkLds t = topk_lds(smem, p);
        rerank_bytes_core(a, qi, cnt, reinterpret_cast<float*>(smem), lane, id_at, [&](int r, float dv) { bytes_keep(p, t, r, dv); });
        topk_select(p, t, cand, qi, cnt, lane);
    } else {
        const int win = rerank_bytes_core(a, qi, cnt, reinterpret_cast<float*>(smem), lane, id_at);
        if (lane == 0) p.out[qi] = (win >= 0) ? cand[win] : kInvalidId;
    }
}

template <typename K>
hipError_t launch_bytes(K kernel, const RerankBytesParams& p, size_t lds, hipStream_t s) {
    const hipError_t e = set_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(p.nq), dim3(64), lds, s, p);
    return hipGetLastError();
}

bool bytes_shape_ok(const RerankBytesParams& p) { return p.db_b && p.dim > 0 && p.dstride % 16 == 0 && p.dstride >= p.dim; }

}  // namespace

hipError_t launch_rerank_bytes(const RerankBytesParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (!bytes_shape_ok(p)) return hipErrorInvalidValue;
    const size_t lds = (size_t)p.dstride * 4;
    if (metric == 1) return launch_bytes(rerank_bytes_kernel<1, false>, p, lds, s);  // (never the chunk-pair form: rerank_plan.h)
    if (rerank_plan(metric, p.dim, true).form == RerankForm::ChunkPairs) return launch_bytes(rerank_bytes_pair_kernel<false>, p, lds, s);
    return launch_bytes(rerank_bytes_kernel<0, false>, p, lds, s);
}

hipError_t launch_rerank_topk_bytes(const RerankBytesParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (!bytes_shape_ok(p) || p.k == 0 || p.k > p.cand_stride) return hipErrorInvalidValue;
    const size_t lds = rerank_topk_lds(p.dstride, p.cand_stride);
    if (metric == 1) return launch_bytes(rerank_bytes_kernel<1, true>, p, lds, s);
    if (rerank_plan(metric, p.dim, true).form == RerankForm::ChunkPairs) return launch_bytes(rerank_bytes_pair_kernel<true>, p, lds, s);
    return launch_bytes(rerank_bytes_kernel<0, true>, p, lds, s);
}

}  // namespace gbnns
