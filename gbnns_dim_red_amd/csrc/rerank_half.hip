// rerank_half.hip -- the stand-alone re-rank kernels of a half-base handle (gbnns_index_create_half_base): rerank.hip's four kernels over rows
// of IEEE binary16 coordinates.  A half is widened by one conversion (v_cvt_f32_f16; no flush flag on this unit: binary16 subnormals are
// kept) and is exact in binary32, so every distance is the float kernels' distance on float32(db_half), bit for bit: the same operations in
// the same order, multiply and add separate (walk_common.h: l2_ordered / negdot_ordered through the HalfRow4 adapter, rerank_half_core for
// the chunk-pair form).  The query is staged as floats in LDS and never rounded, the k-answer selection is rerank_topk.h's.
#include "launch_util.h"
#include "rerank_topk.h"

namespace gbnns {

namespace {

// (RerankHalfParams: dstride = halves of a row = floats of the staged query, a multiple of 8; k == 0 in the one-answer launches)
__device__ __forceinline__ void half_keep(const TopkLds& t, int r, float dv) {
    t.keys[r] = ((uint64_t)fkey(dv) << 32) | (uint32_t)r;
    t.dist[r] = dv;
}

// a lane per row: the negative dot product (any d: the masked tail meets the row's zero padding), and L2 at d % 4 != 0 (the tail ignored, as
// in the float kernel)
template <int METRIC, bool TOPK>
__global__ __launch_bounds__(64) void rerank_half_kernel(RerankHalfParams p) {
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
            const HalfRow4 row{reinterpret_cast<const uint2*>(p.db_h + (size_t)id * p.dstride)};
            const float dv = metric_dist<METRIC>(row, qs, p.dim);
            if constexpr (TOPK) {
                half_keep(t, r, dv);
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

// the chunk-pair form: L2, d % 4 == 0.  DEEP: rerank_plan.h's rerank_half_deep of the row length (the launcher picks the instance).
template <bool TOPK, int DEEP>
__global__ __launch_bounds__(64) void rerank_half_pair_kernel(RerankHalfParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const uint32_t qi = blockIdx.x;
    const int cnt = topk_count(p, qi);
    const uint32_t* cand = p.cand + (size_t)qi * p.cand_stride;
    const RerankHalfSrc a{p.q, p.qstride, p.db_h, p.dstride, p.dim, p.n};
    auto id_at = [&](int r) { return cand[r]; };
    if constexpr (TOPK) {
        const TopkLds t = topk_lds(smem, p);
        rerank_half_core<DEEP>(a, qi, cnt, reinterpret_cast<float*>(smem), lane, id_at, [&](int r, float dv) { half_keep(t, r, dv); });
        topk_select(p, t, cand, qi, cnt, lane);
    } else {
        const int win = rerank_half_core<DEEP>(a, qi, cnt, reinterpret_cast<float*>(smem), lane, id_at);
        if (lane == 0) p.out[qi] = (win >= 0) ? cand[win] : kInvalidId;
    }
}

template <typename K>
hipError_t launch_half(K kernel, const RerankHalfParams& p, size_t lds, hipStream_t s) {
    const hipError_t e = set_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(p.nq), dim3(64), lds, s, p);
    return hipGetLastError();
}

bool half_shape_ok(const RerankHalfParams& p) {
    return p.db_h && (reinterpret_cast<uintptr_t>(p.db_h) & 15u) == 0 && p.dim > 0 && p.dstride % 8 == 0 && p.dstride >= p.dim;
}

template <bool TOPK>
hipError_t launch_half_form(const RerankHalfParams& p, int metric, size_t lds, hipStream_t s) {
    if (metric == 1) return launch_half(rerank_half_kernel<1, TOPK>, p, lds, s);  // (never the chunk-pair form: rerank_plan.h)
    const RerankPlan plan = rerank_half_plan(metric, p.dim);
    if (plan.form != RerankForm::HalfChunkPairs) return launch_half(rerank_half_kernel<0, TOPK>, p, lds, s);
    if (plan.deep > 4) return launch_half(rerank_half_pair_kernel<TOPK, GBNNS_HALF_RERANK_DEEP>, p, lds, s);
    return launch_half(rerank_half_pair_kernel<TOPK, 4>, p, lds, s);
}

}  // namespace

hipError_t launch_rerank_half(const RerankHalfParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (!half_shape_ok(p)) return hipErrorInvalidValue;
    return launch_half_form<false>(p, metric, (size_t)p.dstride * 4, s);
}

hipError_t launch_rerank_topk_half(const RerankHalfParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (!half_shape_ok(p) || p.k == 0 || p.k > p.cand_stride) return hipErrorInvalidValue;
    return launch_half_form<true>(p, metric, rerank_topk_lds(p.dstride, p.cand_stride), s);
}

}  // namespace gbnns
