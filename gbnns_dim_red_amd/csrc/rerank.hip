// rerank.hip -- the stand-alone re-rank kernels (getRealNearest, search_function.h:105-125): gbnns_rerank, d % 8 != 0 and
// GBNNS_FLAG_NO_FUSED_RERANK; the walk kernels re-rank their own query through the same core (walk_common.h).  And their k-answer
// forms (gbnns_rerank_topk, gbnns_search_topk): the same distances, every one of them kept, the k smallest reported in order.
#include "launch_util.h"
#include "rerank_topk.h"

namespace gbnns {

namespace {

// ------------------------------------------------------------------------------------------
// re-rank (search_function.h:105-125 getRealNearest)
// ------------------------------------------------------------------------------------------
// One candidate per lane; each lane streams its own row with 16-B loads against the query staged
// in LDS.  Winner = strict minimum in pop order  <=>  min over (distance, pop index).

template <int METRIC>
__global__ __launch_bounds__(64) void rerank_kernel(RerankParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const uint32_t qi = blockIdx.x;
    float* qf = reinterpret_cast<float*>(smem);
    const float4* qs = reinterpret_cast<const float4*>(qf);
    for (uint32_t i = lane; i < p.dstride; i += 64)
        qf[i] = (i < p.dim) ? p.q[(size_t)qi * p.qstride + i] : 0.f;
    wave_sync();
    const int cnt = p.count[qi];
    const uint32_t* cand = p.cand + (size_t)qi * p.cand_stride;
    uint64_t bestk = ~0ull;
    for (int base = 0; base < cnt; base += 64) {
        const int r = base + lane;
        if (r < cnt) {
            uint32_t id = cand[r];
            id = id < p.n ? id : 0u;  // (never dereference an id outside the table)
            const float dv = metric_dist<METRIC>(
                reinterpret_cast<const float4*>(p.db + (size_t)id * p.dstride), qs, p.dim);
            const uint64_t kv = ((uint64_t)fkey(dv) << 32) | (uint32_t)r;
            bestk = kv < bestk ? kv : bestk;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = shfl_u64(bestk, lane ^ off);
        bestk = o < bestk ? o : bestk;
    }
    if (lane == 0) p.out[qi] = (cnt > 0) ? cand[(uint32_t)(bestk & 0xFFFFFFFFu)] : kInvalidId;
}

template <int METRIC>
__global__ __launch_bounds__(64) void rerank_pair_kernel(RerankParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const uint32_t qi = blockIdx.x;
    const int cnt = p.count[qi];
    const uint32_t* cand = p.cand + (size_t)qi * p.cand_stride;
    RerankSrc a{p.q, p.qstride, p.db, p.dstride, p.dim, p.n};
    const int win = rerank_pairs_deep(METRIC, p.dim) == 24
                        ? rerank_pairs_core<METRIC, 24>(a, qi, cnt, reinterpret_cast<float*>(smem), lane, [&](int r) { return cand[r]; })
                        : rerank_pairs_core<METRIC>(a, qi, cnt, reinterpret_cast<float*>(smem), lane, [&](int r) { return cand[r]; });
    if (lane == 0) p.out[qi] = (win >= 0) ? cand[win] : kInvalidId;
}

// (the k-answer selection -- TopkLds, topk_select, topk_count -- is rerank_topk.h's, shared with the byte-row kernels of rerank_bytes.hip)

// a lane per row (d % 8 != 0 for the dot metric, d % 4 != 0 for L2): rerank_kernel's distances
template <int METRIC>
__global__ __launch_bounds__(64) void rerank_topk_kernel(RerankTopkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const uint32_t qi = blockIdx.x;
    float* qf = reinterpret_cast<float*>(smem);
    const float4* qs = reinterpret_cast<const float4*>(qf);
    const TopkLds t = topk_lds(smem, p);
    for (uint32_t i = lane; i < p.dstride; i += 64)
        qf[i] = (i < p.dim) ? p.q[(size_t)qi * p.qstride + i] : 0.f;
    wave_sync();
    const int cnt = topk_count(p, qi);
    const uint32_t* cand = p.cand + (size_t)qi * p.cand_stride;
    for (int base = 0; base < cnt; base += 64) {
        const int r = base + lane;
        if (r < cnt) {
            uint32_t id = cand[r];
            id = id < p.n ? id : 0u;  // (never dereference an id outside the table)
            const float dv = metric_dist<METRIC>(
                reinterpret_cast<const float4*>(p.db + (size_t)id * p.dstride), qs, p.dim);
            t.keys[r] = ((uint64_t)fkey(dv) << 32) | (uint32_t)r;
            t.dist[r] = dv;
        }
    }
    topk_select(p, t, cand, qi, cnt, lane);
}

// the pair form (rerank_pairs_core, all its shapes): the core's sink keeps what rerank_pair_kernel folds into a minimum
template <int METRIC>
__global__ __launch_bounds__(64) void rerank_topk_pair_kernel(RerankTopkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const uint32_t qi = blockIdx.x;
    const int cnt = topk_count(p, qi);
    const uint32_t* cand = p.cand + (size_t)qi * p.cand_stride;
    const TopkLds t = topk_lds(smem, p);
    RerankSrc a{p.q, p.qstride, p.db, p.dstride, p.dim, p.n};
    auto id_at = [&](int r) { return cand[r]; };
    auto keep = [&](int r, float dv) {
        t.keys[r] = ((uint64_t)fkey(dv) << 32) | (uint32_t)r;
        t.dist[r] = dv;
    };
    if (rerank_pairs_deep(METRIC, p.dim) == 24) rerank_pairs_core<METRIC, 24>(a, qi, cnt, reinterpret_cast<float*>(smem), lane, id_at, 0, 1, nullptr, keep);
    else rerank_pairs_core<METRIC>(a, qi, cnt, reinterpret_cast<float*>(smem), lane, id_at, 0, 1, nullptr, keep);
    topk_select(p, t, cand, qi, cnt, lane);
}

}  // namespace

hipError_t launch_rerank(const RerankParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    const size_t lds = (size_t)p.dstride * 4;
    const bool pairs = rerank_plan(metric, p.dim, false).form == RerankForm::Pairs;
    hipError_t e;
    if (metric == 1) {
        if (pairs) {
            e = set_lds(rerank_pair_kernel<1>, lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((rerank_pair_kernel<1>), dim3(p.nq), dim3(64), lds, s, p);
        } else {
            e = set_lds(rerank_kernel<1>, lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((rerank_kernel<1>), dim3(p.nq), dim3(64), lds, s, p);
        }
    } else if (pairs) {
        e = set_lds(rerank_pair_kernel<0>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((rerank_pair_kernel<0>), dim3(p.nq), dim3(64), lds, s, p);
    } else {
        e = set_lds(rerank_kernel<0>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((rerank_kernel<0>), dim3(p.nq), dim3(64), lds, s, p);
    }
    return hipGetLastError();
}

size_t rerank_topk_lds(uint32_t dstride, uint32_t cand_stride) {
    return (size_t)dstride * 4 + (size_t)rerank_topk_key_slots(cand_stride) * 8 + (size_t)cand_stride * 4;
}

template <typename K>
static hipError_t launch_topk(K kernel, const RerankTopkParams& p, size_t lds, hipStream_t s) {
    const hipError_t e = set_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(p.nq), dim3(64), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_rerank_topk(const RerankTopkParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (p.k == 0 || p.k > p.cand_stride) return hipErrorInvalidValue;
    const size_t lds = rerank_topk_lds(p.dstride, p.cand_stride);
    const bool pairs = rerank_plan(metric, p.dim, false).form == RerankForm::Pairs;  // as launch_rerank
    if (metric == 1) return pairs ? launch_topk(rerank_topk_pair_kernel<1>, p, lds, s) : launch_topk(rerank_topk_kernel<1>, p, lds, s);
    return pairs ? launch_topk(rerank_topk_pair_kernel<0>, p, lds, s) : launch_topk(rerank_topk_kernel<0>, p, lds, s);
}

}  // namespace gbnns
