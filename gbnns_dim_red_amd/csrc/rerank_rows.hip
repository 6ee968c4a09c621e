// rerank_rows.hip -- the stand-alone re-rank kernels of the narrow row kinds (row_kind.h): a byte handle's uint8 rows (gbnns_index_create_bytes)
// and a half-base handle's IEEE binary16 rows (gbnns_index_create_half_base) -- rerank.hip's four kernels over such rows.  An element is
// widened by one conversion (v_cvt_f32_ubyte0..3; v_cvt_f32_f16 -- no flush flag on this unit: binary16 subnormals are kept) and is exact in
// binary32, so every distance is the float kernels' distance on float32(table), bit for bit: the same operations in the same order, multiply
// and add separate (walk_common.h: l2_ordered / negdot_ordered through the kind's Row4 adapter, rerank_chunk_core for the chunk-pair form;
// NarrowRow<K> says what differs between the kinds).  The query is staged as floats in LDS and never rounded, the k-answer selection is
// rerank_topk.h's.
#include "launch_util.h"
#include "rerank_topk.h"

namespace gbnns {

namespace {

// (RerankRowsParams: dstride = elements of a row = floats of the staged query, a multiple of row_pad_elems(K); k == 0 in the one-answer launches)
__device__ __forceinline__ void keep(const TopkLds& t, int r, float dv) {
    t.keys[r] = ((uint64_t)fkey(dv) << 32) | (uint32_t)r;
    t.dist[r] = dv;
}

// a lane per row: the negative dot product (any d: the masked tail meets the row's zero padding), and L2 wherever rerank_plan.h gives no
// chunk-pair form (the d % 4 tail ignored, as in the float kernel)
template <RowKind K, int METRIC, bool TOPK>
__global__ __launch_bounds__(64) void rerank_rows_kernel(RerankRowsParams p) {
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
            const auto row = NarrowRow<K>::row4(static_cast<const typename NarrowRow<K>::Elem*>(p.db_rows) + (size_t)id * p.dstride);
            const float dv = metric_dist<METRIC>(row, qs, p.dim);
            if constexpr (TOPK) {
                keep(t, r, dv);
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

// the chunk-pair form (L2).  DEEP: rerank_plan.h's `deep` of the kind and row length (the launcher picks the instance).
template <RowKind K, bool TOPK, int DEEP>
__global__ __launch_bounds__(64) void rerank_rows_pair_kernel(RerankRowsParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const uint32_t qi = blockIdx.x;
    const int cnt = topk_count(p, qi);
    const uint32_t* cand = p.cand + (size_t)qi * p.cand_stride;
    const RerankRowsSrc a{p.q, p.qstride, p.db_rows, p.dstride, p.dim, p.n};
    auto id_at = [&](int r) { return cand[r]; };
    if constexpr (TOPK) {
        const TopkLds t = topk_lds(smem, p);
        rerank_chunk_core<K, DEEP>(a, qi, cnt, reinterpret_cast<float*>(smem), lane, id_at, [&](int r, float dv) { keep(t, r, dv); });
        topk_select(p, t, cand, qi, cnt, lane);
    } else {
        const int win = rerank_chunk_core<K, DEEP>(a, qi, cnt, reinterpret_cast<float*>(smem), lane, id_at);
        if (lane == 0) p.out[qi] = (win >= 0) ? cand[win] : kInvalidId;
    }
}

bool shape_ok(RowKind k, const RerankRowsParams& p) {
    return k != RowKind::F32 && p.db_rows && (reinterpret_cast<uintptr_t>(p.db_rows) & 15u) == 0 && p.dim > 0 && p.dstride % row_pad_elems(k) == 0 &&
           p.dstride >= p.dim;
}

template <RowKind K, bool TOPK>
hipError_t launch_form(const RerankRowsParams& p, int metric, size_t lds, hipStream_t s) {
    if (metric == 1) return launch_per_query(rerank_rows_kernel<K, 1, TOPK>, p, lds, s);  // (never the chunk-pair form: rerank_plan.h)
    const RerankPlan plan = rerank_plan(metric, p.dim, K);
    if (plan.form != RerankForm::ChunkPairs) return launch_per_query(rerank_rows_kernel<K, 0, TOPK>, p, lds, s);
    if constexpr (K == RowKind::F16)
        if (plan.deep > 4) return launch_per_query(rerank_rows_pair_kernel<K, TOPK, GBNNS_HALF_RERANK_DEEP>, p, lds, s);
    return launch_per_query(rerank_rows_pair_kernel<K, TOPK, 4>, p, lds, s);
}

template <bool TOPK>
hipError_t launch_kind(RowKind k, const RerankRowsParams& p, int metric, size_t lds, hipStream_t s) {
    return k == RowKind::U8 ? launch_form<RowKind::U8, TOPK>(p, metric, lds, s) : launch_form<RowKind::F16, TOPK>(p, metric, lds, s);
}

}  // namespace

hipError_t launch_rerank_rows(RowKind rows, const RerankRowsParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (!shape_ok(rows, p)) return hipErrorInvalidValue;
    return launch_kind<false>(rows, p, metric, (size_t)p.dstride * 4, s);
}

hipError_t launch_rerank_topk_rows(RowKind rows, const RerankRowsParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    if (!shape_ok(rows, p) || p.k == 0 || p.k > p.cand_stride) return hipErrorInvalidValue;
    return launch_kind<true>(rows, p, metric, rerank_topk_lds(p.dstride, p.cand_stride), s);
}

}  // namespace gbnns
