// rerank_topk.h -- the k-answer selection of the stand-alone re-rank kernels (gbnns_rerank_topk / gbnns_search_topk), shared by the float
// kernels (rerank.hip) and the narrow-row kernels (rerank_rows.hip: uint8 and binary16 rows): the distances differ in where the row comes from, the selection does not.
#pragma once

#include "walk_common.h"

namespace gbnns {

namespace {

// ------------------------------------------------------------------------------------------
// the k best of a candidate list (gbnns_rerank_topk / gbnns_search_topk; no reference function: the natural extension of
// getRealNearest -- ascending (distance, pop index), so that column 0 is getRealNearest's answer)
// ------------------------------------------------------------------------------------------
// LDS behind the staged query: keys[r] = fkey(dist_r) << 32 | r (8 bytes, padded with all-ones to an even number of entries) and
// dist[r], the distance's own bits.  The keys are unique (r is part of them), so a candidate's output column is its RANK, the number of
// keys smaller than its own: lane l owns keys l, l + 64, ...; it sweeps the whole array -- every lane reads the same 16 bytes (two keys)
// in the same step, which the LDS broadcasts -- and counts.  A function of the keys alone, whatever the order they were written in.
// Every output column gets exactly one store: ranks < min(k, count) from their owners, the columns behind them the padding.
struct TopkLds {
    uint64_t* keys;
    float* dist;
};
__device__ __forceinline__ TopkLds topk_lds(unsigned char* smem, const RerankTopkParams& p) {
    unsigned char* at = smem + (size_t)p.dstride * 4;  // (dstride % 4 == 0: 16-byte aligned)
    TopkLds t;
    t.keys = reinterpret_cast<uint64_t*>(at);
    t.dist = reinterpret_cast<float*>(at + (size_t)rerank_topk_key_slots(p.cand_stride) * 8);
    return t;
}

// ranks of the keys lane + 64 (t0 + j), j < OWN, and their stores
template <int OWN>
__device__ __forceinline__ void topk_rank_and_store(const RerankTopkParams& p, const TopkLds& t, const uint32_t* cand, uint32_t qi, int cnt,
                                                    int kk, int t0, int lane) {
    uint64_t my[OWN];
    int rank[OWN];
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const int r = lane + 64 * (t0 + j);
        my[j] = r < cnt ? t.keys[r] : ~0ull;  // (all-ones: not below any key, and never stored)
        rank[j] = 0;
    }
    const uint4* two = reinterpret_cast<const uint4*>(t.keys);
    for (int i = 0; 2 * i < cnt; ++i) {  // (keys[cnt] is all-ones when cnt is odd)
        const uint4 v = two[i];
        const uint64_t k0 = ((uint64_t)v.y << 32) | v.x, k1 = ((uint64_t)v.w << 32) | v.z;
#pragma unroll
        for (int j = 0; j < OWN; ++j) rank[j] += (k0 < my[j] ? 1 : 0) + (k1 < my[j] ? 1 : 0);
    }
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const int r = lane + 64 * (t0 + j);
        if (r < cnt && rank[j] < kk) {
            p.out[(size_t)qi * p.k + rank[j]] = cand[r];  // the id as given (an id >= n was read as row 0, like gbnns_rerank)
            if (p.out_dist) p.out_dist[(size_t)qi * p.k + rank[j]] = t.dist[r];
        }
    }
}

__device__ __forceinline__ void topk_select(const RerankTopkParams& p, const TopkLds& t, const uint32_t* cand, uint32_t qi, int cnt, int lane) {
    if (lane == 0 && (cnt & 1)) t.keys[cnt] = ~0ull;
    wave_sync();  // every key and distance is in LDS
    const int kk = cnt < (int)p.k ? cnt : (int)p.k;
    if (cnt <= 64) {
        topk_rank_and_store<1>(p, t, cand, qi, cnt, kk, 0, lane);
    } else {
        for (int t0 = 0; 64 * t0 < cnt; t0 += 4) topk_rank_and_store<4>(p, t, cand, qi, cnt, kk, t0, lane);
    }
    for (int c = kk + lane; c < (int)p.k; c += 64) {
        p.out[(size_t)qi * p.k + c] = kInvalidId;
        if (p.out_dist) p.out_dist[(size_t)qi * p.k + c] = __builtin_inff();
    }
}

// a count outside [0, cand_stride] (DEVICE buffers are not validated) must not reach past the row or the LDS arrays sized by the stride
__device__ __forceinline__ int topk_count(const RerankTopkParams& p, uint32_t qi) {
    const int c = p.count[qi];
    return c < 0 ? 0 : (c > (int)p.cand_stride ? (int)p.cand_stride : c);
}

}  // namespace

}  // namespace gbnns
