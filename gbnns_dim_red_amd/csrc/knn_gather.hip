// knn_gather.hip -- the gathered exact scan of gbnns_index_exact_knn_gather for gfx950 (MI355X): exact tagged kNN that computes distances to
// the rows a query's tag word allows and to no others.
//
// gbnns_index_exact_knn sweeps all n rows for every query and tests the tag per pair, so its cost does not shrink with the filter.  Real
// batches carry a handful of distinct words (the census, tag_census.hip, rests on the same fact), so here the allowed row ids of each
// DISTINCT word are written out once and the queries that share the word scan that list: sum over queries of allowed[i] x d work, in the
// reference's own arithmetic -- no bf16 filter, no rescoring, no packed copy of the table, no float copy of a byte table.
//   gather_schedule     host, pure: queries grouped by word, groups dealt into rounds whose lists fit a budget, a group's queries cut into
//                       workgroups of W (gbnns_debug_gather_schedule exposes it)
//   gather_fill_kernel  the census kernel's shape -- a tile of 1 024 tag words in registers, the round's words looped over it --: per word and
//                       wavefront the ballots of the tile's four registers, one vector atomicAdd on the word's cursor, every lane with an
//                       allowed row stores its id at its prefix position.  The order inside a list is whatever the atomics give; selection
//                       is by (distance key << 32 | id), so it does not matter.  A store beyond the census count is dropped.
//   knn_gather_kernel   knn_scan_kernel's loop (knn.hip) with two indirections: the tile's rows come through the group's id list, a thread's
//                       queries through the schedule's permutation.  Per distance the operations and their order are knn_scan_kernel's -- the
//                       loop body is the same text (knn_scan_row.inc).  No tag test in the loop: every listed row is allowed.  Byte rows are
//                       widened to float while they are staged, byte queries into registers: every partial sum is then an integer below
//                       2^24 (d <= 128 here), so the float arithmetic is exact and equals the int8 matrix cores' distance of knn_bytes.hip.
// Heaps [k][heap_stride] by original query index as the scan's; knn_finalize_kernel (knn.hip) sorts them and writes the outputs.  Every global
// write is an ordinary vector store or a vector atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>

#include "kernels.h"
#include "knn_select.h"
#include "knn_scan_dist.h"

namespace gbnns {

namespace {

constexpr uint32_t kFillThreads = 256;             // four wavefronts
constexpr uint32_t kFillTile = kFillThreads * 4;   // 1 024 rows a workgroup, one 16-byte load a lane (the census kernel's measured optimum)

// Lane l of wavefront v holds in register e the tag word of row tile0 + v * 256 + l * 4 + e.  Rows behind n read as 0, which no word allows.
__global__ __launch_bounds__(kFillThreads) void gather_fill_kernel(GatherFillParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t j0 = (uint64_t)blockIdx.x * kFillTile + (uint64_t)threadIdx.x * 4;
    uint32_t v[4];
    if (j0 + 4 <= p.n) {
        const uint4 t = *reinterpret_cast<const uint4*>(p.tags + j0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) v[e] = j0 + e < p.n ? p.tags[j0 + e] : 0u;
    }
    for (uint32_t u0 = 0; u0 < p.groups; u0 += 64) {
        const uint32_t m = min(64u, p.groups - u0);
        // the chunk's words, one per lane: a word then comes out of a register by its lane number, not out of memory
        const uint32_t wv = lane < m ? p.words[u0 + lane] : 0u;
        for (uint32_t l = 0; l < m; ++l) {  // (l, and with it the word, is the same in every lane of the workgroup)
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)wv, (int)l);
            uint32_t before[4], total = 0;  // allowed rows in the lanes below this one, per register; the wavefront's count
            bool hit[4];
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {
                hit[e] = (v[e] & w) != 0u;
                const unsigned long long b = __ballot(hit[e]);
                before[e] = total + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                total += (uint32_t)__popcll(b);
            }
            if (total == 0) continue;  // (uniform over the wavefront)
            const uint32_t u = u0 + l;
            uint32_t pos0 = 0;
            if (lane == 0) pos0 = atomicAdd(&p.cursor[u], total);
            pos0 = (uint32_t)__shfl((int)pos0, 0);
            const uint32_t cap = p.caps[u];
            uint32_t* const dst = p.list + p.offs[u];
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {
                const uint32_t pos = pos0 + before[e];
                if (hit[e] && pos < cap) dst[pos] = (uint32_t)(j0 + e);  // (beyond the census count: dropped, never written)
            }
        }
    }
}

// S = 16-byte steps of a query held in registers (d <= 4 * S), QPT = queries per thread, U8 = byte rows and byte queries.  A workgroup serves
// up to W = QPT x 128 queries of ONE group: thread t owns the queries at places t and (QPT = 2) 128 + t of the workgroup's slice of `order`.
template <int METRIC, int S, int QPT, bool U8>
__global__ __launch_bounds__(kKnnThreads) void knn_gather_kernel(KnnGatherParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* tile = reinterpret_cast<float4*>(smem);                        // [kKnnTile][S]
    uint32_t* tile_id = reinterpret_cast<uint32_t*>(tile + kKnnTile * S);  // [kKnnTile] the tile's row ids
    const int t = threadIdx.x;
    const GatherWorkgroup wg = p.wgs[blockIdx.x];
    const uint32_t* const list = p.list + (((uint64_t)wg.list_off_hi << 32) | wg.list_off_lo);
    const uint32_t len = wg.list_len;
    // L2Metric::Dist uses the first 4 * floor(d / 4) dims only; the dot form is offered for d % 8 == 0
    const uint32_t steps = p.dim >> 2;
    const bool vec_ok = (p.bstride & 3u) == 0;   // rows 16-B aligned -> float4 loads
    const bool qvec_ok = (p.qstride & 3u) == 0;

    float4 q[QPT][S];
    uint32_t qi[QPT];
    bool live[QPT];
    uint64_t root[QPT];
#pragma unroll
    for (int a = 0; a < QPT; ++a) {
        const uint32_t place = (uint32_t)a * kKnnThreads + (uint32_t)t;
        live[a] = place < wg.q_count;
        qi[a] = live[a] ? p.order[wg.q_begin + place] : 0u;
        root[a] = live[a] ? p.heap[qi[a]] : ~0ull;  // (all-ones in a fresh heap)
#pragma unroll
        for (int c = 0; c < S; ++c) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((uint32_t)c < steps) {
                if constexpr (U8) {
                    const uint8_t* qp = p.q_b + (size_t)qi[a] * p.qstride + 4 * c;  // (rows of d bytes: no alignment to rely on)
                    v = make_float4((float)qp[0], (float)qp[1], (float)qp[2], (float)qp[3]);
                } else {
                    const float* qp = p.q + (size_t)qi[a] * p.qstride;
                    if (qvec_ok) v = reinterpret_cast<const float4*>(qp)[c];
                    else v = make_float4(qp[4 * c], qp[4 * c + 1], qp[4 * c + 2], qp[4 * c + 3]);
                }
            }
            q[a][c] = v;
        }
    }

    for (uint32_t base0 = 0; base0 < len; base0 += kKnnTile) {
        __syncthreads();  // everyone is done with the previous tile
        if (t < kKnnTile) tile_id[t] = base0 + t < len ? list[base0 + t] : 0u;
        __syncthreads();
        for (int e = t; e < kKnnTile * S; e += kKnnThreads) {
            const int r = e / S, c = e % S;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (base0 + r < len && (uint32_t)c < steps) {
                const uint32_t row = tile_id[r];
                if constexpr (U8) {
                    // (a byte row is 16-byte aligned and zero padded to bstride, a multiple of 16: step c is one aligned word)
                    const uint32_t w4 = *reinterpret_cast<const uint32_t*>(p.base_b + (size_t)row * p.bstride + 4 * c);
                    v = make_float4((float)(w4 & 255u), (float)((w4 >> 8) & 255u), (float)((w4 >> 16) & 255u), (float)(w4 >> 24));
                } else {
                    const float* bp = p.base + (size_t)row * p.bstride;
                    if (vec_ok) v = reinterpret_cast<const float4*>(bp)[c];
                    else v = make_float4(bp[4 * c], bp[4 * c + 1], bp[4 * c + 2], bp[4 * c + 3]);
                }
            }
            tile[e] = v;
        }
        __syncthreads();
        const int rows = (len - base0 < (uint32_t)kKnnTile) ? (int)(len - base0) : kKnnTile;  // (a list's tail offers only the rows it has)
        for (int r = 0; r < rows; ++r) {
            float dist[QPT];
            const float4* trow = tile + r * S;
#include "knn_scan_row.inc"  // dist[] = the row's distances to q[]: knn_scan_kernel's operations in its order
            const uint64_t row = tile_id[r];
#pragma unroll
            for (int a = 0; a < QPT; ++a) {
                const uint64_t key = ((uint64_t)knn_fkey(dist[a]) << 32) | (uint32_t)row;
                const bool self = p.self_offset >= 0 && row == (uint64_t)qi[a] + (uint64_t)p.self_offset;
                if (live[a] && !self && key < root[a])
                    root[a] = heap_replace_root(p.heap + qi[a], p.heap_stride, p.k, key);
            }
        }
    }
}

template <int METRIC, int S, int QPT, bool U8>
hipError_t launch_gather_t(const KnnGatherParams& p, hipStream_t s) {
    const size_t lds = (size_t)kKnnTile * S * 16 + kKnnTile * 4;
    hipLaunchKernelGGL((knn_gather_kernel<METRIC, S, QPT, U8>), dim3(p.n_wgs), dim3(kKnnThreads), lds, s, p);
    return hipGetLastError();
}

// The gather instance of a shape: launch, name and W from one place (launch_knn_gather starts what gbnns_debug_gather_plan names).  The
// shapes are knn_scan_pick's narrow ones.
struct KnnGatherPick {
    hipError_t (*launch)(const KnnGatherParams&, hipStream_t);
    const char* name;
    uint32_t W;
};
#define KNN_GATHER(M, S, QPT, U8) \
    KnnGatherPick{&launch_gather_t<M, S, QPT, U8>, "knn_gather_kernel<" #M ", " #S ", " #QPT ", " #U8 ">", (uint32_t)(QPT * kKnnThreads)}
#define KNN_GATHER_BY(S, QPT)                                                      \
    (metric == 1 ? (bytes ? KNN_GATHER(1, S, QPT, true) : KNN_GATHER(1, S, QPT, false)) \
                 : (bytes ? KNN_GATHER(0, S, QPT, true) : KNN_GATHER(0, S, QPT, false)))
KnnGatherPick knn_gather_pick(int metric, uint32_t dim, bool bytes) {
    if (dim <= 32) return KNN_GATHER_BY(8, 2);
    if (dim <= 64) return KNN_GATHER_BY(16, 2);
    if (dim <= 128) return KNN_GATHER_BY(32, 1);
    return KnnGatherPick{nullptr, nullptr, 0};  // wider rows: the caller runs the existing scan
}
#undef KNN_GATHER_BY
#undef KNN_GATHER

}  // namespace

void gather_schedule(const uint32_t* words, const uint32_t* allowed, uint64_t nq, uint64_t n, uint64_t budget, uint32_t W, GatherSchedule& out) {
    (void)n;
    if (W == 0) W = 1;
    out = GatherSchedule{};
    out.order.resize(nq);
    std::iota(out.order.begin(), out.order.end(), 0u);
    // queries that may see something first, by (word, index); the rest behind them, by index
    std::stable_sort(out.order.begin(), out.order.end(), [&](uint32_t a, uint32_t b) {
        const bool ea = allowed[a] == 0, eb = allowed[b] == 0;
        if (ea != eb) return eb;
        return !ea && words[a] < words[b];
    });
    uint64_t in_round = 0;
    uint32_t round = 0;
    out.round_group0.push_back(0);
    out.round_wg0.push_back(0);
    for (uint64_t b = 0; b < nq && allowed[out.order[b]] != 0;) {
        uint64_t e = b + 1;
        while (e < nq && allowed[out.order[e]] != 0 && words[out.order[e]] == words[out.order[b]]) ++e;
        const uint32_t len = allowed[out.order[b]];
        if (in_round != 0 && in_round + len > budget) {  // (a group longer than the budget: a round of its own)
            out.round_entries.push_back(in_round);
            out.round_group0.push_back((uint32_t)out.groups.size());
            out.round_wg0.push_back((uint32_t)out.wgs.size());
            in_round = 0;
            ++round;
        }
        out.groups.push_back(GatherGroup{words[out.order[b]], len, (uint32_t)b, (uint32_t)(e - b), round, in_round});
        for (uint64_t q0 = b; q0 < e; q0 += W)
            out.wgs.push_back(GatherWorkgroup{(uint32_t)in_round, (uint32_t)(in_round >> 32), len, (uint32_t)q0, (uint32_t)std::min<uint64_t>(W, e - q0), 0u});
        in_round += len;
        b = e;
    }
    if (!out.groups.empty()) {
        out.round_entries.push_back(in_round);
        out.round_group0.push_back((uint32_t)out.groups.size());
        out.round_wg0.push_back((uint32_t)out.wgs.size());
    }
}

hipError_t launch_gather_fill(const GatherFillParams& p, hipStream_t s) {
    if (p.groups == 0 || p.n == 0) return hipSuccess;
    if (!p.tags || !p.words || !p.caps || !p.offs || !p.cursor || !p.list || p.n >= 0xFFFFFFFFull || (reinterpret_cast<uintptr_t>(p.tags) & 15u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_fill_kernel, dim3((unsigned)((p.n + kFillTile - 1) / kFillTile)), dim3(kFillThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_knn_gather(const KnnGatherParams& p, int metric, hipStream_t s) {
    if (p.n_wgs == 0) return hipSuccess;
    const bool bytes = p.base_b != nullptr;
    if (bytes ? (!p.q_b || (p.bstride & 15u) || (reinterpret_cast<uintptr_t>(p.base_b) & 15u)) : (!p.base || !p.q)) return hipErrorInvalidValue;
    const KnnGatherPick k = knn_gather_pick(metric, p.dim, bytes);
    return k.launch ? k.launch(p, s) : hipErrorInvalidValue;
}

const char* knn_gather_kernel_name(int metric, uint32_t dim, bool bytes, uint32_t* W) {
    const KnnGatherPick k = knn_gather_pick(metric, dim, bytes);
    if (W) *W = k.W;
    return k.name;
}

}  // namespace gbnns
