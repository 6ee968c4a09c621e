// walk_general.hip -- the end of the hand-over chain: walk_general_kernel, exact for every input (any ef, any number of ties,
// any visited count, several entry points; everything in global memory), and the tests' merge probe.
#include <algorithm>

#include "launch_util.h"
#include "row_kind.h"
#include "walk_lists.h"

namespace gbnns {

namespace {

// ---- general kernel: exact for every input (any ef, any number of ties, any visited count) ----
//
// Persistent wavefronts pull query indices from the hand-over list.  Visited set = one bit per
// node in a per-slot global bitmap (cleared per query); result list and tie list in global
// memory (tie capacity n: every node can be in it at most once).

// TAG (gbnns_search_tagged): p.tags / p.qtags are set -- a neighbour j with (tags[j] & qtags[qi]) == 0 is an empty slot of its adjacency row
// (main and auxiliary alike; the row still ends at its first chunk without a live slot), and an entry row the query may not see is a bad
// entry.  A kernel of its own (walk_general_tag_kernel): walk_general_kernel keeps its instructions (the shared body moved the operand order
// of 18 commutative instructions and the registers they name, nothing else).
// TAG == 2 (GBNNS_FLAG_TAG_BRIDGE, walk_general_bridge_kernel): a disallowed neighbour is looked through -- the allowed entries of its own row
// (main graph through the main graph, auxiliary through the auxiliary) take its place, one level deep.  The ids of that row G'' are compacted
// in order into `bst` (64 words of LDS) and run through the expansion a chunk at a time; of equal ids inside a chunk only the first stays
// (two lanes that claim one id at once would both be told it is new, or the later one alone).
// RR == U8 (walk_general_bytes_kernel: the hand-overs of a byte handle's fused first pass, gbnns_index_create_bytes): the same walk, the fused
// re-rank over uint8 rows (WalkParams::rr_db_b).
// WALKED == U8 (GBNNS_FLAG_BYTE_WALK: walk_general_bwalk_kernel<METRIC, TAG>): the WALKED rows are uint8 (WalkParams::db_b, p.dstride bytes a
// row = the floats of the staged query) -- the three distances read the row through ByteRow4, a lane per row: l2_ordered / negdot_ordered on
// float32(row), any dimension, both metrics.  Exact, not tuned.  It takes every flagged call outside the domain of walk_bytes.hip's instances
// and every query those hand over.
// WALKED == F16 (GBNNS_FLAG_HALF_WALK: walk_general_hwalk_kernel<METRIC, TAG>): the WALKED rows are a half-base handle's binary16 rows (WalkParams::db_h,
// p.dstride halves a row = the floats of the staged query) -- the three distances read the row through HalfRow4, a lane per row: l2_ordered /
// negdot_ordered on float32(row), any dimension, both metrics (L2 never reads a coordinate beyond 4 * floor(d / 4): such a tail may hold any
// bit pattern; the negative dot reads all d and the row's zero padding against the staged zeros).  Exact, not tuned.  It takes every flagged
// call outside the domain of walk_half_base.hip's instances and every query those hand over.
// The distance of row `id` of the walked table from the staged query, by the table's kind: float4 rows, ByteRow4, HalfRow4 (a lane per row).
template <int METRIC, RowKind WALKED>
__device__ __forceinline__ float walked_row_dist(const WalkParams& p, const float4* qs, uint32_t id) {
    if constexpr (WALKED == RowKind::F16) return metric_dist<METRIC>(qs, HalfRow4{reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p.db_h) + (size_t)id * p.dstride)}, p.dim);
    else if constexpr (WALKED == RowKind::U8) return metric_dist<METRIC>(qs, ByteRow4{reinterpret_cast<const uint32_t*>(p.db_b + (size_t)id * p.dstride)}, p.dim);
    else return metric_dist<METRIC>(qs, reinterpret_cast<const float4*>(p.db + (size_t)id * p.dstride), p.dim);
}

template <int METRIC, int TAG, RowKind WALKED = RowKind::F32, RowKind RR = RowKind::F32>
__device__ __forceinline__ void walk_general_body(WalkParams p, unsigned char* smem, uint32_t* bst = nullptr) {
    const int lane = lane_id();
    const uint32_t slot = blockIdx.x;
    float* qf = reinterpret_cast<float*>(smem);
    const float4* qs = reinterpret_cast<const float4*>(qf);
    uint32_t* bitmap = p.g_bitmap + (size_t)slot * 2u * p.bitmap_words;  // [visited bits][tie bits]
    const uint32_t n_ent = p.n_entries ? p.n_entries : 1u;
    uint64_t* keys = p.g_keys + (size_t)slot * ((size_t)p.ef + n_ent - 1u);  // one extra slot per extra entry point
    // tie set: one bit per node (second half of the slot's bitmap block); the host zeroes it when it allocates the
    // block, clear() leaves it all zero after every use
    TieBits tie{bitmap + p.bitmap_words, 0xFFFFFFFFu, 0u};
    const int ef = p.ef;
    const uint32_t total = p.all_general ? p.nq : *p.ovf2_count;
    if (slot == 0 && lane == 0 && total) atomicAdd(p.g_total, total);
    if (slot == 0 && lane < 7 && lane != 5 && p.next_ctrl) p.next_ctrl[lane] = 0u;  // control words of the next call (word 5 of block 0 is the persistent general-kernel total)

    while (true) {
        uint32_t w = 0;
        if (lane == 0) w = atomicAdd(p.g_cursor, 1u);
        w = (uint32_t)__shfl((int)w, 0);
        if (w >= total) break;
        const uint32_t qi = p.all_general ? w : p.ovf2_list[w];

        for (uint32_t i = lane; i < p.dstride; i += 64)
            qf[i] = (i < p.dim) ? p.q[(size_t)qi * p.qstride + i] : 0.f;
        wave_sync();

        uint32_t qtag = 0u;
        if constexpr (TAG != 0) qtag = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.qtags[qi]);
        {
            bool bad = false;  // an entry id outside the index: empty result, no row is touched
            for (uint32_t e = 0; e < n_ent; ++e) bad |= (p.entries ? p.entries[(size_t)qi * n_ent + e] : 0u) >= p.n;
            if constexpr (TAG != 0) {  // ... or an entry row the query may not see
                for (uint32_t e = 0; e < n_ent && !bad; ++e) bad |= (p.tags[p.entries ? p.entries[(size_t)qi * n_ent + e] : 0u] & qtag) == 0u;
            }
            if (bad) {
                if constexpr (RR == RowKind::U8) write_bad_entry_bytes(p, qi, lane);
                else write_bad_entry(p, qi, lane);
                wave_sync();
                continue;
            }
        }
        WalkState st;
        st.size = 0; st.tsize = 0; st.first_un = 0; st.hops = 0; st.dist_calc = 1; st.edges = 0;
        // search_function.h:54-64: one walk per entry point -- fresh candidate set (every result so far counts as
        // expanded, the tie list is dropped) and fresh visited set; the result heap, hops and dist_calc carry
        // over; the entry's own distance is not counted and it is pushed without the size test (so the heap
        // stays one longer per extra entry point: makeStep pops once per push, :36-37)
        for (uint32_t e = 0; e < n_ent; ++e) {
        for (uint32_t i = lane; i < p.bitmap_words; i += 64) bitmap[i] = 0u;
        if (e > 0) {
            for (int i = lane; i < st.size; i += 64) keys[i] = keys[i] | 1ull;
            tie.clear(st.tsize, lane);
        }
        wave_sync();
        const uint32_t entry = p.entries ? p.entries[(size_t)qi * n_ent + e] : 0u;
        {
            const float d0 = walked_row_dist<METRIC, WALKED>(p, qs, entry);
            if (e == 0) {
                if (lane == 0) keys[0] = make_key(fkey(d0), entry);
                st.size = 1;
            } else {
                uint64_t ev;
                bool did;
                const int pos = list_insert(keys, st.size, 0x7FFFFFFF, make_key(fkey(d0), entry), ev, did, lane);
                st.first_un = pos;
            }
            if (lane == 0) bitmap[entry >> 5] = 1u << (entry & 31u);
            wave_sync();
        }
        uint32_t node;
        auto make_step = [&](const uint32_t* row, uint32_t stride, bool& found) {  // search_function.h:15-40
            for (uint32_t c = 0; c < stride; c += 64) {
                const uint32_t nb = (c + lane < stride) ? row[c + lane] : kInvalidId;
                bool valid = nb != kInvalidId;
                uint64_t mv = __ballot(valid);
                if (!mv) break;
                if constexpr (TAG == 1) {  // a disallowed neighbour is an empty slot from here on (a chunk of them is not the end of the row)
                    valid = valid && (p.tags[nb] & qtag) != 0u;
                    mv = __ballot(valid);
                    if (!mv) continue;
                }
                st.edges += __popcll(mv);
                bool fresh = false;
                if (valid) {
                    const uint32_t bit = 1u << (nb & 31u);
                    fresh = !(atomicOr(&bitmap[nb >> 5], bit) & bit);
                }
                uint32_t dk = 0xFFFFFFFFu;
                if (fresh) dk = fkey(walked_row_dist<METRIC, WALKED>(p, qs, nb));
                const uint64_t mf = __ballot(fresh);
                st.dist_calc += __popcll(mf);
                const uint32_t worst0 = key_hi(keys[st.size - 1]);
                uint64_t m = __ballot(fresh && (st.size < ef || dk < worst0));
                if (m) found = true;
                while (m) {
                    const int l = __ffsll((unsigned long long)m) - 1;
                    m &= m - 1;
                    const uint32_t dl = (uint32_t)__shfl((int)dk, l);
                    const uint32_t il = (uint32_t)__shfl((int)nb, l);
                    offer(keys, tie, st, ef, dl, il, lane);
                }
            }
        };
        // TAG == 2: one chunk of a row of G'' -- every id allowed, in order; what make_step does with a chunk, behind the first-occurrence filter
        // (the tail from `fresh` on is make_step's, line for line, and stays written out twice: shared through one lambda, every instance of this
        // body compiles to the same instructions in another order -- and the kernels' instructions are pinned)
        auto offer_chunk = [&](uint32_t nb, bool valid, bool& found) {
            uint64_t mv = __ballot(valid);
            st.edges += __popcll(mv);  // (the degree in G'' counts repeated ids)
            uint64_t dup = 0ull;
            for (uint64_t rem = mv; rem;) {
                const int j = __ffsll((unsigned long long)rem) - 1;
                const uint64_t eq = __ballot(valid && nb == (uint32_t)__shfl((int)nb, j));
                dup |= eq & ~(1ull << j);
                rem &= ~eq;
            }
            valid = valid && !((dup >> lane) & 1ull);
            bool fresh = false;
            if (valid) {
                const uint32_t bit = 1u << (nb & 31u);
                fresh = !(atomicOr(&bitmap[nb >> 5], bit) & bit);
            }
            uint32_t dk = 0xFFFFFFFFu;
            if (fresh) dk = fkey(walked_row_dist<METRIC, WALKED>(p, qs, nb));
            const uint64_t mf = __ballot(fresh);
            st.dist_calc += __popcll(mf);
            const uint32_t worst0 = key_hi(keys[st.size - 1]);
            uint64_t m = __ballot(fresh && (st.size < ef || dk < worst0));
            if (m) found = true;
            while (m) {
                const int l = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const uint32_t dl = (uint32_t)__shfl((int)dk, l);
                const uint32_t il = (uint32_t)__shfl((int)nb, l);
                offer(keys, tie, st, ef, dl, il, lane);
            }
        };
        auto bridged_step = [&](const uint32_t* ell, uint32_t stride, bool& found) {
            int cnt = 0;  // ids staged in bst
            auto flush = [&]() {
                wave_sync();
                const uint32_t id = lane < cnt ? bst[lane] : kInvalidId;
                offer_chunk(id, lane < cnt, found);
                wave_sync();
                cnt = 0;
            };
            auto emit = [&](uint32_t id, bool pred) {  // appends the ids of the lanes with `pred`, in lane order
                const uint64_t m = __ballot(pred);
                if (!m) return;
                const int idx = cnt + __popcll(m & ((1ull << lane) - 1ull));
                const int tot = cnt + __popcll(m);
                if (pred && idx < 64) bst[idx] = id;
                if (tot >= 64) {
                    cnt = 64;
                    flush();
                    if (pred && idx >= 64) bst[idx - 64] = id;
                    cnt = tot - 64;
                } else cnt = tot;
            };
            const uint32_t* row = ell + (size_t)node * stride;
            for (uint32_t c = 0; c < stride; c += 64) {
                const uint32_t nb = (c + lane < stride) ? row[c + lane] : kInvalidId;
                const bool live = nb != kInvalidId;
                const uint64_t mlive = __ballot(live);
                if (!mlive) break;  // (the end of a row: decided before the tag test, for u's row and for a looked-through one)
                const bool allowed = live && (p.tags[nb] & qtag) != 0u;
                uint64_t md = mlive & ~__ballot(allowed);
                int pos = 0;  // slots below it are emitted
                while (md) {
                    const int d = __ffsll((unsigned long long)md) - 1;
                    md &= md - 1;
                    emit(nb, allowed && lane >= pos && lane < d);
                    const uint32_t* vrow = ell + (size_t)(uint32_t)__shfl((int)nb, d) * stride;
                    for (uint32_t c2 = 0; c2 < stride; c2 += 64) {
                        const uint32_t nb2 = (c2 + lane < stride) ? vrow[c2 + lane] : kInvalidId;
                        const bool live2 = nb2 != kInvalidId;
                        if (!__ballot(live2)) break;
                        emit(nb2, live2 && (p.tags[nb2] & qtag) != 0u);
                    }
                    pos = d + 1;
                }
                emit(nb, allowed && lane >= pos);
            }
            if (cnt) flush();
        };
        while (select_candidate(keys, tie, st, node, lane)) {
            bool found = false;
            if constexpr (TAG == 2) {
                if (p.aux_ell && (uint32_t)st.hops < p.hops_bound) bridged_step(p.aux_ell, p.aux_stride, found);
                if (!(found && p.llf)) bridged_step(p.ell, p.ell_stride, found);
            } else {
            if (p.aux_ell && (uint32_t)st.hops < p.hops_bound)  // :73-80
                make_step(p.aux_ell + (size_t)node * p.aux_stride, p.aux_stride, found);
            if (!(found && p.llf))                                // :82-89
                make_step(p.ell + (size_t)node * p.ell_stride, p.ell_stride, found);
            }
            st.hops += 1;
        }
        }  // entry points
        tie.clear(st.tsize, lane);  // leaves the tie bits all zero for the next query
        write_results(p, qi, keys, st, lane);
        if constexpr (RR == RowKind::U8) {
            if (p.rr_db_b) {
                const int kept = st.size < p.k ? st.size : p.k;
                fused_rerank<8, true>(p, qi, kept, smem, lane, [&](int rank) { return key_id(keys[rank]); });
            }
        } else if (p.rr_db) {
            const int kept = st.size < p.k ? st.size : p.k;
            fused_rerank(p, qi, kept, smem, lane, [&](int rank) { return key_id(keys[rank]); });
        }
        wave_sync();
    }
}

template <int METRIC>
__global__ __launch_bounds__(64) void walk_general_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_general_body<METRIC, 0>(p, smem);
}

template <int METRIC>
__global__ __launch_bounds__(64) void walk_general_tag_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_general_body<METRIC, 1>(p, smem);
}

__global__ __launch_bounds__(64) void walk_general_bytes_kernel(WalkParams p) {  // (the byte instances are L2 ones)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_general_body<0, 0, RowKind::F32, RowKind::U8>(p, smem);
}

template <int METRIC>
__global__ __launch_bounds__(64) void walk_general_bridge_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t bst[64];
    walk_general_body<METRIC, 2>(p, smem, bst);
}

// GBNNS_FLAG_BYTE_WALK: plain, cut (gbnns_search_tagged) and bridged (GBNNS_FLAG_TAG_BRIDGE) over uint8 walked rows
template <int METRIC, int TAG>
__global__ __launch_bounds__(64) void walk_general_bwalk_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t bst[TAG == 2 ? 64 : 1];
    walk_general_body<METRIC, TAG, RowKind::U8>(p, smem, TAG == 2 ? bst : nullptr);
}

// GBNNS_FLAG_HALF_WALK: plain, cut and bridged over binary16 walked rows
template <int METRIC, int TAG>
__global__ __launch_bounds__(64) void walk_general_hwalk_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t bst[TAG == 2 ? 64 : 1];
    walk_general_body<METRIC, TAG, RowKind::F16>(p, smem, TAG == 2 ? bst : nullptr);
}

template <typename K>
hipError_t launch_general(K kernel, const WalkParams& p, size_t lds, hipStream_t s) {
    const hipError_t e = set_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(kGeneralSlots), dim3(64), lds, s, p);
    return hipGetLastError();
}

// Diagnostic kernel (tests only): runs one batch merge on a list / survivor set supplied by the host.
template <int R>
__global__ __launch_bounds__(64) void debug_merge_kernel(const uint64_t* entries, int size, const uint64_t* surv, int ef,
                                                         uint64_t* out, int* out_size) {
    __shared__ uint64_t stage[64 * R + 2];
    const int lane = lane_id();
    RegList<R> L;
    L.clear();
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r * 64 + lane < size) {
            L.lo[r] = (uint32_t)entries[r * 64 + lane];
            L.hi[r] = (uint32_t)(entries[r * 64 + lane] >> 32);
        }
    const uint64_t sk = surv[lane];
    const bool is_surv = sk != ~0ull;
    const uint64_t m = __ballot(is_surv);
    uint32_t worst = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t t = readlane_u32(L.hi[r], (size - 1) & 63);
        if (((size - 1) >> 6) == r) worst = t;
    }
    int tsize = 0;
    bool ok;
    if constexpr (R == 1) ok = reg_merge(m, is_surv, (uint32_t)(sk >> 32), (uint32_t)sk >> 1, L, size, worst, tsize, stage, ef, lane);
    else ok = reg_merge_multi<R>(m, is_surv, (uint32_t)(sk >> 32), (uint32_t)sk >> 1, L, size, worst, tsize, stage, ef, lane);
#pragma unroll
    for (int r = 0; r < R; ++r) out[r * 64 + lane] = ((uint64_t)L.hi[r] << 32) | L.lo[r];
    if (lane == 0) {
        out_size[0] = size;
        out_size[1] = ok ? 1 : 0;
        out_size[2] = (int)worst;
    }
}

}  // namespace

hipError_t launch_walk_general(const WalkParams& p, int metric, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    const bool rerank = p.rr_db || p.rr_db_b;
    // a PLAIN walk over the handle's own uint8 / binary16 rows (GBNNS_FLAG_BYTE_WALK / GBNNS_FLAG_HALF_WALK): one kind of rows, its table, no re-rank
    if (p.walk_half && (!p.db_h || p.db || p.walk_bytes)) return hipErrorInvalidValue;
    if (p.walk_bytes && !p.db_b) return hipErrorInvalidValue;
    if ((p.walk_half || p.walk_bytes) && rerank) return hipErrorInvalidValue;
    // a byte handle's fused call: untagged, L2 (walk_plan.cpp)
    if (p.rr_db_b && (p.rr_db || p.tagged || metric != 0)) return hipErrorInvalidValue;
    if (p.tagged && (!p.tags || !p.qtags)) return hipErrorInvalidValue;
    const size_t lds = std::max((size_t)p.dstride * 4, rerank ? (size_t)p.rr_dstride * 4 : (size_t)0);
    using Kernel = void (*)(WalkParams);
    // [metric][untagged / cut / bridged] per kind of walked rows
    static const Kernel f32[2][3] = {{walk_general_kernel<0>, walk_general_tag_kernel<0>, walk_general_bridge_kernel<0>},
                                     {walk_general_kernel<1>, walk_general_tag_kernel<1>, walk_general_bridge_kernel<1>}};
    static const Kernel u8[2][3] = {{walk_general_bwalk_kernel<0, 0>, walk_general_bwalk_kernel<0, 1>, walk_general_bwalk_kernel<0, 2>},
                                    {walk_general_bwalk_kernel<1, 0>, walk_general_bwalk_kernel<1, 1>, walk_general_bwalk_kernel<1, 2>}};
    static const Kernel f16[2][3] = {{walk_general_hwalk_kernel<0, 0>, walk_general_hwalk_kernel<0, 1>, walk_general_hwalk_kernel<0, 2>},
                                     {walk_general_hwalk_kernel<1, 0>, walk_general_hwalk_kernel<1, 1>, walk_general_hwalk_kernel<1, 2>}};
    const int m = metric == 1 ? 1 : 0, tag = p.tagged ? (p.bridged ? 2 : 1) : 0;
    if (p.rr_db_b) return launch_general(walk_general_bytes_kernel, p, lds, s);
    return launch_general((p.walk_half ? f16 : (p.walk_bytes ? u8 : f32))[m][tag], p, lds, s);
}

hipError_t launch_debug_merge(int regs, const uint64_t* entries, int size, const uint64_t* surv, int ef, uint64_t* out,
                              int* out_size, hipStream_t s) {
    if (regs == 1) hipLaunchKernelGGL((debug_merge_kernel<1>), dim3(1), dim3(64), 0, s, entries, size, surv, ef, out, out_size);
    else if (regs == 2) hipLaunchKernelGGL((debug_merge_kernel<2>), dim3(1), dim3(64), 0, s, entries, size, surv, ef, out, out_size);
    else hipLaunchKernelGGL((debug_merge_kernel<4>), dim3(1), dim3(64), 0, s, entries, size, surv, ef, out, out_size);
    return hipGetLastError();
}


}  // namespace gbnns
