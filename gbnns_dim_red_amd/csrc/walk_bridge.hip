// walk_bridge.hip -- gbnns_search_tagged with GBNNS_FLAG_TAG_BRIDGE: first-pass walks that look THROUGH a disallowed neighbour.  The walk of
// query i is the reference's search on G''(i): the row of node u is u's adjacency row, in order, with an allowed neighbour v standing for
// itself and a disallowed v replaced by the allowed entries of v's own row (one level: a disallowed entry of v's row is dropped).  The row is
// a plain concatenation -- it may hold u and may hold an id twice; the visited test disposes of both.
//
// The kernel is walk_reg_one's walk (walk_generic.h: register lists, pair form, compact index, visited set in LDS, batch merge, hand-over, fused
// re-rank) around a hop of its own.  A bridged row has no useful upper bound (degree x longest row), so a hop never holds it whole:
//   fill   u's row is read 64 slots at a time and its tag words tested.  Runs of allowed slots are compacted, in order, into a staging area of
//          kBridgeStageIds words in LDS (__ballot prefix counts give the positions).  For the disallowed live slots the adjacency rows are
//          requested four at a time -- four independent loads, then the four loads of their entries' tag words, no dependent chain per slot --
//          and their allowed entries compacted behind what is staged.  The end of an adjacency row is decided by the live slots BEFORE the tag
//          test, for u's row and for a looked-through one.
//   flush  whenever the staging area is full, and at the end of the row, the staged ids go through the hop step 32 at a time: row gather, first-
//          occurrence filter, visited claim, distance, ordered merge -- the pass loop of walk_reg_one reading its "row" from LDS.  Every staged id
//          is allowed: the step has no tag test.  The sequential semantics do not depend on where the row is cut.
// First-occurrence filter: the visited-set claims take the ids of a chunk at once and rely on their being distinct (the packed and quotient
// forms hand a slot to each of two lanes that bring the same id: it would be measured and offered twice).  Adjacency rows hold distinct ids,
// a bridged row need not, so a chunk that holds looked-through ids drops every id an earlier lane of the chunk holds too -- what the
// sequential visited test would answer for it.  Chunks of u's own allowed neighbours skip the filter.
// Looking through v is not a hop; v is never claimed, measured or counted.  edges counts the ids of G'' rows, repeated ones included.  There is
// no bridged retry pass: hand-overs go to the general kernel's bridged instance (walk_general.hip), which also takes every batch outside the
// domain of the table below (two-list beams above 128 and 144-float rows included).
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

namespace {

constexpr int kBridgeBatch = 4;  // looked-through rows requested together

template <int METRIC, int STEPS, int R>
__device__ __forceinline__ void walk_bridge_one(const WalkParams& p, uint32_t qi, unsigned char* smem, uint32_t* ovf_count, uint32_t* ovf_list) {
    static_assert(STEPS == 8 || (METRIC == 0 && (STEPS == 12 || STEPS == 16)), "pair-form instances of a compact index");
    constexpr bool kAlt = (STEPS == 8 && METRIC == 1);  // dot metric: even / odd 16-B pieces instead of halves
    constexpr int kQSteps = STEPS / 2;                  // 16-B steps of the row one lane holds
    constexpr uint32_t kRowBytes = (uint32_t)STEPS * 16u;
    constexpr uint64_t kSlotLanes = 0x5555555555555555ull;  // lanes that own a slot of a 32-id chunk
    const int lane = lane_id();
    const uint32_t slot = (uint32_t)lane >> 1, half = (uint32_t)lane & 1u;
    const int ef = p.ef;
    // LDS: [tie list][merge buffer][query][staged ids of the bridged row][visited set]
    uint64_t* tie = reinterpret_cast<uint64_t*>(smem);
    uint64_t* stage = tie + kRegTieCap;
    float* qf = reinterpret_cast<float*>(stage + reg_stage_slots(R));
    uint32_t* bst = reinterpret_cast<uint32_t*>(qf + p.dstride);
    uint32_t* hash = bst + kBridgeStageIds;
    const float4* qs = reinterpret_cast<const float4*>(qf);
    const uint32_t cap = p.hash_cap;
    const uint32_t hash_lds = (uint32_t)(size_t)((__attribute__((address_space(3))) unsigned char*)reinterpret_cast<unsigned char*>(hash));
    const uint32_t vs_shr = p.vs_shr;  // quotient form of the visited set where the host asked for it, else five 24-bit ids per bucket
    const uint32_t nbuckets = vs_shr ? cap / 7u - kStashBuckets : cap / 5u;
    if (vs_shr) quotient_table_init(hash, nbuckets, lane);
    else packed_table_init(hash, nbuckets, 0u, lane);
    for (uint32_t i = lane; i < p.dstride; i += 64) qf[i] = (i < p.dim) ? p.q[(size_t)qi * p.qstride + i] : 0.f;
    wave_sync();
    RowRegs<kQSteps> qreg;
#pragma unroll
    for (int t = 0; t < kQSteps; ++t) qreg.v[t] = kAlt ? qs[2 * t + half] : qs[kQSteps * half + t];

    RegList<R> L;
    L.clear();
    int size = 1, tsize = 0, hops = 0, dist_calc = 1, edges = 0;
    uint32_t worst;
    const uint32_t entry = p.entries ? p.entries[qi] : 0u;
    if (entry >= p.n) { write_bad_entry(p, qi, lane); return; }
    const uint32_t qtag = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.qtags[qi]);
    // the entry enters untested, as in the reference, and must be allowed: every expanded node then is
    if ((tag_word(p.tags, entry) & qtag) == 0u) { write_bad_entry(p, qi, lane); return; }
    {
        const float d0 = walk_dist<METRIC, STEPS>(qs, row_ptr<true>(p.db, entry, p.dstride), p.dim);
        worst = fkey(d0);
        if (lane == 0) {
            L.hi[0] = worst;
            L.lo[0] = entry << 1;
            if (vs_shr) quotient_table_put_first(hash, nbuckets, entry, vs_shr);
            else packed_table_put_first(hash, nbuckets, entry);
        }
        wave_sync();
    }

    int status = 0;  // 0 = walking, 1 = finished, 2 = handed over to the general kernel
    while (true) {
        // ---- next node to expand: closest unexpanded entry, ties -> largest id (walk_reg_one's selection) -------------
        uint64_t mu[R];
        int p1 = -1, p2 = -1;
        uint32_t node = 0;
        bool picked = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            mu[r] = __ballot(!(L.lo[r] & 1u)) & RegList<R>::lane_mask(r, ef);
            uint64_t m = mu[r];
            if (p1 < 0 && m) {
                p1 = r * 64 + __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
            }
            if (p1 >= 0 && p2 < 0 && m) p2 = r * 64 + __ffsll((unsigned long long)m) - 1;
        }
        if (p1 >= 0 && tsize == 0) {  // common case: the two closest unexpanded entries have different distances
            if (p2 < 0 || L.hi_at(p1) != L.hi_at(p2)) {
                picked = true;
                node = L.lo_at(p1) >> 1;
                L.mark_expanded(p1, lane);
            }
        }
        if (!picked) {  // rare: equal-distance run among the unexpanded entries, a non-empty tie list, or the end
            int best = -1;
            uint32_t hi_p = 0;
            if (p1 >= 0) {
                hi_p = L.hi_at(p1);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint64_t ms = __ballot(!(L.lo[r] & 1u) && L.hi[r] == hi_p) & RegList<R>::lane_mask(r, ef);
                    if (ms) best = r * 64 + 63 - __clzll((long long)ms);
                }
            }
            bool from_tie = false;
            if (tsize > 0 && (best < 0 || hi_p == worst)) {  // tie entries all sit at the worst distance: the largest id among them competes
                uint32_t v = (lane < tsize) ? key_id(tie[lane]) + 1u : 0u;
                int w = lane;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const uint32_t ov = (uint32_t)__shfl_xor((int)v, off);
                    const int ow = __shfl_xor(w, off);
                    if (ov > v) { v = ov; w = ow; }
                }
                v = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
                w = __builtin_amdgcn_readfirstlane(w);
                const uint32_t lid = (best >= 0) ? (L.lo_at(best) >> 1) : 0u;
                if (best < 0 || v - 1u > lid) {
                    from_tie = true;
                    node = v - 1u;
                    if (lane == 0) tie[w] = tie[tsize - 1];
                    tsize -= 1;
                    wave_sync();
                }
            }
            if (!from_tie) {
                if (best < 0) { status = 1; break; }
                node = L.lo_at(best) >> 1;
                L.mark_expanded(best, lane);
            }
        }

        // ---- the hop: fill the staging area from the row of G'', flush it through the hop step ---------------------------------------
        int cnt = 0;         // ids staged
        bool mixed = false;  // looked-through ids are among them (sticky for the hop): the first-occurrence filter runs
        // a chunk of 32 staged ids with its rows: walk_reg_one's pass over a chunk of allowed neighbours, behind the first-occurrence filter
        auto step = [&](uint32_t nb, const RowRegs<kQSteps>& rr) -> bool {
            bool valid = nb != kInvalidId;
            uint64_t mv = __ballot(valid);
            if (mixed) {  // of equal ids the first occurrence stays
                uint64_t dup = 0ull;
                for (uint64_t rem = mv & kSlotLanes; rem;) {
                    const int j = __ffsll((unsigned long long)rem) - 1;
                    const uint64_t eq = __ballot(valid && nb == readlane_u32(nb, j));
                    dup |= eq & ~(3ull << j);
                    rem &= ~eq;
                }
                mv &= ~dup;
                valid = __builtin_amdgcn_inverse_ballot_w64(mv);
            }
            // the even lane of a pair tests / claims the id, the odd lane ends up with the distance
            uint64_t mclaimed;
            if (vs_shr) {
                uint64_t movf;
                mclaimed = visited_claim_mask_quotient(hash_lds, nbuckets, nb, mv & kSlotLanes, vs_shr, movf);
                if (__builtin_expect(movf != 0, 0)) {
                    if (!stash_claim(hash_lds, nbuckets, movf, nb, mclaimed, lane)) return false;
                }
            } else mclaimed = visited_claim_mask_packed(hash_lds, nbuckets, nb, mv & kSlotLanes);
            const uint64_t mfresh = mclaimed << 1;
            const bool fresh = __builtin_amdgcn_inverse_ballot_w64(mfresh);
            uint32_t kd;
            if constexpr (kAlt) kd = fkey(dot_pair_from_regs(rr, qreg.v));
            else if constexpr (STEPS == 8) kd = fkey_sumsq(l2_pair_from_regs(rr, qreg.v));
            else kd = fkey_sumsq(l2_pair_from_regs_wide<kQSteps>(rr, qreg.v));
            const uint32_t dk = fresh ? kd : 0xFFFFFFFFu;
            dist_calc += __popcll(mfresh);
            const bool offer_it = fresh && (size < ef || dk < worst);
            uint64_t m = __ballot(offer_it);
            // several survivors: one batch merge (falls through to the sequential offers on a boundary tie)
            if ((m & (m - 1)) != 0) {
                bool merged;
                if constexpr (R == 1) merged = reg_merge(m, offer_it, dk, nb, L, size, worst, tsize, stage, ef, lane);
                else merged = reg_merge_multi<R>(m, offer_it, dk, nb, L, size, worst, tsize, stage, ef, lane);
                if (merged) m = 0;
            }
            while (m) {
                const int l = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                if (!reg_offer<R>(readlane_u32(dk, l), readlane_u32(nb, l) << 1, L, size, worst, tsize, tie, ef, lane)) return false;
            }
            return true;
        };
        auto flush = [&]() {
            wave_sync();
            for (int c = 0; c < cnt; c += 32) {
                if ((uint32_t)dist_calc + 64u > p.hash_limit) { status = 2; return; }
                // every lane loads (empty slots read row 0), ahead of the filter and the visited test: their LDS round trips overlap the gather
                // (both chunks' rows at once and eight looked-through rows a batch measured slower: 0.59 against 0.49 ms with every row
                // allowed, 5.0 against 4.5 with half of them, sift ef 64 -- 20 to 35 more registers)
                const uint32_t nb = (c + (int)slot < cnt) ? bst[c + slot] : kInvalidId;
                const uint32_t roff = (nb != kInvalidId ? nb : 0u) * kRowBytes + half * (kAlt ? 16u : kRowBytes / 2u);
                const float* rp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.db) + roff);
                RowRegs<kQSteps> rr;
                if constexpr (kAlt) load_row_alt(rr, rp);
                else load_row<kQSteps>(rr, rp);
                if (!step(nb, rr)) { status = 2; return; }
                asm volatile("" ::"v"(roff));  // (the address register does not double as a load destination, walk_reg_one)
            }
            wave_sync();
            cnt = 0;
        };
        // appends the ids of the lanes with `pred`, in lane order; a full staging area is flushed on the way
        auto emit = [&](uint32_t id, bool pred) {
            const uint64_t m = __ballot(pred);
            if (!m) return;
            edges += __popcll(m);
            const int idx = cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const int tot = cnt + __popcll(m);
            if (pred && idx < kBridgeStageIds) bst[idx] = id;
            if (tot >= kBridgeStageIds) {
                cnt = kBridgeStageIds;
                flush();
                if (status) return;
                if (pred && idx >= kBridgeStageIds) bst[idx - kBridgeStageIds] = id;
                cnt = tot - kBridgeStageIds;
            } else cnt = tot;
        };
        {
            const uint32_t stride = p.ell_stride;
            const uint32_t* row = reinterpret_cast<const uint32_t*>(row_ptr<true>(reinterpret_cast<const float*>(p.ell), node, stride));
            for (uint32_t c = 0; c < stride; c += 64) {
                const uint32_t nb = (c + lane < stride) ? row[c + lane] : kInvalidId;
                const bool live = nb != kInvalidId;
                const uint64_t mlive = __ballot(live);
                if (!mlive) break;  // the end of the row: decided before the tag test
                const uint32_t tg = live ? tag_word(p.tags, nb) : 0u;
                const bool allowed = live && (tg & qtag) != 0u;
                uint64_t md = mlive & ~__ballot(allowed);  // disallowed live slots: looked through
                int pos = 0;                               // slots of this chunk below it are emitted
                while (md) {
                    // up to kBridgeBatch looked-through rows at once: their first 64 slots, then the tag words of those
                    int d[kBridgeBatch];
                    uint32_t w[kBridgeBatch], t[kBridgeBatch];
                    int nd = 0;
#pragma unroll
                    for (int k = 0; k < kBridgeBatch; ++k) {
                        d[k] = 64;
                        w[k] = kInvalidId;
                        if (md) {
                            d[k] = __ffsll((unsigned long long)md) - 1;
                            md &= md - 1;
                            nd = k + 1;
                            const uint32_t* vrow = reinterpret_cast<const uint32_t*>(row_ptr<true>(reinterpret_cast<const float*>(p.ell), readlane_u32(nb, d[k]), stride));
                            if ((uint32_t)lane < stride) w[k] = vrow[lane];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < kBridgeBatch; ++k) t[k] = w[k] != kInvalidId ? tag_word(p.tags, w[k]) : 0u;
#pragma unroll
                    for (int k = 0; k < kBridgeBatch; ++k) {
                        if (k < nd) {
                            emit(nb, allowed && lane >= pos && lane < d[k]);
                            if (status) goto hop_done;
                            mixed = true;
                            const bool live2 = w[k] != kInvalidId;
                            if (__ballot(live2)) {
                                emit(w[k], live2 && (t[k] & qtag) != 0u);
                                if (status) goto hop_done;
                                // (rows beyond 64 slots: the further chunks one after the other)
                                const uint32_t* vrow = reinterpret_cast<const uint32_t*>(row_ptr<true>(reinterpret_cast<const float*>(p.ell), readlane_u32(nb, d[k]), stride));
                                for (uint32_t c2 = 64; c2 < stride; c2 += 64) {
                                    const uint32_t nb2 = (c2 + lane < stride) ? vrow[c2 + lane] : kInvalidId;
                                    const bool l2 = nb2 != kInvalidId;
                                    if (!__ballot(l2)) break;
                                    emit(nb2, l2 && (tag_word(p.tags, nb2) & qtag) != 0u);
                                    if (status) goto hop_done;
                                }
                            }
                            pos = d[k] + 1;
                        }
                    }
                }
                emit(nb, allowed && lane >= pos);
                if (status) goto hop_done;
            }
            if (cnt) flush();
        }
    hop_done:
        if (status) break;
        hops += 1;
    }

    if (status == 2) {
        if (lane == 0) {
            const uint32_t s = atomicAdd(ovf_count, 1u);
            ovf_list[s] = qi;
        }
        return;
    }
    reg_write_results<R>(p, qi, L, size, hops, dist_calc, edges, lane);
    if (p.rr_db) {
        const int kept = size < p.k ? size : p.k;
        fused_rerank(p, qi, kept, smem, lane, [&](int rank) { return reg_id_at_rank<R>(L, rank); });
    }
}

template <int METRIC, int STEPS, int R>
__global__ __launch_bounds__(64) void walk_bridge_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_bridge_one<METRIC, STEPS, R>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

#define WALK_BRIDGE(M, S, R) {{WalkFamily::RegList, M, S, R, kOff32 | kTag | kBridge}, WALK_KERNEL(walk_bridge_kernel<M, S, R>)}
#define WALK_BRIDGE_SET(M, S) WALK_BRIDGE(M, S, 1), WALK_BRIDGE(M, S, 2)

const WalkEntry kEntries[] = {WALK_BRIDGE_SET(0, 8), WALK_BRIDGE_SET(1, 8), WALK_BRIDGE_SET(0, 12), WALK_BRIDGE_SET(0, 16)};

}  // namespace

const WalkEntry* walk_bridge_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
