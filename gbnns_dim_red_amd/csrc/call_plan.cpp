// call_plan.cpp -- call_plan: which kernels one search call launches, on which visited set, decided from const facts (call_plan.h).  Plain host
// code.  The order of the steps is the behaviour: plan, the coop rule, sizing, the coop residency check (re-plan and re-size), all_general, the
// bitmap rule, the late-rows rule, re-plan, the fuse room, skip_retry, the retry plan.  Which instance serves a shape stays walk_plan.cpp's.
#include "call_plan.h"

#include <algorithm>
#include <cstdlib>

namespace gbnns_api {

void set_walk_shape(WalkParams& w, const CallFacts& f) {
    static const uint32_t present[4] = {};  // (the plan asks only WHETHER there is an auxiliary graph, and whether the call brought byte queries)
    w.dim = f.dim; w.dstride = f.dstride; w.n = (uint32_t)f.n; w.ell_stride = f.ell_stride; w.ef = f.ef; w.n_entries = f.n_entries ? f.n_entries : 1u;
    w.nq = f.nq;
    w.aux_ell = f.aux_stride ? present : nullptr; w.aux_stride = f.aux_stride;
    w.half_rows = f.half_rows ? 1 : 0;
    w.tagged = f.tagged ? 1 : 0; w.bridged = f.bridged ? 1 : 0;
    w.walk_bytes = f.walked == RowKind::U8 ? 1 : 0;
    w.walk_half = f.walked == RowKind::F16 ? 1 : 0;
    w.half_general = (w.walk_half && !f.knob.half_walk_fast) ? 1 : 0;
    w.half_unkept = (w.walk_half && f.knob.half_walk_fast == 2) ? 1 : 0;
    // byte queries: the plan may name the integer twin of a byte-walk instance (walk_plan.cpp; knob "byte_query_int": for which beam classes)
    w.q_b = (w.walk_bytes && f.byte_queries) ? reinterpret_cast<const uint8_t*>(present) : nullptr;
    w.bq_classes = w.walk_bytes ? (uint32_t)f.knob.byte_query_int : 0u;
    w.stamps_on = f.stamps_on ? 1 : 0;
    w.force_wide = (f.flags & GBNNS_FLAG_WIDE_INDEX) ? 1 : 0;
    w.generic_only = f.knob.hot ? 0 : 1;
}

void set_walked_table(WalkParams& w, RowKind walked, const void* table) {
    w.db = walked == RowKind::F32 ? static_cast<const float*>(table) : nullptr;
    if (walked == RowKind::U8) w.db_b = static_cast<const uint8_t*>(table);
    if (walked == RowKind::F16) w.db_h = table;
}

void set_fused_rerank_table(WalkParams& w, RowKind rows, const void* table) {
    w.rr_db = rows == RowKind::F32 ? static_cast<const float*>(table) : nullptr;
    w.rr_db_b = rows == RowKind::U8 ? static_cast<const uint8_t*>(table) : nullptr;
}

// the decision fields, under the same names in WalkParams and CallPlan: out of the plan's scratch parameters, into a call's
template <class From, class To>
static void copy_decisions(const From& a, To& b) {
    b.coop = a.coop; b.late_rows = a.late_rows; b.spec_rows = a.spec_rows; b.spec_from = a.spec_from;
    b.vs_shr = a.vs_shr; b.hash_cap = a.hash_cap; b.hash_limit = a.hash_limit;
    b.all_general = a.all_general; b.rr_reserve = a.rr_reserve; b.bytes_dim = a.bytes_dim; b.force_wide = a.force_wide; b.generic_only = a.generic_only;
}
void CallPlan::apply(WalkParams& w) const { copy_decisions(*this, w); }

namespace {

size_t granules(size_t bytes) { return (bytes + kLdsGran - 1) / kLdsGran * kLdsGran; }
size_t first_lds(const WalkParams& w, const WalkPlan& plan) { return plan.lds_fixed + walk_hash_bytes(w.hash_cap, plan.hash_form(w.vs_shr)); }

// sizing statistics are kept per (ef, mode, aux, wide, byte instances: no retry pass behind them, half rows: another table, other walks; tagged: other graphs, shorter walks; bridged: two to three times the rows claimed; knob "hot" = 0: other kernels; a half-base handle: a class of its own, like the byte handle's; a half walk, GBNNS_FLAG_HALF_WALK: one more -- bit 23 --, and with the knob "half_walk_fast" = 0 another -- bit 22: other kernels; beams below 2^18)
int stats_key(const CallFacts& f, const WalkParams& w) {
    const bool aux = f.aux_stride != 0;
    return ((f.ef * 8 + f.mode * 2 + (aux ? 1 : 0)) * 2 + w.force_wide) | (w.half_rows ? 1 << 30 : 0) | (w.tagged ? 1 << 29 : 0) | (w.bridged ? 1 << 27 : 0) | (w.generic_only ? 1 << 28 : 0) | (w.bytes_dim ? 1 << 26 : 0) | (w.walk_bytes ? 1 << 25 : 0) | (f.rows == RowKind::F16 ? 1 << 24 : 0) | (w.walk_half ? 1 << 23 : 0) | (w.half_general ? 1 << 22 : 0);
}

// A small batch that runs ALONE (the reference's gist row: 1 000 queries per synchronous call, final_test.cpp:87) on the shapes that
// have it: the two-wavefront walk (walk_coop.hip) -- a keeper wavefront with the result lists, a scout wavefront that expands the
// predicted next node ahead.  One wavefront per query leaves such a launch a chain of dependent latencies on a mostly idle machine
// (at most four queries per CU); measured on the gist shape at ef 200: first-pass kernel 0.487 against 0.526 ms.  NOT with batches in
// flight: those fill the machine by themselves and are bound by bytes, and the second wavefront's issue slots and speculative rows
// cost them (1.8 against 2.5 M queries/s).  Knob "coop": 0 never, 1 whenever the shape allows (tests), -1 this rule.
bool coop_rule(const CallFacts& f, const WalkPlan& plan) {
    const int knob = f.knob.coop;
    return knob != 0 && f.n_entries == 1 && !(f.flags & (GBNNS_FLAG_BITMAP_PASS | GBNNS_FLAG_WIDE_INDEX)) && plan.coop_serves &&
           (knob > 0 || (f.nq <= 4u * f.cus && !f.in_flight));
}

// Large ef: the visited table of such a walk would leave a handful of wavefronts per CU, so the first pass
// keeps its visited sets as bitmaps in HBM and runs as many persistent wavefronts as the LDS holds result
// lists (LDS-list kernel); taken when that at least doubles the resident wavefronts.
// Returns the wavefronts per CU of the bitmap pass; 0: the first pass keeps its visited sets in LDS.
size_t bitmap_rule(const CallFacts& f, const WalkParams& w, const WalkPlan& plan, int form) {
    const int ef = f.ef;
    const uint32_t nq = f.nq;
    const size_t cus = f.cus;
    // measured crossover on the GloVe-like shape: ef = 300 is faster with the register list + LDS table
    // (4.3 vs 5.5 ms), ef = 400 with the bitmap pass (7.1 vs 9.4 ms); SIFT-like ef <= 180 clearly the former
    // (with the register-list variant of the pass: ef = 300 4.2 vs 4.3 ms, a tie; SIFT-like ef 140 .. 180 5.2 .. 4.3
    // against 8.5 .. 6.0 M queries/s on the hot instances -- clearing n/8 bytes per query is not free there)
    // with the quotient form of the table (round 3) the crossover moved up: GloVe-like ef = 400 3.85 ms (table) against
    // 4.85 (bitmap pass), ef = 500 5.61 / 5.51, ef = 600 8.86 / 6.83; SIFT-like ef = 450 4.41 / 4.68, ef = 500 5.30 / 5.29
    static const int min_ef_env = getenv("GBNNS_BITMAP_MIN_EF") ? atoi(getenv("GBNNS_BITMAP_MIN_EF")) : 0;  // (tuning runs)
    // 576-byte rows (the reference's glove 300 -> 144; pair form of the two-list kernels, 8 wavefronts per CU by registers whatever
    // the table): walk + re-rank at ef 600 / 800 / 1 000 11.2 / 18.5 / 23.7 ms with the table against 12.5 / 16.3 / 20.1 with the
    // bitmap pass in the same form and its rows requested after the bit test -- the bitmap pass from ef = 700
    const bool rows576 = w.dim == 144u && w.dstride == 144u && f.metric == GBNNS_METRIC_L2;
    // (second half of round 5: for 576-byte rows the beam alone does not decide -- on a GD(M = 30) graph ef = 600 computes 10 500
    // distances per query, four wavefronts per CU by LDS, 21.4 ms on the table against 1.75 us per distance on the bitmap pass; the rule
    // below -- the pass must at least double the resident wavefronts: 8 by registers against <= 4 by the table -- does from ef 450 on)
    const int min_ef = min_ef_env ? min_ef_env : (rows576 ? 450 : (form == 2 ? 480 : 385));
    const bool forced = (f.flags & GBNNS_FLAG_BITMAP_PASS) != 0;  // diagnostic: whatever ef and batch size
    if (w.all_general || w.coop || w.tagged || w.walk_bytes || w.walk_half || !(ef >= min_ef || forced) || (f.flags & GBNNS_FLAG_WIDE_INDEX) || !(f.hash_capacity == 0 || forced))
        return 0;
    const WalkPlan bitmap_plan = plan_walk(w, f.metric, WalkPass::Bitmap);
    const size_t per_wave = granules(bitmap_plan.lds_fixed);   // (the slot counts below follow the device's CU count, as in sizing.cpp)
    const size_t per_cu = std::min<size_t>(rows576 ? 8 : 32, kMaxLds / per_wave);  // (576-byte rows: 223 registers, two wavefronts per SIMD)
    const size_t table_waves = std::min<size_t>(32, kMaxLds / granules(first_lds(w, plan)));
    // ... and only when the batch is deeper than 1.5 rounds of the wavefronts the table would allow (a
    // 1 000-query batch is resident at once either way, and the register list is faster per hop)
    // ... or, short of that, when the table needs a second round and the bitmap pass holds the whole batch at once
    const bool one_round = (size_t)nq > table_waves * cus && (size_t)nq <= per_cu * cus;
    if (((per_cu >= 2 * std::max<size_t>(table_waves, 1) && (2 * (size_t)nq > 3 * table_waves * cus || one_round)) || forced) &&
        per_cu >= 1 && per_cu * cus * (size_t)bitmap_words_of(f.n) * 4 <= (8ull << 30))
        return per_cu;
    return 0;
}

// Two-list kernels over wide rows: rows after the visited test where the launch is bound by bandwidth -- 576-byte rows with at
// least five wavefronts per CU by LDS (ef 300 / 400 / 600: 4.15 / 5.36 / 10.4 against 5.08 / 6.74 / 10.7 ms; ef 800 / 1 000, four and
// fewer per CU: 18.2 / 23.8 against 17.4 / 22.3) on a batch that fills the machine
int late_rows_rule(const CallFacts& f, const WalkParams& w, const WalkPlan& plan, size_t bitmap_per_cu) {
    if (w.walk_half) return 0;  // (GBNNS_FLAG_HALF_WALK: no instance with its rows requested late)
    const int knob = f.knob.late_rows;
    const size_t per_wave = granules(first_lds(w, plan));
    const size_t lds_waves = per_wave ? kMaxLds / per_wave : 0;
    // ... and 192-byte rows at ef <= 64 (walk_reg_wide_kernel<12>, the reference's deep 96 -> 48: 2.24 GB moved for 1.62 GB of
    // algorithmic bytes at ef = 40, 6.5 TB/s; 0.351 -> 0.342 ms alone, 29.4 -> 30.9 M queries/s in flight; its longer beams: no gain)
    const bool l2 = f.metric == GBNNS_METRIC_L2 && w.dim == w.dstride && f.nq >= 2048u;
    // ... and the 384- / 512-byte rows of PLAIN walks over deep / sift vectors at beams of more than 128 (2.15 -> 2.08 ms at d = 128,
    // ef = 140; 1.63 -> 1.52 ms at d = 96, ef = 160)
    const bool big_rows = w.dim == 144u || ((w.dim == 96u || w.dim == 128u) && f.ef > 128);
    const bool auto_late = l2 && ((big_rows && lds_waves >= 5) || (w.dim == 48u && f.ef <= 64));
    // (the bitmap pass over 576-byte rows: always -- 8 wavefronts per CU whatever the beam)
    const bool bitmap_late = bitmap_per_cu != 0 && w.dim == 144u && l2;
    return knob < 0 ? ((auto_late || bitmap_late) ? 1 : 0) : knob;
}

// retry pass: hand-overs of the first pass, one wavefront per CU with all the LDS
void retry_rule(const CallFacts& f, const WalkParams& w, CallPlan& cp) {
    const bool bytes = f.rows == RowKind::U8;
    WalkParams w2 = w;
    w2.vs_shr = 0;  // (the retry kernels keep the packed form)
    w2.coop = 0;    // (... and one wavefront per query)
    cp.retry = plan_walk(w2, f.metric, WalkPass::Retry);
    cp.retry_hash_cap = walk_hash_entries(kMaxLds / kLdsGran * kLdsGran - cp.retry.lds_fixed, cp.retry.hash_form(0));
    cp.retry_hash_limit = cp.retry_hash_cap - cp.retry_hash_cap / 16;
    if (cp.skip_retry)
        cp.retry_action = RetryAction::None;  // nothing to launch
    else if (cp.retry_hash_cap > cp.sizing.cap && !w.tagged && !(cp.fuse && bytes) && !w.walk_bytes && !w.walk_half)  // (a tagged first pass has no retry pass: its hand-overs go straight to the general kernel; a byte instance's and a byte walk's to the general kernel's byte instances, a half walk's to its half-walk instance)
        cp.retry_action = RetryAction::Launch;
    else
        cp.retry_action = RetryAction::Copy;  // nothing to gain: A -> B
}

}  // namespace

CallPlan call_plan(const CallFacts& f, const SizingHistory& h) {
    CallPlan cp{};
    const bool plain = f.mode == GBNNS_MODE_PLAIN;
    WalkParams w{};
    set_walk_shape(w, f);
    // A byte handle (gbnns_index_create_bytes): the re-rank is fused only into the byte instances (walk_plan.cpp decides, from bytes_dim);
    // every other first pass runs as on a float handle with GBNNS_FLAG_NO_FUSED_RERANK, the stand-alone byte kernel behind it
    const bool bytes = f.rows == RowKind::U8;
    if (bytes && !plain && !(f.flags & GBNNS_FLAG_NO_FUSED_RERANK) && rerank_plan(f.metric, f.d, true).fuses) w.bytes_dim = f.d;
    // (a byte walk, GBNNS_FLAG_BYTE_WALK: a bit of its own too -- other kernels, no retry pass, and never the float handle's or the byte re-rank's state)
    cp.skey = stats_key(f, w);
    const int calm = h.calm(cp.skey);
    // The first pass's instance and LDS layout (walk_plan.h); the instance depends on late / speculative rows, decided below: taken again then.
    WalkPlan plan = plan_walk(w, f.metric, WalkPass::First);
    if (coop_rule(f, plan)) {
        w.coop = 1;
        plan = plan_walk(w, f.metric, WalkPass::First);
    }
    // the first pass's visited set: capacity, form (packed / quotient), the wavefronts per CU it leaves (sizing.cpp)
    FirstPassSizing fps = size_first_pass(f, h, cp.skey, w, plan);
    if (w.coop && f.knob.coop < 0) {
        // (auto: only when every workgroup of the batch is resident at once -- LDS share per query, eight workgroups of two wavefronts per CU)
        const size_t per_wg = granules(first_lds(w, plan));
        const size_t per_cu = std::min<size_t>(8, per_wg ? kMaxLds / per_wg : 0);
        if ((size_t)f.nq > per_cu * f.cus) {
            w.coop = 0;
            plan = plan_walk(w, f.metric, WalkPass::First);
            fps = size_first_pass(f, h, cp.skey, w, plan);
        }
    }
    w.all_general = (first_lds(w, plan) > kMaxLds || plan.general_only) ? 1 : 0;
    // Fused re-rank: with a register-list first pass (ef <= 512; and its retry / general successors) every
    // wavefront re-ranks its own query when its walk ends; no re-rank launch.  Needs the pair form
    // (d % 8 == 0) and room for the original-space query in the walk kernels' LDS.
    // (rerank_plan.h: the pair form; L2: d % 8 == 4 too -- glove's 300 -- its last 16-byte step is the even lane's alone)
    // A half-base handle (gbnns_index_create_half_base): rerank_half_plan never fuses -- every first pass runs as on a float handle with
    // GBNNS_FLAG_NO_FUSED_RERANK, the stand-alone half kernel behind it, and sets no LDS aside for a re-rank query
    const bool want_fuse = f.rows == RowKind::F16 ? rerank_half_plan(f.metric, f.d).fuses
                                       : (bytes ? w.bytes_dim != 0u : (!plain && rerank_plan(f.metric, f.d, false).fuses && !(f.flags & GBNNS_FLAG_NO_FUSED_RERANK)));
    w.rr_reserve = (want_fuse && !bytes) ? (uint32_t)f.d_pad * 4u : 0u;  // (the bitmap pass has no byte instance)
    cp.bitmap_per_cu = bitmap_rule(f, w, plan, fps.form);
    cp.bitmap_pass = cp.bitmap_per_cu != 0;
    w.late_rows = late_rows_rule(f, w, plan, cp.bitmap_per_cu);
    cp.first = plan_walk(w, f.metric, cp.bitmap_pass ? WalkPass::Bitmap : WalkPass::First);
    // (the two-list instances keep their result list in LDS and stage the re-rank query in the visited-set area)
    const size_t rr_room = cp.first.rr_room(walk_hash_bytes(w.hash_cap, cp.first.hash_form(w.vs_shr)));
    cp.fuse = !cp.first.lds_list && want_fuse && !w.all_general && (size_t)f.d_pad * 4 <= rr_room && (!bytes || (cp.first.inst.flags & kRrBytes));
    // Once batches of this (ef, mode) have been calm (no hand-over, size settled), the retry launch is left
    // out: the first pass then appends what it cannot finish to list B directly and the general kernel --
    // always launched -- takes it.  Still exact; a surprise hand-over is just slower once, and un-calms.
    cp.skip_retry = fps.auto_cap && calm >= 2 && !w.all_general;
    cp.sizing = fps;
    cp.retry_action = RetryAction::None;
    if (!w.all_general) retry_rule(f, w, cp);
    copy_decisions(w, cp);
    return cp;
}

}  // namespace gbnns_api
