// walk_plan.cpp -- plan_walk: the one mapping from (shape, beam, pass) to a walk kernel instance and its LDS layout (walk_plan.h).  Plain host code.
// The tuning rules (when the two-wavefront walk, the bitmap pass, late or speculative rows are WANTED) stay in call_plan.cpp and sizing.cpp.
#include "walk_plan.h"
#include <cstdlib>

namespace gbnns {

const WalkEnv& walk_env() {
    static const WalkEnv env{!getenv("GBNNS_WIDE2") || atoi(getenv("GBNNS_WIDE2")) != 0, getenv("GBNNS_STAMPS_GENERIC") != nullptr};  // read once
    return env;
}

// "compact" index: every table the walk indexes is < 4 GiB (32-bit byte offsets) and ids fit 24 bits
static bool compact_index(const WalkParams& p) {
    return !p.force_wide && (uint64_t)p.n * p.dstride * 4 < (1ull << 32) && (uint64_t)p.n * p.ell_stride * 4 < (1ull << 32) &&
           (!p.aux_ell || (uint64_t)p.n * p.aux_stride * 4 < (1ull << 32)) && p.n <= 0xFFFFFFu;
}

// LDS of one wavefront without the visited set.  Register kernels: tie list + merge buffer + query (the hot kernel stages it inside the merge buffer).
static size_t lds_fixed_bytes(int ef, uint32_t dstride, bool hot, bool lds_list, bool coop) {
    if (coop) return big_list_fixed_bytes(ef) + (size_t)dstride * 4 + kCoopExtraLds;  // (walk_coop.hip: the two-list layout + result buffers)
    if (hot)  // tie list + merge buffer of 1 / 2 list registers; ef > 128: + the base list and the flush's flag bytes (walk_hot_big)
        return ef <= 64 ? (size_t)kRegTieCap * 8 + (size_t)kRegStageSlots * 8 + (GBNNS_HOT1_QLDS ? 128 : 0)   // (+ the query, re-read every hop)
                        : (ef <= kHot2MaxEf ? (size_t)kRegTieCap * 8 + (size_t)(64 * 2 + 2) * 8 : big_list_fixed_bytes(ef));
    if (!lds_list) {  // tie list + merge buffer (ranks 0..ef of the 1 / 2-register list) + query
        if (ef > kHot2MaxEf) return big_list_fixed_bytes(ef) + (size_t)dstride * 4;  // walk_reg_big_one
        return (size_t)kRegTieCap * 8 + (size_t)(64 * (ef <= 64 ? 1 : 2) + 2) * 8 + (size_t)dstride * 4;
    }
    return (((size_t)ef + 63) & ~(size_t)63) * 8 + (size_t)kTieCap * 8 + (size_t)dstride * 4;  // the list, padded to 64 entries + tie list + query
}

// The half instances (walk_half.hip): first pass, one wavefront and one entry point per query, no auxiliary graph, compact index, unpadded rows
// (the caller has checked those: `steps` is only set for unpadded rows) of 32 / 48 / 64 floats with L2 and 32 floats with the negative dot in
// the one- / two-register-list and two-list kernels, of 144 floats with L2 in the two-list kernel.  Everything else walks the float32 copy of R.
static bool half_serves(int metric, int steps, int regs, uint32_t n_entries) {
    if (n_entries > 1u) return false;
    if (steps == 8) return true;
    return metric == 0 && (steps == 12 || steps == 16 || (steps == 36 && regs == 4));
}

// The tag instances (walk_tag.hip): the same shapes -- first pass of a compact index, one entry point per query, no auxiliary graph (plan_walk
// checks those).  A tagged call outside them runs whole on the general kernel (WalkPlan::general_only).
static bool tag_serves(int metric, int steps, int regs) { return half_serves(metric, steps, regs, 1u); }

// The bridge instances (walk_bridge.hip): the tag instances' domain cut to the register lists (ef <= 128) over rows of 32 / 48 / 64 floats.  The
// two-list shapes (beams above 128, 144-float rows) of a bridged call run whole on the general kernel.
static bool bridge_serves(int metric, int steps, int regs) { return regs <= 2 && (steps == 8 || (metric == 0 && (steps == 12 || steps == 16))); }

WalkPlan plan_walk(const WalkParams& p, int metric, WalkPass pass, const WalkEnv& env) {
    const bool off32 = compact_index(p), aux = p.aux_ell != nullptr, retry = pass == WalkPass::Retry;
    const int ef = p.ef, regs = ef <= 64 ? 1 : (ef <= kHot2MaxEf ? 2 : 4);
    const uint32_t rows = p.dim == p.dstride ? p.dim : 0u;  // floats of an unpadded row (0: padded -- run-time-length instances only)
    const bool one = p.ell_stride <= 32u, late = p.late_rows != 0;
    WalkPlan pl{};
    WalkInstance& k = pl.inst;
    pl.pass = pass;
    // (gbnns_search_tagged: first pass only -- a tagged call has neither a retry nor a bitmap pass, call_plan.cpp)
    const bool tag = p.tagged != 0 && pass == WalkPass::First;
    const bool bridge = tag && p.bridged != 0;  // GBNNS_FLAG_TAG_BRIDGE: a table and instances of their own
    pl.general_only = p.n_entries > 1 || (tag && (aux || !off32));
    // The LDS-list kernel serves ef beyond the register lists, and auxiliary-graph walks over tables >= 4 GiB (the register-list /
    // two-list kernels have their auxiliary-graph hop in the 32-bit-offset instances only).
    pl.lds_list = ef > kRegListMaxEf || (aux && !off32);
    // Every LDS kernel packs its visited set when ids fit 24 bits (the register-list kernels: in their compact, 32-bit-offset instances).
    pl.packed = pl.lds_list ? (p.n <= 0xFFFFFFu && !p.force_wide) : off32;
    // (a visited set in the packed form: no id may look like a half-written slot -- see visited_test_mask_packed)
    pl.coop_serves = metric == 0 && (rows == 32u || rows == 48u || rows == 64u) && regs == 4 && ef <= kRegListMaxEf && off32 && p.n < 0xFF0000u && !aux &&
                     one && p.n_entries <= 1u && !tag;
    if (p.walk_bytes) {
        // GBNNS_FLAG_BYTE_WALK: the walked rows are a byte handle's uint8 rows (WalkParams::db_b; dstride = the BYTES of a row).  The byte-walk
        // instances (walk_bytes.hip): first pass, L2 over 128-byte rows of d = 128 (eight 16-byte chunks a lane pair shares), compact index
        // (the byte table, the adjacency table < 4 GiB, 24-bit ids), one entry point per query, no auxiliary graph, untagged, ef <= 1 024 --
        // the register lists with ONE_CHUNK, the two-list kernel with ONE_PASS where the adjacency rows are one 32-slot pass.  Everything else
        // runs whole on the general kernel's byte-walk instance, which is also where a fast instance's hand-overs go: there is no byte form of
        // the retry pass, the bitmap pass, the two-wavefront walk, the walk_hot* family, late / speculative rows or the LDS-list kernel.
        const bool compact = !p.force_wide && (uint64_t)p.n * p.dstride < (1ull << 32) && (uint64_t)p.n * p.ell_stride * 4 < (1ull << 32) && p.n <= 0xFFFFFFu;
        const bool fast = pass == WalkPass::First && metric == 0 && p.dim == 128u && p.dstride == 128u && compact && p.n_entries <= 1u && !aux && !p.tagged &&
                          ef <= kRegListMaxEf;
        pl.coop_serves = false;
        pl.lds_list = false;
        pl.general_only = !fast;
        if (fast) {
            k = {regs == 4 ? WalkFamily::TwoList : WalkFamily::RegList, 0, 8, regs, kOff32 | flag_if(one, kOne) | kByteWalk};
            pl.packed = true;
            pl.lds_fixed = lds_fixed_bytes(ef, p.dstride, false, false, false);  // (the query: dstride = 128 floats, re-read from LDS every hop)
            pl.knows_quotient = true;  // (as the float pair-form instances of a compact index)
            // gbnns_search_byte_queries: the call brought its queries as bytes -- the integer twin of the same instance (walk_bytes_q.hip), for the
            // beam classes the handle's knob "byte_query_int" names.  Its query lives in registers: no query area in LDS.
            if (p.q_b && (p.bq_classes & (regs == 4 ? 4u : (uint32_t)regs))) {
                k.flags |= kByteQuery;
                pl.lds_fixed = lds_fixed_bytes(ef, 0u, false, false, false);
            }
        }
        return pl;  // (no rr_* room: PLAIN has no re-rank)
    }
    if (p.walk_half) {
        // GBNNS_FLAG_HALF_WALK: the walked rows are a half-base handle's binary16 rows (WalkParams::db_h; dstride = the HALVES of a row).  The
        // half-walk instances (walk_half_base.hip): first pass, L2, compact index (the half table, the adjacency table < 4 GiB, 24-bit ids), one
        // entry point per query, no auxiliary graph, untagged, ef <= 1 024 --
        //   d = 96 (192-byte rows): the 24-step pair form in the instance set the float path has for it -- one list register over one- and
        //     two-pass adjacency rows, two list registers over one-pass rows, the two-list kernel without and with the pass loop;
        //   d >= 128, d % 4 == 0: the run-time-length instances on l2_pair_rows_half -- one list register (ONE_CHUNK: rows of one 64-slot pass),
        //     two list registers, the two-list kernel (ONE_PASS likewise).
        // Everything else -- and the whole batch with the handle knob "half_walk_fast" = 0 (WalkParams::half_general) -- runs on the general kernel's
        // half-walk instance, which is also where a fast instance's hand-overs go: there is no half form of the retry pass, the bitmap pass,
        // the two-wavefront walk, the walk_hot* family, late rows or the LDS-list kernel.
        // The rule (tools/half_walk_timing.py, profiles/half_walk_timing.txt): a dimension class stays on its fast instance only if
        // that beat the general instance by more than the float baseline's own run-to-run range in the same run, at every beam of the class.
        //   d = 96 (deep, 10^6 x 96, 10 000 queries, ef 40 / 80 / 120 / 160 / 200): fast 0.371 / 0.681 / 0.930 / 1.454 / 1.980 ms against the general
        //     instance's 45.0 / 78.8 / 107.4 / 143.9 / 180.5 ms, float ranges 0.007 - 0.027 ms: KEPT.
        //   d >= 128 (gist's 960, glove's 300): not measured yet -- by the rule such a class goes to the general instance (kLongRowsKept); its
        //     fast instances run with the handle knob "half_walk_fast" = 2 (WalkParams::half_unkept: the timing tool and the tests).
        constexpr bool kLongRowsKept = false;
        const bool compact = !p.force_wide && (uint64_t)p.n * p.dstride * 2 < (1ull << 32) && (uint64_t)p.n * p.ell_stride * 4 < (1ull << 32) && p.n <= 0xFFFFFFu;
        const bool domain = !p.half_general && pass == WalkPass::First && metric == 0 && compact && p.n_entries <= 1u && !aux && !p.tagged && ef <= kRegListMaxEf &&
                            p.dstride == ((p.dim + 7u) & ~7u);
        const bool pair24 = domain && p.dim == 96u && (regs == 4 || one || (regs == 1 && p.ell_stride <= 64u));
        const bool longrow = domain && p.dim >= 128u && p.dim % 4u == 0u && (kLongRowsKept || p.half_unkept);
        pl.coop_serves = false;
        pl.lds_list = false;
        pl.general_only = !(pair24 || longrow);
        if (pair24) k = {regs == 4 ? WalkFamily::TwoList : WalkFamily::RegList, 0, 24, regs, kOff32 | flag_if(one, kOne) | kHalfWalk};
        else if (longrow) k = {regs == 4 ? WalkFamily::TwoList : WalkFamily::RegList, 0, 0, regs, kOff32 | flag_if(regs != 2 && p.ell_stride <= 64u, kOne) | kHalfWalk};
        if (!pl.general_only) {
            pl.packed = true;
            pl.lds_fixed = lds_fixed_bytes(ef, p.dstride, false, false, false);  // (the query: dstride floats)
            pl.knows_quotient = true;  // (as the float register-list / two-list instances of a compact index)
        }
        return pl;  // (no rr_* room: PLAIN has no re-rank)
    }
    if (pass == WalkPass::Bitmap) {
        // The bitmap first pass runs the register-list (ef <= 128, L2) / two-list (128 < ef <= 1 024, both metrics) walk for 128-byte rows
        // of a compact index, the two-list walk for 256- and 576-byte rows with L2 (the reference's glove 300 -> 144), else the LDS-list walk.
        const bool reg = (metric == 0 || regs == 4) && ef <= kRegListMaxEf && (rows == 32u || ((rows == 64u || rows == 144u) && metric == 0 && regs == 4)) && off32 && !aux;
        const bool big = reg && regs == 4;
        if (big) k = {WalkFamily::BitmapBig, metric, (int)rows / 4, 0, flag_if(one, kOne) | flag_if(rows == 144u && late, kLate)};
        else if (reg) k = {WalkFamily::BitmapReg, 0, 0, regs};
        else k = {WalkFamily::BitmapLds, metric, metric == 0 && rows == 32u ? 8 : 0};
        pl.lds_list = !reg;
        // no visited table (two-list kernel: + the re-rank query, which cannot overlay the base list it reads its candidates from)
        pl.lds_fixed = lds_fixed_bytes(ef, p.dstride, false, !reg, false) + (big ? p.rr_reserve : 0u);
        pl.rr_base = big ? (size_t)p.rr_reserve : pl.lds_fixed;
        return pl;
    }
    const bool coop = !retry && p.coop && !tag;
    // Shape served by the walk_hot* kernels (first pass only): 128-byte rows, adjacency rows of one 32-slot pass (walk_hotw*: 33 .. 64
    // slots, two passes), compact index (their visited set stores 24-bit ids)
    // (half rows, GBNNS_FLAG_HALF_ROWS: never -- the family reads float32 rows; the generic instances below have half forms)
    const bool half = p.half_rows != 0 && pass == WalkPass::First;
    // (a tagged call: never either -- the generic instances below have tag forms)
    const bool hot = !retry && !coop && !half && !tag && !p.generic_only && (metric == 0 || metric == 1) && rows == 32u && ef <= kBigMaxEf && p.ell_stride <= 64u && off32 &&
             (!p.stamps_on || (regs == 4 && !env.stamps_generic)) && !aux;
    pl.lds_fixed = lds_fixed_bytes(ef, p.dstride, hot, pl.lds_list, coop);
    // the quotient form: the walk_hot* family and the register-list / two-list kernels of a compact index (the retry kernels keep the packed form)
    pl.knows_quotient = !retry && (hot || (off32 && !pl.lds_list && !aux));
    // the re-rank query is staged once the walk is over: two-list instances keep their result list in LDS and use the visited-set area
    pl.rr_in_table = true;
    pl.rr_base = (regs == 4 && !pl.lds_list) ? 0 : pl.lds_fixed;
    if (coop || hot) {  // (the two-wavefront walk on a shape it has no instance for: WalkFamily::None)
        if (hot) k = {WalkFamily::Hot, metric, 0, regs, flag_if(one, kOne) | flag_if(regs == 1 && metric == 0 && one && p.spec_rows && !GBNNS_HOT1_SPEC, kSpec)};
        // a byte handle (gbnns_index_create_bytes) that wants its re-rank fused: where walk_hot_kernel / walk_hot2_kernel serve -- not the
        // speculative-rows instance, not walk_hotw*, not the two-list form -- and the chunk-pair core serves the rows (L2, d % 16 == 0), their
        // byte twins; every other first pass of such a handle runs unfused, followed by the stand-alone byte kernel (rerank_bytes.hip)
        if (hot) k.flags |= flag_if(p.bytes_dim != 0u && p.bytes_dim % 16u == 0u && metric == 0 && regs <= 2 && one && !(k.flags & kSpec), kRrBytes);
        else if (pl.coop_serves) k = {WalkFamily::Coop, 0, (int)rows / 4, 0, flag_if(late, kLate)};
        return pl;
    }
    // steps the generic instances are unrolled for: 128-byte rows (both metrics); with L2 192-, 256- and 576-byte rows and, by beam, the
    // 384- / 512-byte rows of PLAIN walks over deep / sift vectors -- 512-byte rows up to ef = 200 are faster on the run-time-length
    // two-list instance, four lanes per row (ef 130 / 200: 1.72 / 2.77 against 1.93 / 2.87 ms; ef 300 / 400: 5.25 / 8.25 against 4.20 / 5.51)
    int steps = 0;
    if (metric == 1) steps = rows == 32u ? 8 : 0;
    else if (rows == 32u || rows == 48u || rows == 64u || rows == 144u) steps = (int)rows / 4;
    else if (rows == 96u && env.wide2 && regs == 4 && !pl.lds_list) steps = 24;
    else if (rows == 128u && env.wide2 && ef > kPlain512PairMinEf && !pl.lds_list) steps = 32;
    if (pl.lds_list) {
        k = {WalkFamily::LdsList, metric, steps, 0, flag_if(retry, kRetry) | flag_if(pl.packed, kPacked)};
        pl.general_only = pl.general_only || tag;  // (no tag form)
        return pl;
    }
    if (regs == 4) {  // the two-list kernels, one instance for every ef up to 1 024
        const bool l2_unrolled = metric == 0 && steps >= 12;
        k = {WalkFamily::TwoList, metric, steps, 4, flag_if(off32, kOff32) | flag_if(retry, kRetry) | flag_if(aux, kAux)};  // (aux: off32 -- over a non-compact index it is an LDS-list plan)
        if (!aux && off32 && !retry) {
            // the common shape (compact index, adjacency rows of one pass; pair form: 32 slots per pass) gets the hop without the pass loop;
            // 384- / 512- / 576-byte rows have instances with the rows requested after the visited test, in the pass loop too
            k.flags |= flag_if(p.ell_stride <= ((steps == 8 || l2_unrolled) ? 32u : 64u), kOne);
            k.flags |= flag_if(l2_unrolled && steps >= 24 && late, kLate);
            k.flags |= flag_if(half && half_serves(metric, steps, 4, p.n_entries), kHalf);
            k.flags |= flag_if(tag && !bridge && tag_serves(metric, steps, 4), kTag);  // (no bridged two-list instance)
        }
        pl.general_only = pl.general_only || (tag && !(k.flags & kTag));
        return pl;
    }
    // one / two list registers.  384-byte rows: the pair form for the first pass of a compact index over one-pass adjacency rows
    // (two-pass ones: the one-register list only -- GD(M = 30) graph, rows of up to 45 slots, ef 40: 0.678 against 0.763 ms a lane per
    // row; the two-register list 1.254 / 1.834 at ef 80 / 120 against 1.255 / 1.814: stays on the run-time-length instance)
    if (rows == 96u && metric == 0 && env.wide2 && !retry && off32 && !aux && (one || (p.ell_stride <= 64u && regs == 1)) && !p.stamps_on) {
        k = {WalkFamily::RegList, 0, 24, regs, kOff32 | flag_if(one, kOne)};
        pl.general_only = pl.general_only || tag;  // (no tag form)
        return pl;
    }
    if (steps >= 24) steps = 0;  // (576-byte rows at ef <= 128: the run-time-length instances)
    k = {WalkFamily::RegList, metric, steps, regs, flag_if(off32, kOff32) | flag_if(retry, kRetry) | flag_if(aux, kAux)};
    if (!aux && regs == 1 && off32 && !retry && !bridge && p.ell_stride <= ((steps == 8 || (metric == 0 && steps >= 12)) ? 32u : 64u)) {
        // ef <= 64, adjacency rows of one pass: a loop-free expansion; 192- / 256-byte rows with L2: the instance with the query in LDS
        // (half rows: the loop-free expansion of the list family itself -- the query-in-LDS instances have no half form)
        if (metric == 0 && steps >= 12 && !p.stamps_on && !half && !tag && !p.generic_only) k = {WalkFamily::RegWide, 0, steps, 0, flag_if(late, kLate)};
        else k.flags |= kOne;
    }
    k.flags |= flag_if(half && !aux && off32 && half_serves(metric, steps, regs, p.n_entries), kHalf);
    k.flags |= flag_if(tag && !aux && off32 && p.n_entries <= 1u && tag_serves(metric, steps, regs) && (!bridge || bridge_serves(metric, steps, regs)), kTag);
    k.flags |= flag_if(bridge && (k.flags & kTag), kBridge);
    if (k.flags & kBridge) {  // the staged ids of a bridged row sit between the query and the visited set
        pl.lds_fixed += (size_t)kBridgeStageIds * 4;
        pl.rr_base = pl.lds_fixed;
    }
    pl.general_only = pl.general_only || (tag && !(k.flags & kTag));
    return pl;
}

}  // namespace gbnns
