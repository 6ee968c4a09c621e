// search_core.cpp -- one batch on one lane: workspaces, copies in and out, the kernel sequence projection -> first-pass walk (+ retry)
// -> general kernel (-> re-rank), statistics feedback.  Cut out of api.cpp in round 5; the sizing rule it calls is in sizing.cpp.

#include "api_internal.h"

using namespace gbnns;
using namespace gbnns_api;

namespace gbnns_api {

// One (sub-)batch on one lane's workspace, enqueued on stream s; arguments validated by gbnns_search_ex.  With HOST
// buffers the copies in and out are enqueued on s too and, when sync_host, waited for.  `topk` (optional, NET / LOWQ): the k best of
// each query's candidates go to its arrays as well (rerank_topk kernels, behind stage 3).
// `q_u8` (gbnns_search_byte_queries; a->queries is then nullptr): the queries as [n_q x d] bytes, a buffer of a->mem_kind.  They are widened
// into the lane's q_in (widen.hip) and that copy takes a->queries' place everywhere below; the bytes themselves reach the walk as
// WalkParams::q_b, for the integer byte-walk instances.
int search_core(gbnns_index* ix, Lane& L, const gbnns_search_args* a, hipStream_t s, bool sync_host, const TopkOut* topk, const TagIn* tag, const uint8_t* q_u8) {
    int rc;
    const uint32_t n_ent = a->n_entries ? a->n_entries : 1u;
    const bool host = a->mem_kind == GBNNS_MEM_HOST;
    const uint32_t nq = (uint32_t)a->n_q;
    const int ef = a->ef;
    const bool plain = a->mode == GBNNS_MODE_PLAIN;
    const int k = plain ? std::max(1, std::min(a->k > 0 ? a->k : 1, ef)) : ef;
    const uint32_t cstride = (uint32_t)k;

    // ---- workspace ----------------------------------------------------------------------
    if ((rc = L.cnt.ensure((size_t)nq * 4))) return rc;
    if ((rc = L.hops.ensure((size_t)nq * 4))) return rc;
    if ((rc = L.dc.ensure((size_t)nq * 4))) return rc;
    if ((rc = L.ovf_list.ensure((size_t)nq * 4))) return rc;
    if ((rc = L.ovf2_list.ensure((size_t)nq * 4))) return rc;
    if (host || !a->out_cand)
        if ((rc = L.cand.ensure((size_t)nq * cstride * 4))) return rc;
    if (a->out_cand_dist && host)
        if ((rc = L.cand_dist.ensure((size_t)nq * cstride * 4))) return rc;
    // ids into HOST memory: page-locked memory takes the kernels' stores directly (40 KB of a 10 000-query batch: no
    // copy launch behind the walk), pageable memory gets a copy out of the lane's buffer
    uint32_t* const ids_alias = host ? pinned_alias(a->out_ids, (size_t)nq * 4) : nullptr;
    if (host && !ids_alias)
        if ((rc = L.out.ensure((size_t)nq * 4))) return rc;
    if (host && a->out_edges)
        if ((rc = L.edges.ensure((size_t)nq * 4))) return rc;
    if (host && topk) {
        if ((rc = L.top_ids.ensure((size_t)nq * topk->k * 4))) return rc;
        if (topk->dist && (rc = L.top_dist.ensure((size_t)nq * topk->k * 4))) return rc;
    }
    // general-kernel slots: visited bits + tie bits (n / 4 bytes per slot) and the result list -- 16 n bytes + 512 ef
    // per handle in all (see gbnns.h, "Device memory")
    const uint32_t bitmap_words = ((uint32_t)((ix->n + 31) / 32) + 3u) & ~3u;  // per slot; a multiple of 4 words: slots stay 16-B aligned (the bitmap pass clears with 16-B stores)
    {
        const size_t before = L.g_bitmap.bytes;  // (re)allocation always changes the size
        if ((rc = L.g_bitmap.ensure((size_t)kGeneralSlots * 2 * bitmap_words * 4))) return rc;
        // the tie bits must start out all zero (the kernel keeps them so); the visited bits are cleared per query
        if (L.g_bitmap.bytes != before) HIP_TRY(hipMemsetAsync(L.g_bitmap.p, 0, L.g_bitmap.bytes, s));
    }
    if ((rc = L.g_keys.ensure((size_t)kGeneralSlots * ((size_t)ef + n_ent - 1) * 8))) return rc;

    g_slow.mark("workspace");
    // ---- inputs -------------------------------------------------------------------------
    const float* q_dev = a->queries;
    const uint8_t* qb_dev = q_u8;
    if (q_u8) {
        // (HOST buffers, and a DEVICE buffer that does not start on a 16-byte boundary: through the lane's byte staging buffer -- the integer
        // instances read a query as 16-byte pieces)
        const size_t count = (size_t)nq * ix->d;
        if (host || (reinterpret_cast<uintptr_t>(q_u8) & 15u)) {
            if ((rc = L.q_in_b.ensure(count))) return rc;
            if (host) {
                if ((rc = host_copy_in(L, L.q_in_b.p, q_u8, count, s))) return rc;
            } else {
                HIP_TRY(hipMemcpyAsync(L.q_in_b.p, q_u8, count, hipMemcpyDeviceToDevice, s));
            }
            qb_dev = L.q_in_b.as<uint8_t>();
        }
        if ((rc = L.q_in.ensure(count * 4))) return rc;
        q_dev = L.q_in.as<float>();  // (filled by the widening kernel, behind the profile's first event: its time counts as stage 1's)
    } else if (host) {
        if ((rc = L.q_in.ensure((size_t)nq * ix->d * 4))) return rc;
        if ((rc = host_copy_in(L, L.q_in.p, a->queries, (size_t)nq * ix->d * 4, s))) return rc;
        q_dev = L.q_in.as<float>();
    }
    const uint32_t* entries_dev = a->entry_ids;
    if (a->entry_ids && host) {
        if ((rc = L.entries.ensure((size_t)nq * n_ent * 4))) return rc;
        if ((rc = host_copy_in(L, L.entries.p, a->entry_ids, (size_t)nq * n_ent * 4, s))) return rc;
        entries_dev = L.entries.as<uint32_t>();
        // (a tagged call: an entry the query cannot start from is data, HOST and DEVICE buffers alike -- the kernels write its empty row)
        for (size_t i = 0; i < (size_t)nq * n_ent && !tag; ++i)
            if (a->entry_ids[i] >= ix->n) return fail(GBNNS_ERR_INVALID, "entry id %u >= n", a->entry_ids[i]);
    }
    const uint32_t* qtags_dev = tag ? tag->qtags : nullptr;
    if (tag && host) {
        if ((rc = L.qtags.ensure((size_t)nq * 4))) return rc;
        if ((rc = host_copy_in(L, L.qtags.p, tag->qtags, (size_t)nq * 4, s))) return rc;
        qtags_dev = L.qtags.as<uint32_t>();
    }

    g_slow.mark("copy_in");
    ProfCall pc{};
    const bool prof = ix->profiling;
    if (prof) {
        for (int i = 0; i < 5; ++i) HIP_TRY(hipEventCreate(&pc.ev[i]));
        pc.queries = nq;
        HIP_TRY(hipEventRecord(pc.ev[0], s));
    }

    // ---- stage 1: queries in the walked space ------------------------------------------
    WalkParams w{};
    if (q_u8) HIP_TRY(launch_widen_u8(qb_dev, L.q_in.as<float>(), (size_t)nq * ix->d, s));
    if (plain) {
        w.q = q_dev; w.qstride = ix->d; w.db = ix->db; w.dstride = ix->d_pad; w.dim = ix->d;
        if (ix->db_b) {  // GBNNS_FLAG_BYTE_WALK (checked by search_call): the walked rows are the handle's uint8 rows, d_pad bytes each; no float table exists
            w.db = nullptr; w.db_b = ix->db_b; w.walk_bytes = 1;
            // byte queries: the plan may name the integer twin of a byte-walk instance (walk_plan.cpp; knob "byte_query_int": for which beam classes)
            w.q_b = qb_dev; w.bq_classes = (uint32_t)ix->knob.byte_query_int;
        }
    } else {
        if ((rc = L.q_low.ensure((size_t)nq * ix->dl_pad * 4))) return rc;
        float* ql = L.q_low.as<float>();
        if (a->mode == GBNNS_MODE_NET) {
            if ((rc = run_project(ix, L, q_dev, ix->d, nq, ql, s, s == L.stream && L.stream != nullptr,
                                  (a->flags & GBNNS_FLAG_MFMA_PROJECTION) != 0)))
                return rc;
            w.q = ql; w.qstride = ix->dl_pad;
        } else if (host) {
            if ((rc = host_copy_in(L, ql, a->queries_low, (size_t)nq * ix->d_low * 4, s))) return rc;
            w.q = ql; w.qstride = ix->d_low;
        } else {
            w.q = a->queries_low; w.qstride = ix->d_low;
        }
        w.db = ix->db_low; w.dstride = ix->dl_pad; w.dim = ix->d_low;
        if (a->flags & GBNNS_FLAG_HALF_ROWS) {
            // the walked table is R = float32(float16(db_low)): every kernel reads its float32 copy, in db_low's layout, but the half
            // instances of the first pass (walk_plan.cpp), whose hops gather the 2-byte rows
            w.db = ix->low_r.as<float>(); w.db_h = ix->low_half.p; w.half_rows = 1;
        }
        if (a->out_q_low && a->mode == GBNNS_MODE_NET) {
            if (host) {
                if ((rc = host_copy_out(L, a->out_q_low, ql, (size_t)ix->dl_pad * 4, (size_t)ix->d_low * 4, nq, s))) return rc;
            } else {
                HIP_TRY(hipMemcpy2DAsync(a->out_q_low, (size_t)ix->d_low * 4, ql, (size_t)ix->dl_pad * 4,
                                         (size_t)ix->d_low * 4, nq, hipMemcpyDeviceToDevice, s));
            }
        }
    }
    // Deep batches are walked in locality order (walk_common.h, walk_query_of): a counting sort on the sign bits of the
    // first 12 walked-space coordinates, three small launches.  Wavefronts resident together then walk neighbouring
    // regions and find each other's rows in the caches: -8 % kernel time on a 4 M-node index, -3 % on 1 M -- which the
    // sort's launches would eat on a 10 000-query batch, so only from the knob "order_min" queries on (default 32 768, 0 = never;
    // "order_bits": the key width, 10 .. 16, default 12 -- handle.cpp).
    const uint32_t order_min = (uint32_t)ix->knob.order_min, order_bits = (uint32_t)ix->knob.order_bits;
    ix->order_last = 0;
    if (!plain && nq >= order_min && order_min > 0 && w.dim >= 16u) {
        if ((rc = L.order.ensure((size_t)nq * 4))) return rc;
        if ((rc = L.order_hist.ensure((size_t)4 << 16))) return rc;
        HIP_TRY(launch_query_order(w.q, w.qstride, w.dim, nq, order_bits, L.order_hist.as<uint32_t>(), L.order.as<uint32_t>(), s));
        w.order = L.order.as<uint32_t>();
        ix->order_last = ix->order_perm_n = nq;   // (gbnns_index_order_last: this lane's permutation)
        ix->order_perm_lane = (int)(&L - ix->lanes);
    }
    if (prof) HIP_TRY(hipEventRecord(pc.ev[1], s));

    // ---- stage 2: beam walk -----------------------------------------------------------
    w.ell = ix->ell.as<uint32_t>(); w.ell_stride = ix->ell_stride; w.n = (uint32_t)ix->n; w.nq = nq;
    w.ef = ef; w.k = k; w.entries = entries_dev; w.n_entries = n_ent;
    w.cand = (!host && a->out_cand) ? a->out_cand : L.cand.as<uint32_t>();
    w.cand_dist = a->out_cand_dist ? (host ? L.cand_dist.as<float>() : a->out_cand_dist) : nullptr;
    w.cand_stride = cstride;
    w.zero_dist_bits = ix->metric == GBNNS_METRIC_NEG_DOT ? 0x80000000u : 0u;
    w.count = L.cnt.as<int32_t>();
    // (per-query counters into page-locked HOST memory are stored there directly, like the ids: written once per
    // query by the kernel that finishes it)
    int32_t* const hops_alias = host ? pinned_alias(a->out_hops, (size_t)nq * 4) : nullptr;
    int32_t* const dc_alias = host ? pinned_alias(a->out_dist_calc, (size_t)nq * 4) : nullptr;
    int32_t* const edges_alias = host ? pinned_alias(a->out_edges, (size_t)nq * 4) : nullptr;
    w.hops = host ? (hops_alias ? hops_alias : L.hops.as<int32_t>()) : (a->out_hops ? a->out_hops : L.hops.as<int32_t>());
    w.dist_calc = host ? (dc_alias ? dc_alias : L.dc.as<int32_t>()) : (a->out_dist_calc ? a->out_dist_calc : L.dc.as<int32_t>());
    w.edges = a->out_edges ? (host ? (edges_alias ? edges_alias : L.edges.as<int32_t>()) : a->out_edges) : nullptr;
    uint32_t* out_dev = host ? (ids_alias ? ids_alias : L.out.as<uint32_t>()) : a->out_ids;
    w.best = plain ? out_dev : nullptr;
    // Control words, two per-call blocks used alternately: [0] list A count, [1] general cursor,
    // [2] max dist_calc, [3] list B count, [4] retry cursor, [6] bitmap-pass cursor.  A call works on one block while its
    // general kernel (the last walk launch) clears the other for the next call -- no per-call memset
    // launch.  Word 5 of block 0 = general-kernel query total (persistent); words 8..71 = diagnostics.
    uint32_t* ctrl_base = L.ctrl.as<uint32_t>();
    const int cur = L.ctrl_phase;
    uint32_t* ctrl = ctrl_base + (cur ? 72 : 0);
    uint32_t* ctrl_next = ctrl_base + (cur ? 0 : 72);
    if (!L.ctrl_clean[cur]) {  // after a failed call only (word 5 of block 0 is the persistent general-kernel total)
        HIP_TRY(hipMemsetAsync(ctrl, 0, 20, s));
        HIP_TRY(hipMemsetAsync(ctrl + 6, 0, 4, s));
    }
    L.ctrl_clean[cur] = false;
    L.ctrl_phase = cur ^ 1;
    w.next_ctrl = ctrl_next;
    w.ovf_count = ctrl; w.g_cursor = ctrl + 1; w.max_dc = ctrl + 2; w.ovf2_count = ctrl + 3; w.r_cursor = ctrl + 4;
    w.g_total = ix->lanes[0].ctrl.as<uint32_t>() + 5; w.ovf_list = L.ovf_list.as<uint32_t>(); w.ovf2_list = L.ovf2_list.as<uint32_t>();
    w.g_bitmap = L.g_bitmap.as<uint32_t>(); w.g_keys = L.g_keys.as<uint64_t>();
    w.bitmap_words = bitmap_words;

    // Visited-set capacity.  The walk kernel's occupancy is LDS-bound, and a 10k-query batch is only
    // a few "rounds" deep (queries / (256 CUs x resident wavefronts)), so the table is sized from
    // the LDS budget: take the number of entries the walks need (first guess 43*ef; afterwards
    // 17/15 x the largest dist_calc of earlier batches, doubled whenever a batch handed queries
    // over), find how many wavefronts per CU that allows, then give each wavefront the whole
    // 160 KB / wavefronts share (capacity need not be a power of two: slot = mulhi(hash, cap)).
    g_slow.mark("stage1");
    if (L.stats_pending && hipEventQuery(L.stats_ev) == hipSuccess) {
        L.stats_pending = false;
        const uint32_t ovf = L.h_stats[0], maxdc = L.h_stats[2];
        {   // diagnostic (GBNNS_DEBUG_SIZING): what the first pass of that call handed over -- hand-overs stay exact but cost a retry pass
            static const bool dbg = getenv("GBNNS_DEBUG_SIZING") != nullptr;
            if (dbg && (ovf || L.h_stats[3]))
                std::fprintf(stderr, "[gbnns stats] key %d: first pass handed over %u queries, %u went on to the general kernel (longest walk %u, capacity %u)\n",
                             L.stats_ef, ovf, L.h_stats[3], maxdc, L.stats_cap);
        }
        // entries so that the largest walk seen (+ 1/16 margin + one pass of new ids) stays under the
        // 15/16 fill limit
        uint32_t need = (maxdc + maxdc / 16 + 64) / 15 * 16 + 16;
        // max_dc covers the retry / general passes too, so a hand-over needs no extra sizing rule
        uint32_t& seen = ix->maxdc_for_ef[L.stats_ef];
        seen = std::max(seen, maxdc);
        uint32_t& slot = ix->cap_for_ef[L.stats_ef];  // stats_ef = skey of that call
        const bool grew = need > slot;
        slot = std::max(slot, need);  // never shrinks: batches with one long walk do not make it oscillate
        // calm = the last observed batch of this (ef, mode) handed nothing over and did not move the size
        const bool quiet = ovf + L.h_stats[3] == 0 && !grew;
        int& streak = ix->calm_streak[L.stats_ef];
        streak = quiet ? std::min(streak + 1, 1 << 20) : 0;
    }
    w.force_wide = (a->flags & GBNNS_FLAG_WIDE_INDEX) ? 1 : 0;
    w.generic_only = ix->knob.hot ? 0 : 1;
    const bool aux = (a->flags & GBNNS_FLAG_AUX_GRAPH) != 0;
    if (tag) {  // gbnns_search_tagged: the walk of the graph cut to the rows each query may see (walk_tag.hip)
        w.tags = ix->tags.as<uint32_t>(); w.qtags = qtags_dev; w.tagged = 1;
        w.bridged = tag->bridge ? 1 : 0;  // (walk_bridge.hip)
    }
    // A byte handle (gbnns_index_create_bytes): the re-rank is fused only into the byte instances (walk_plan.cpp decides, from bytes_dim);
    // every other first pass runs as on a float handle with GBNNS_FLAG_NO_FUSED_RERANK, the stand-alone byte kernel behind it
    const bool bytes = ix->db_b != nullptr;
    if (bytes && !plain && !(a->flags & GBNNS_FLAG_NO_FUSED_RERANK) && rerank_plan(ix->metric, ix->d, true).fuses) w.bytes_dim = ix->d;
    // (a byte walk, GBNNS_FLAG_BYTE_WALK: a bit of its own too -- other kernels, no retry pass, and never the float handle's or the byte re-rank's state)
    // sizing statistics are kept per (ef, mode, aux, wide, byte instances: no retry pass behind them, half rows: another table, other walks; tagged: other graphs, shorter walks; bridged: two to three times the rows claimed; knob "hot" = 0: other kernels)
    const int skey = ((ef * 8 + a->mode * 2 + (aux ? 1 : 0)) * 2 + w.force_wide) | (w.half_rows ? 1 << 30 : 0) | (w.tagged ? 1 << 29 : 0) | (w.bridged ? 1 << 27 : 0) | (w.generic_only ? 1 << 28 : 0) | (w.bytes_dim ? 1 << 26 : 0) | (w.walk_bytes ? 1 << 25 : 0);
    const int calm = ix->calm_streak.count(skey) ? ix->calm_streak[skey] : 0;
    if (aux) {
        w.aux_ell = ix->aux_ell.as<uint32_t>(); w.aux_stride = ix->aux_stride;
        w.hops_bound = a->hops_bound; w.llf = (a->flags & GBNNS_FLAG_LLF) ? 1 : 0;
    }
    w.stamps = reinterpret_cast<unsigned long long*>(ctrl_base + 8);  // words 8..71, diagnostic builds
#ifdef GBNNS_STAMPS
    w.stamps_on = 1;
#endif
    // A small batch that runs ALONE (the reference's gist row: 1 000 queries per synchronous call, final_test.cpp:87) on the shapes that
    // have it: the two-wavefront walk (walk_coop.hip) -- a keeper wavefront with the result lists, a scout wavefront that expands the
    // predicted next node ahead.  One wavefront per query leaves such a launch a chain of dependent latencies on a mostly idle machine
    // (at most four queries per CU); measured on the gist shape at ef 200: first-pass kernel 0.487 against 0.526 ms.  NOT with batches in
    // flight: those fill the machine by themselves and are bound by bytes, and the second wavefront's issue slots and speculative rows
    // cost them (1.8 against 2.5 M queries/s).  Knob "coop": 0 never, 1 whenever the shape allows (tests), -1 this rule.
    // The first pass's instance and LDS layout (walk_plan.h); the instance depends on late / speculative rows, decided below: taken again then.
    const size_t cus = ix->cu_count();
    WalkPlan plan = plan_walk(w, ix->metric, WalkPass::First);
    {
        const int knob = ix->knob.coop;
        const bool in_flight = s == L.stream && L.stream != nullptr;
        if (knob != 0 && n_ent == 1 && !(a->flags & (GBNNS_FLAG_BITMAP_PASS | GBNNS_FLAG_WIDE_INDEX)) && plan.coop_serves &&
            (knob > 0 || (nq <= 4u * cus && !in_flight))) {
            w.coop = 1;
            plan = plan_walk(w, ix->metric, WalkPass::First);
        }
    }
    auto first_lds = [&] { return plan.lds_fixed + walk_hash_bytes(w.hash_cap, plan.hash_form(w.vs_shr)); };
    auto granules = [](size_t bytes) { return (bytes + kLdsGran - 1) / kLdsGran * kLdsGran; };
    // the first pass's visited set: capacity, form (packed / quotient), the wavefronts per CU it leaves (sizing.cpp)
    FirstPassSizing fps = size_first_pass(ix, w, plan, a, ef, skey, nq, sync_host);
    if (w.coop && ix->knob.coop < 0) {
        // (auto: only when every workgroup of the batch is resident at once -- LDS share per query, eight workgroups of two wavefronts per CU)
        const size_t per_wg = granules(first_lds());
        const size_t per_cu = std::min<size_t>(8, per_wg ? kMaxLds / per_wg : 0);
        if ((size_t)nq > per_cu * cus) {
            w.coop = 0;
            plan = plan_walk(w, ix->metric, WalkPass::First);
            fps = size_first_pass(ix, w, plan, a, ef, skey, nq, sync_host);
        }
    }
    const auto [auto_cap, form, cap] = fps;
    w.all_general = (first_lds() > kMaxLds || plan.general_only) ? 1 : 0;
    // Fused re-rank: with a register-list first pass (ef <= 512; and its retry / general successors) every
    // wavefront re-ranks its own query when its walk ends; no re-rank launch.  Needs the pair form
    // (d % 8 == 0) and room for the original-space query in the walk kernels' LDS.
    // Large ef: the visited table of such a walk would leave a handful of wavefronts per CU, so the first pass
    // keeps its visited sets as bitmaps in HBM and runs as many persistent wavefronts as the LDS holds result
    // lists (LDS-list kernel); taken when that at least doubles the resident wavefronts.
    size_t bitmap_per_cu = 0;
    WalkPlan bitmap_plan{};
    // (rerank_plan.h: the pair form; L2: d % 8 == 4 too -- glove's 300 -- its last 16-byte step is the even lane's alone)
    const bool want_fuse = bytes ? w.bytes_dim != 0u : (!plain && rerank_plan(ix->metric, ix->d, false).fuses && !(a->flags & GBNNS_FLAG_NO_FUSED_RERANK));
    w.rr_reserve = (want_fuse && !bytes) ? (uint32_t)ix->d_pad * 4u : 0u;  // (the bitmap pass has no byte instance)
    {
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
        const bool rows576 = w.dim == 144u && w.dstride == 144u && ix->metric == GBNNS_METRIC_L2;
        // (second half of round 5: for 576-byte rows the beam alone does not decide -- on a GD(M = 30) graph ef = 600 computes 10 500
        // distances per query, four wavefronts per CU by LDS, 21.4 ms on the table against 1.75 us per distance on the bitmap pass; the rule
        // below -- the pass must at least double the resident wavefronts: 8 by registers against <= 4 by the table -- does from ef 450 on)
        const int min_ef = min_ef_env ? min_ef_env : (rows576 ? 450 : (form == 2 ? 480 : 385));
        const bool forced = (a->flags & GBNNS_FLAG_BITMAP_PASS) != 0;  // diagnostic: whatever ef and batch size
        if (!w.all_general && !w.coop && !w.tagged && !w.walk_bytes && (ef >= min_ef || forced) && !(a->flags & GBNNS_FLAG_WIDE_INDEX) && (a->hash_capacity == 0 || forced)) {
            bitmap_plan = plan_walk(w, ix->metric, WalkPass::Bitmap);
            const size_t per_wave = granules(bitmap_plan.lds_fixed);   // (the slot counts below follow the device's CU count, as in sizing.cpp)
            const size_t per_cu = std::min<size_t>(rows576 ? 8 : 32, kMaxLds / per_wave);  // (576-byte rows: 223 registers, two wavefronts per SIMD)
            const size_t table_waves = std::min<size_t>(32, kMaxLds / granules(first_lds()));
            // ... and only when the batch is deeper than 1.5 rounds of the wavefronts the table would allow (a
            // 1 000-query batch is resident at once either way, and the register list is faster per hop)
            // ... or, short of that, when the table needs a second round and the bitmap pass holds the whole batch at once
            const bool one_round = (size_t)nq > table_waves * cus && (size_t)nq <= per_cu * cus;
            if (((per_cu >= 2 * std::max<size_t>(table_waves, 1) && (2 * (size_t)nq > 3 * table_waves * cus || one_round)) || forced) &&
                per_cu >= 1 && per_cu * cus * (size_t)bitmap_words * 4 <= (8ull << 30))
                bitmap_per_cu = per_cu;
        }
    }
    {
        // Two-list kernels over wide rows: rows after the visited test where the launch is bound by bandwidth -- 576-byte rows with at
        // least five wavefronts per CU by LDS (ef 300 / 400 / 600: 4.15 / 5.36 / 10.4 against 5.08 / 6.74 / 10.7 ms; ef 800 / 1 000, four and
        // fewer per CU: 18.2 / 23.8 against 17.4 / 22.3) on a batch that fills the machine
        const int knob = ix->knob.late_rows;
        const size_t per_wave = granules(first_lds());
        const size_t lds_waves = per_wave ? kMaxLds / per_wave : 0;
        // ... and 192-byte rows at ef <= 64 (walk_reg_wide_kernel<12>, the reference's deep 96 -> 48: 2.24 GB moved for 1.62 GB of
        // algorithmic bytes at ef = 40, 6.5 TB/s; 0.351 -> 0.342 ms alone, 29.4 -> 30.9 M queries/s in flight; its longer beams: no gain)
        const bool l2 = ix->metric == GBNNS_METRIC_L2 && w.dim == w.dstride && nq >= 2048u;
        // ... and the 384- / 512-byte rows of PLAIN walks over deep / sift vectors at beams of more than 128 (2.15 -> 2.08 ms at d = 128,
        // ef = 140; 1.63 -> 1.52 ms at d = 96, ef = 160)
        const bool big_rows = w.dim == 144u || ((w.dim == 96u || w.dim == 128u) && ef > 128);
        const bool auto_late = l2 && ((big_rows && lds_waves >= 5) || (w.dim == 48u && ef <= 64));
        // (the bitmap pass over 576-byte rows: always -- 8 wavefronts per CU whatever the beam)
        const bool bitmap_late = bitmap_per_cu != 0 && w.dim == 144u && l2;
        w.late_rows = knob < 0 ? ((auto_late || bitmap_late) ? 1 : 0) : knob;
    }
    plan = plan_walk(w, ix->metric, WalkPass::First);
    if (bitmap_per_cu) bitmap_plan = plan_walk(w, ix->metric, WalkPass::Bitmap);
    const WalkPlan& first = bitmap_per_cu ? bitmap_plan : plan;
    // (the two-list instances keep their result list in LDS and stage the re-rank query in the visited-set area)
    const size_t rr_room = first.rr_room(walk_hash_bytes(w.hash_cap, first.hash_form(w.vs_shr)));
    const bool fuse = !first.lds_list && want_fuse && !w.all_general && (size_t)ix->d_pad * 4 <= rr_room && (!bytes || first.inst.bytes);
    if (fuse) {
        // (a byte instance: rr_db_b, rows of d_pad bytes; rr_db stays nullptr)
        w.rr_q = q_dev; w.rr_qstride = ix->d; w.rr_db = ix->db; w.rr_db_b = ix->db_b; w.rr_dstride = ix->d_pad; w.rr_dim = ix->d;
        w.rr_n = (uint32_t)ix->n; w.rr_out = out_dev; w.rr_metric = ix->metric;
    }

    // Once batches of this (ef, mode) have been calm (no hand-over, size settled), the retry launch is left
    // out: the first pass then appends what it cannot finish to list B directly and the general kernel --
    // always launched -- takes it.  Still exact; a surprise hand-over is just slower once, and un-calms.
    const bool skip_retry = auto_cap && calm >= 2 && !w.all_general;
    if (skip_retry) {
        w.ovf_count = w.ovf2_count;
        w.ovf_list = w.ovf2_list;
    }
    bool bitmap_pass = false;
    const char* retry_planned = nullptr;  // the retry instance this call launched (profiling)
    if (bitmap_per_cu) {
        if ((rc = L.fp_bitmap.ensure(bitmap_per_cu * cus * (size_t)bitmap_words * 4))) return rc;
        w.fp_bitmap = L.fp_bitmap.as<uint32_t>();
        w.fp_cursor = ctrl + 6;
        HIP_TRY(launch_walk(bitmap_plan, w, (unsigned)(bitmap_per_cu * cus), s));
        bitmap_pass = true;
    }
    if (!w.all_general) {
        if (!bitmap_pass) HIP_TRY(launch_walk(plan, w, 0, s));
        // retry pass: hand-overs of the first pass, one wavefront per CU with all the LDS
        WalkParams w2 = w;
        w2.vs_shr = 0;  // (the retry kernels keep the packed form)
        w2.coop = 0;    // (... and one wavefront per query)
        const WalkPlan retry = plan_walk(w2, ix->metric, WalkPass::Retry);
        w2.hash_cap = walk_hash_entries(kMaxLds / kLdsGran * kLdsGran - retry.lds_fixed, retry.hash_form(0));
        w2.hash_limit = w2.hash_cap - w2.hash_cap / 16;
        if (skip_retry) {
            // nothing to launch
        } else if (w2.hash_cap > cap && !w.tagged && !w.rr_db_b && !w.walk_bytes) {  // (a tagged first pass has no retry pass: its hand-overs go straight to the general kernel; a byte instance's and a byte walk's to the general kernel's byte instances)
            HIP_TRY(launch_walk(retry, w2, 0, s));
            if (prof) retry_planned = walk_plan_name(retry);
        } else {
            HIP_TRY(hipMemcpyAsync(ctrl + 3, ctrl, 4, hipMemcpyDeviceToDevice, s));  // nothing to gain: A -> B
            HIP_TRY(hipMemcpyAsync(w.ovf2_list, w.ovf_list, (size_t)nq * 4, hipMemcpyDeviceToDevice, s));
        }
    }
    if (prof) {
        HIP_TRY(hipEventRecord(pc.ev[2], s));
        // name of the first-pass kernel of this call, template arguments included ("walk_general_kernel" when there was none)
        auto printable = [](const char* mangled) {  // drop "void gbnns::(anonymous namespace)::" and the parameter list
            int st = 0;
            char* dm = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
            std::string name = (st == 0 && dm) ? dm : mangled;
            std::free(dm);
            size_t pos = name.find("walk_");
            if (pos == std::string::npos) pos = name.find("beam_");  // (the integer byte-walk instances, walk_bytes_q.hip)
            if (pos != std::string::npos) name = name.substr(pos);
            pos = name.rfind("(gbnns::WalkParams)");
            if (pos != std::string::npos) name = name.substr(0, pos);
            return name;
        };
        const char* mangled = w.all_general ? nullptr : walk_first_pass_name(s);
        std::string name = "walk_general_kernel";  // (a tagged call: its tagged instance, walk_general_tag_kernel -- one name for both, gbnns.h)
        if (mangled) {
            name = printable(mangled);
            const char* planned = walk_plan_name(first);
            if (!planned || name != planned)
                return fail(GBNNS_ERR_INTERNAL, "first pass: planned %s, launched %s", planned ? planned : "(none)", name.c_str());
        }
        std::snprintf(ix->acc.walk_kernel, sizeof(ix->acc.walk_kernel), "%s", name.c_str());
        // ... and of its retry-pass kernel (empty: none launched)
        std::string retry_name;
        if (retry_planned) {
            const char* rm = walk_retry_pass_name(s);
            retry_name = rm ? printable(rm) : "(none)";
            if (retry_name != retry_planned)
                return fail(GBNNS_ERR_INTERNAL, "retry pass: planned %s, launched %s", retry_planned, retry_name.c_str());
        }
        std::snprintf(ix->acc.retry_kernel, sizeof(ix->acc.retry_kernel), "%s", retry_name.c_str());
    }
    g_slow.mark("walk");
    HIP_TRY(launch_walk_general(w, ix->metric, s));
    g_slow.mark("general");
    L.ctrl_clean[cur ^ 1] = true;  // cleared by that launch
    if (prof) HIP_TRY(hipEventRecord(pc.ev[3], s));
    // statistics of this call (hand-over counts, largest walk), read back asynchronously: every call until
    // things are calm, every 16th afterwards (each read is a small copy on the stream)
    // (a bridged call: every call -- the length of its walks follows the allowed fraction of the batch, and what a table sized for another
    // fraction hands over runs on the general kernel: 10 000 queries at sift ef 64 took it 2 s)
    ix->stats_tick += 1;
    if (auto_cap && !w.all_general && !L.stats_pending && (calm < 4 || (ix->stats_tick & 15u) == 0 || w.bridged)) {
        if (!L.h_stats) {
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&L.h_stats), 16, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&L.stats_ev, hipEventDisableTiming));
        }
        HIP_TRY(hipMemcpyAsync(L.h_stats, ctrl, 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(L.stats_ev, s));
        L.stats_pending = true;
        L.stats_ef = skey;
        L.stats_cap = cap;
    }

    g_slow.mark("stats");
    // ---- stage 3: re-rank in the original space ------------------------------------------
    if (!plain && !fuse) {
        RerankParams r{};
        r.q = q_dev; r.qstride = ix->d; r.db = ix->db; r.dstride = ix->d_pad; r.dim = ix->d;
        r.cand = w.cand; r.cand_stride = cstride; r.count = w.count; r.nq = nq; r.n = (uint32_t)ix->n; r.out = out_dev;
        HIP_TRY(rerank_launch(ix, r, s));
    }
    // ... and the k best of the same candidates (gbnns_search_topk): every first pass, the retry pass and the general kernel leave the
    // candidate row and its count behind, whether they re-ranked their query themselves or not
    RerankTopkParams tk{};
    if (topk) {
        tk.q = q_dev; tk.qstride = ix->d; tk.db = ix->db; tk.dstride = ix->d_pad; tk.dim = ix->d;
        tk.cand = w.cand; tk.cand_stride = cstride; tk.count = w.count; tk.nq = nq; tk.n = (uint32_t)ix->n;
        tk.k = (uint32_t)topk->k;
        tk.out = host ? L.top_ids.as<uint32_t>() : topk->ids;
        tk.out_dist = topk->dist ? (host ? L.top_dist.as<float>() : topk->dist) : nullptr;
        HIP_TRY(rerank_topk_launch(ix, tk, s));
    }
    if (prof) {
        HIP_TRY(hipEventRecord(pc.ev[4], s));
        ix->pending.push_back(pc);
        // hand-over counts of this call for gbnns_profile_read, behind the timed stages: this call's control block stays as it is until a
        // later call's general kernel clears it
        if (!ix->prof_ctrl) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ix->prof_ctrl), 16, hipHostMallocDefault));
        HIP_TRY(hipMemcpyAsync(ix->prof_ctrl, ctrl, 16, hipMemcpyDeviceToHost, s));
        ix->prof_ctrl_pending = true;
        ix->prof_ctrl_direct = skip_retry;
    }

    // ---- outputs ----------------------------------------------------------------------
    if (host) {
        // (pageable buffers: through the lane's staging buffer, each copy complete on return -- host_copy_out)
        const size_t b4 = (size_t)nq * 4, bc = (size_t)nq * cstride * 4;
        if (!ids_alias && (rc = host_copy_out(L, a->out_ids, out_dev, b4, b4, 1, s))) return rc;
        if (a->out_hops && !hops_alias && (rc = host_copy_out(L, a->out_hops, w.hops, b4, b4, 1, s))) return rc;
        if (a->out_dist_calc && !dc_alias && (rc = host_copy_out(L, a->out_dist_calc, w.dist_calc, b4, b4, 1, s))) return rc;
        if (a->out_edges && !edges_alias && (rc = host_copy_out(L, a->out_edges, w.edges, b4, b4, 1, s))) return rc;
        if (a->out_cand && (rc = host_copy_out(L, a->out_cand, w.cand, bc, bc, 1, s))) return rc;
        if (a->out_cand_dist && (rc = host_copy_out(L, a->out_cand_dist, w.cand_dist, bc, bc, 1, s))) return rc;
        if (topk) {
            const size_t bk = (size_t)nq * topk->k * 4;
            if ((rc = host_copy_out(L, topk->ids, tk.out, bk, bk, 1, s))) return rc;
            if (topk->dist && (rc = host_copy_out(L, topk->dist, tk.out_dist, bk, bk, 1, s))) return rc;
        }
        g_slow.mark("copy_out");
        if (sync_host) {
            HIP_TRY(hipStreamSynchronize(s));
            ix->in_flight = false;
        }
    }
    return GBNNS_OK;
}


}  // namespace gbnns_api
