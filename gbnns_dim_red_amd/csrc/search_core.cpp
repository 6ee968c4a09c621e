// search_core.cpp -- one batch on one lane, as a sequence of stages over one per-call context: workspaces, copies in, the queries in the walked
// space, the statistics of earlier calls, the call's plan (call_plan.cpp: pure), the walk launches the plan names (-> general kernel), statistics
// read-back, re-rank, copies out.  Cut out of api.cpp in round 5; the sizing rule the plan calls is in sizing.cpp.

#include "api_internal.h"

using namespace gbnns;
using namespace gbnns_api;

namespace gbnns_api {

namespace {

// One call's context: the arguments, what they imply, and what each stage leaves for the later ones.
struct Call {
    gbnns_index* ix;
    Lane& L;
    const gbnns_search_args* a;
    hipStream_t s;
    bool sync_host;
    const TopkOut* topk;
    const TagIn* tag;
    const uint8_t* q_u8;
    // from the arguments
    uint32_t n_ent, nq, cstride;
    bool host, plain, prof;
    int ef, k;
    // workspace
    uint32_t bitmap_words;
    uint32_t* ids_alias;
    // inputs
    const float* q_dev;
    const uint8_t* qb_dev;
    const uint32_t* entries_dev;
    const uint32_t* qtags_dev;
    ProfCall pc;
    // stage 1 on
    WalkParams w;
    int32_t *hops_alias, *dc_alias, *edges_alias;
    uint32_t* out_dev;
    CallFacts facts;
    CallPlan plan;
    uint32_t* ctrl;                // this call's block of control words
    int cur;                       // ... and which of the two it is
    const char* retry_planned;     // the retry instance this call launched (profiling)
    RerankTopkParams tk;
    // the stages, in the order search_core runs them
    int workspace();
    int inputs();
    CallFacts call_facts() const;
    int project();
    void absorb_stats();
    int walk_params();
    int walk();
    int profile_names();
    int general_and_stats();
    int rerank();
    int outputs();
};

int Call::workspace() {
    int rc;
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
    ids_alias = host ? pinned_alias(a->out_ids, (size_t)nq * 4) : nullptr;
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
    bitmap_words = bitmap_words_of(ix->n);  // per slot
    {
        const size_t before = L.g_bitmap.bytes;  // (re)allocation always changes the size
        if ((rc = L.g_bitmap.ensure((size_t)kGeneralSlots * 2 * bitmap_words * 4))) return rc;
        // the tie bits must start out all zero (the kernel keeps them so); the visited bits are cleared per query
        if (L.g_bitmap.bytes != before) HIP_TRY(hipMemsetAsync(L.g_bitmap.p, 0, L.g_bitmap.bytes, s));
    }
    if ((rc = L.g_keys.ensure((size_t)kGeneralSlots * ((size_t)ef + n_ent - 1) * 8))) return rc;
    g_slow.mark("workspace");
    return GBNNS_OK;
}

int Call::inputs() {
    int rc;
    q_dev = a->queries;
    qb_dev = q_u8;
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
    entries_dev = a->entry_ids;
    if (a->entry_ids && host) {
        if ((rc = L.entries.ensure((size_t)nq * n_ent * 4))) return rc;
        if ((rc = host_copy_in(L, L.entries.p, a->entry_ids, (size_t)nq * n_ent * 4, s))) return rc;
        entries_dev = L.entries.as<uint32_t>();
        // (a tagged call: an entry the query cannot start from is data, HOST and DEVICE buffers alike -- the kernels write its empty row)
        for (size_t i = 0; i < (size_t)nq * n_ent && !tag; ++i)
            if (a->entry_ids[i] >= ix->n) return fail(GBNNS_ERR_INVALID, "entry id %u >= n", a->entry_ids[i]);
    }
    qtags_dev = tag ? tag->qtags : nullptr;
    if (tag && host) {
        if ((rc = L.qtags.ensure((size_t)nq * 4))) return rc;
        if ((rc = host_copy_in(L, L.qtags.p, tag->qtags, (size_t)nq * 4, s))) return rc;
        qtags_dev = L.qtags.as<uint32_t>();
    }
    g_slow.mark("copy_in");
    if (prof) {
        for (int i = 0; i < 5; ++i) HIP_TRY(hipEventCreate(&pc.ev[i]));
        pc.queries = nq;
        HIP_TRY(hipEventRecord(pc.ev[0], s));
    }
    return GBNNS_OK;
}

// What the plan reads of this call (call_plan.h); the walked space follows from the mode.
CallFacts Call::call_facts() const {
    CallFacts f{};
    f.metric = ix->metric; f.n = ix->n; f.d = ix->d; f.d_pad = ix->d_pad; f.ell_stride = ix->ell_stride;
    f.aux_stride = (a->flags & GBNNS_FLAG_AUX_GRAPH) ? ix->aux_stride : 0u;
    f.rows = ix->rows; f.cus = ix->cu_count(); f.knob = ix->knob;
    f.dim = plain ? ix->d : ix->d_low; f.dstride = plain ? ix->d_pad : ix->dl_pad;
    f.half_rows = !plain && (a->flags & GBNNS_FLAG_HALF_ROWS);
    // a PLAIN call walks the handle's own rows, d_pad elements each, whatever their kind (GBNNS_FLAG_BYTE_WALK / GBNNS_FLAG_HALF_WALK: checked by
    // search_call; no float copy of such a table exists); NET / LOWQ walk db_low, which is float32
    f.walked = plain ? ix->rows : RowKind::F32;
    f.byte_queries = q_u8 != nullptr;
    f.mode = a->mode; f.ef = ef; f.n_entries = n_ent; f.flags = a->flags; f.hash_capacity = a->hash_capacity; f.nq = nq;
    f.tagged = tag != nullptr; f.bridged = tag && tag->bridge;
    f.in_flight = s == L.stream && L.stream != nullptr;
    f.sync_host = sync_host;
#ifdef GBNNS_STAMPS
    f.stamps_on = true;
#endif
    return f;
}

// stage 1: queries in the walked space
int Call::project() {
    int rc;
    set_walk_shape(w, facts);
    if (q_u8) HIP_TRY(launch_widen_u8(qb_dev, L.q_in.as<float>(), (size_t)nq * ix->d, s));
    if (plain) {
        w.q = q_dev; w.qstride = ix->d;
        set_walked_table(w, facts.walked, ix->base);
        w.q_b = w.walk_bytes ? qb_dev : nullptr;
    } else {
        if ((rc = L.q_low.ensure((size_t)nq * ix->dl_pad * 4))) return rc;
        float* ql = L.q_low.as<float>();
        if (a->mode == GBNNS_MODE_NET) {
            if ((rc = run_project(ix, L, q_dev, ix->d, nq, ql, s, facts.in_flight, (a->flags & GBNNS_FLAG_MFMA_PROJECTION) != 0))) return rc;
            w.q = ql; w.qstride = ix->dl_pad;
        } else if (host) {
            if ((rc = host_copy_in(L, ql, a->queries_low, (size_t)nq * ix->d_low * 4, s))) return rc;
            w.q = ql; w.qstride = ix->d_low;
        } else {
            w.q = a->queries_low; w.qstride = ix->d_low;
        }
        w.db = ix->db_low;
        if (w.half_rows) {
            // the walked table is R = float32(float16(db_low)): every kernel reads its float32 copy, in db_low's layout, but the half
            // instances of the first pass (walk_plan.cpp), whose hops gather the 2-byte rows
            w.db = ix->low_r.as<float>(); w.db_h = ix->low_half.p;
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
    g_slow.mark("stage1");
    return GBNNS_OK;
}

// The statistics an earlier call of this lane left, once they have arrived, folded into the handle's sizing history -- before the plan reads it.
// Visited-set capacity.  The walk kernel's occupancy is LDS-bound, and a 10k-query batch is only
// a few "rounds" deep (queries / (256 CUs x resident wavefronts)), so the table is sized from
// the LDS budget: take the number of entries the walks need (first guess 43*ef; afterwards
// 17/15 x the largest dist_calc of earlier batches, doubled whenever a batch handed queries
// over), find how many wavefronts per CU that allows, then give each wavefront the whole
// 160 KB / wavefronts share (capacity need not be a power of two: slot = mulhi(hash, cap)).
void Call::absorb_stats() {
    SizingHistory& h = ix->history;
    if (!L.stats_pending || hipEventQuery(L.stats_ev) != hipSuccess) return;
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
    uint32_t& seen = h.maxdc_for_ef[L.stats_ef];
    seen = std::max(seen, maxdc);
    uint32_t& slot = h.cap_for_ef[L.stats_ef];  // stats_ef = skey of that call
    const bool grew = need > slot;
    slot = std::max(slot, need);  // never shrinks: batches with one long walk do not make it oscillate
    // calm = the last observed batch of this (ef, mode) handed nothing over and did not move the size
    const bool quiet = ovf + L.h_stats[3] == 0 && !grew;
    int& streak = h.calm_streak[L.stats_ef];
    streak = quiet ? std::min(streak + 1, 1 << 20) : 0;
}

// stage 2, before its launches: the call's parameters -- outputs, control words, workspaces, and the plan's decisions
int Call::walk_params() {
    plan.apply(w);
    w.ell = ix->ell.as<uint32_t>(); w.k = k; w.entries = entries_dev;
    w.cand = (!host && a->out_cand) ? a->out_cand : L.cand.as<uint32_t>();
    w.cand_dist = a->out_cand_dist ? (host ? L.cand_dist.as<float>() : a->out_cand_dist) : nullptr;
    w.cand_stride = cstride;
    w.zero_dist_bits = ix->metric == GBNNS_METRIC_NEG_DOT ? 0x80000000u : 0u;
    w.count = L.cnt.as<int32_t>();
    // (per-query counters into page-locked HOST memory are stored there directly, like the ids: written once per
    // query by the kernel that finishes it)
    hops_alias = host ? pinned_alias(a->out_hops, (size_t)nq * 4) : nullptr;
    dc_alias = host ? pinned_alias(a->out_dist_calc, (size_t)nq * 4) : nullptr;
    edges_alias = host ? pinned_alias(a->out_edges, (size_t)nq * 4) : nullptr;
    w.hops = host ? (hops_alias ? hops_alias : L.hops.as<int32_t>()) : (a->out_hops ? a->out_hops : L.hops.as<int32_t>());
    w.dist_calc = host ? (dc_alias ? dc_alias : L.dc.as<int32_t>()) : (a->out_dist_calc ? a->out_dist_calc : L.dc.as<int32_t>());
    w.edges = a->out_edges ? (host ? (edges_alias ? edges_alias : L.edges.as<int32_t>()) : a->out_edges) : nullptr;
    out_dev = host ? (ids_alias ? ids_alias : L.out.as<uint32_t>()) : a->out_ids;
    w.best = plain ? out_dev : nullptr;
    // Control words, two per-call blocks used alternately: [0] list A count, [1] general cursor,
    // [2] max dist_calc, [3] list B count, [4] retry cursor, [6] bitmap-pass cursor.  A call works on one block while its
    // general kernel (the last walk launch) clears the other for the next call -- no per-call memset
    // launch.  Word 5 of block 0 = general-kernel query total (persistent); words 8..71 = diagnostics.
    uint32_t* ctrl_base = L.ctrl.as<uint32_t>();
    cur = L.ctrl_phase;
    ctrl = ctrl_base + (cur ? 72 : 0);
    if (!L.ctrl_clean[cur]) {  // after a failed call only (word 5 of block 0 is the persistent general-kernel total)
        HIP_TRY(hipMemsetAsync(ctrl, 0, 20, s));
        HIP_TRY(hipMemsetAsync(ctrl + 6, 0, 4, s));
    }
    L.ctrl_clean[cur] = false;
    L.ctrl_phase = cur ^ 1;
    w.next_ctrl = ctrl_base + (cur ? 0 : 72);
    w.ovf_count = ctrl; w.g_cursor = ctrl + 1; w.max_dc = ctrl + 2; w.ovf2_count = ctrl + 3; w.r_cursor = ctrl + 4;
    w.g_total = ix->lanes[0].ctrl.as<uint32_t>() + 5; w.ovf_list = L.ovf_list.as<uint32_t>(); w.ovf2_list = L.ovf2_list.as<uint32_t>();
    w.g_bitmap = L.g_bitmap.as<uint32_t>(); w.g_keys = L.g_keys.as<uint64_t>();
    w.bitmap_words = bitmap_words;
    if (tag) {  // gbnns_search_tagged: the walk of the graph cut to the rows each query may see (walk_tag.hip; bridged: walk_bridge.hip)
        w.tags = ix->tags.as<uint32_t>(); w.qtags = qtags_dev;
    }
    if (w.aux_ell) {
        w.aux_ell = ix->aux_ell.as<uint32_t>();
        w.hops_bound = a->hops_bound; w.llf = (a->flags & GBNNS_FLAG_LLF) ? 1 : 0;
    }
    w.stamps = reinterpret_cast<unsigned long long*>(ctrl_base + 8);  // words 8..71, diagnostic builds
    if (plan.fuse) {
        // (a byte instance: rr_db_b, rows of d_pad bytes; rr_db stays nullptr)
        set_fused_rerank_table(w, ix->rows, ix->base);
        w.rr_q = q_dev; w.rr_qstride = ix->d; w.rr_dstride = ix->d_pad; w.rr_dim = ix->d;
        w.rr_n = (uint32_t)ix->n; w.rr_out = out_dev; w.rr_metric = ix->metric;
    }
    if (plan.skip_retry) {  // the first pass appends what it cannot finish to list B directly
        w.ovf_count = w.ovf2_count;
        w.ovf_list = w.ovf2_list;
    }
    if (plan.bitmap_pass) {
        int rc;
        if ((rc = L.fp_bitmap.ensure(plan.bitmap_per_cu * facts.cus * (size_t)bitmap_words * 4))) return rc;
        w.fp_bitmap = L.fp_bitmap.as<uint32_t>();
        w.fp_cursor = ctrl + 6;
    }
    return GBNNS_OK;
}

// stage 2: the first pass and what the plan names for its hand-overs
int Call::walk() {
    const CallPlan& p = plan;
    retry_planned = nullptr;
    if (p.bitmap_pass) HIP_TRY(launch_walk(p.first, w, (unsigned)(p.bitmap_per_cu * facts.cus), s));
    else if (!p.all_general) HIP_TRY(launch_walk(p.first, w, 0, s));
    if (p.retry_action == RetryAction::Launch) {
        WalkParams w2 = w;
        w2.vs_shr = 0;  // (the retry kernels keep the packed form)
        w2.coop = 0;    // (... and one wavefront per query)
        w2.hash_cap = p.retry_hash_cap;
        w2.hash_limit = p.retry_hash_limit;
        HIP_TRY(launch_walk(p.retry, w2, 0, s));
        if (prof) retry_planned = walk_plan_name(p.retry);
    } else if (p.retry_action == RetryAction::Copy) {
        HIP_TRY(hipMemcpyAsync(ctrl + 3, ctrl, 4, hipMemcpyDeviceToDevice, s));  // nothing to gain: A -> B
        HIP_TRY(hipMemcpyAsync(w.ovf2_list, w.ovf_list, (size_t)nq * 4, hipMemcpyDeviceToDevice, s));
    }
    return GBNNS_OK;
}

// the profile's names of this call's walk kernels, each checked against the plan's
int Call::profile_names() {
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
    const char* mangled = plan.all_general ? nullptr : walk_first_pass_name(s);
    std::string name = "walk_general_kernel";  // (a tagged call: its tagged instance, walk_general_tag_kernel -- one name for both, gbnns.h)
    if (mangled) {
        name = printable(mangled);
        const char* planned = walk_plan_name(plan.first);
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
    return GBNNS_OK;
}

// the general kernel -- always launched -- and the read-back of this call's statistics
int Call::general_and_stats() {
    HIP_TRY(launch_walk_general(w, ix->metric, s));
    g_slow.mark("general");
    L.ctrl_clean[cur ^ 1] = true;  // cleared by that launch
    if (prof) HIP_TRY(hipEventRecord(pc.ev[3], s));
    // statistics of this call (hand-over counts, largest walk), read back asynchronously: every call until
    // things are calm, every 16th afterwards (each read is a small copy on the stream)
    // (a bridged call: every call -- the length of its walks follows the allowed fraction of the batch, and what a table sized for another
    // fraction hands over runs on the general kernel: 10 000 queries at sift ef 64 took it 2 s)
    ix->stats_tick += 1;
    const int calm = ix->history.calm(plan.skey);
    if (plan.sizing.auto_cap && !plan.all_general && !L.stats_pending && (calm < 4 || (ix->stats_tick & 15u) == 0 || w.bridged)) {
        if (!L.h_stats) {
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&L.h_stats), 16, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&L.stats_ev, hipEventDisableTiming));
        }
        HIP_TRY(hipMemcpyAsync(L.h_stats, ctrl, 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(L.stats_ev, s));
        L.stats_pending = true;
        L.stats_ef = plan.skey;
        L.stats_cap = plan.sizing.cap;
    }
    g_slow.mark("stats");
    return GBNNS_OK;
}

// stage 3: re-rank in the original space
int Call::rerank() {
    if (!plain && !plan.fuse) {
        RerankParams r{};
        r.q = q_dev; r.qstride = ix->d; r.dstride = ix->d_pad; r.dim = ix->d;
        r.cand = w.cand; r.cand_stride = cstride; r.count = w.count; r.nq = nq; r.n = (uint32_t)ix->n; r.out = out_dev;
        HIP_TRY(rerank_launch(ix, r, s));
    }
    // ... and the k best of the same candidates (gbnns_search_topk): every first pass, the retry pass and the general kernel leave the
    // candidate row and its count behind, whether they re-ranked their query themselves or not
    if (topk) {
        tk.q = q_dev; tk.qstride = ix->d; tk.dstride = ix->d_pad; tk.dim = ix->d;
        tk.cand = w.cand; tk.cand_stride = cstride; tk.count = w.count; tk.nq = nq; tk.n = (uint32_t)ix->n;
        tk.k = (uint32_t)topk->k;
        tk.out = host ? L.top_ids.as<uint32_t>() : topk->ids;
        tk.out_dist = topk->dist ? (host ? L.top_dist.as<float>() : topk->dist) : nullptr;
        HIP_TRY(rerank_launch(ix, tk, s));
    }
    if (prof) {
        HIP_TRY(hipEventRecord(pc.ev[4], s));
        ix->pending.push_back(pc);
        // hand-over counts of this call for gbnns_profile_read, behind the timed stages: this call's control block stays as it is until a
        // later call's general kernel clears it
        if (!ix->prof_ctrl) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ix->prof_ctrl), 16, hipHostMallocDefault));
        HIP_TRY(hipMemcpyAsync(ix->prof_ctrl, ctrl, 16, hipMemcpyDeviceToHost, s));
        ix->prof_ctrl_pending = true;
        ix->prof_ctrl_direct = plan.skip_retry;
    }
    return GBNNS_OK;
}

int Call::outputs() {
    if (!host) return GBNNS_OK;
    int rc;
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
    return GBNNS_OK;
}

}  // namespace

// One (sub-)batch on one lane's workspace, enqueued on stream s; arguments validated by gbnns_search_ex.  With HOST
// buffers the copies in and out are enqueued on s too and, when sync_host, waited for.  `topk` (optional, NET / LOWQ): the k best of
// each query's candidates go to its arrays as well (rerank_topk kernels, behind stage 3).
// `q_u8` (gbnns_search_byte_queries; a->queries is then nullptr): the queries as [n_q x d] bytes, a buffer of a->mem_kind.  They are widened
// into the lane's q_in (widen.hip) and that copy takes a->queries' place everywhere below; the bytes themselves reach the walk as
// WalkParams::q_b, for the integer byte-walk instances.
int search_core(gbnns_index* ix, Lane& L, const gbnns_search_args* a, hipStream_t s, bool sync_host, const TopkOut* topk, const TagIn* tag, const uint8_t* q_u8) {
    int rc;
    Call c{ix, L, a, s, sync_host, topk, tag, q_u8};
    c.n_ent = a->n_entries ? a->n_entries : 1u;
    c.host = a->mem_kind == GBNNS_MEM_HOST;
    c.nq = (uint32_t)a->n_q;
    c.ef = a->ef;
    c.plain = a->mode == GBNNS_MODE_PLAIN;
    c.k = c.plain ? std::max(1, std::min(a->k > 0 ? a->k : 1, c.ef)) : c.ef;
    c.cstride = (uint32_t)c.k;
    c.prof = ix->profiling;
    c.facts = c.call_facts();
    if ((rc = c.workspace())) return rc;
    if ((rc = c.inputs())) return rc;
    if ((rc = c.project())) return rc;
    c.absorb_stats();  // (before the plan reads the history)
    c.plan = call_plan(c.facts, ix->history);
    if ((rc = c.walk_params())) return rc;
    if ((rc = c.walk())) return rc;
    if (c.prof && (rc = c.profile_names())) return rc;
    g_slow.mark("walk");
    if ((rc = c.general_and_stats())) return rc;
    if ((rc = c.rerank())) return rc;
    return c.outputs();
}

}  // namespace gbnns_api
