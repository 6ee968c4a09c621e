// lanes.cpp -- gbnns_search_ex / gbnns_search_topk and the batches-in-flight machinery: lanes (workspace + internal stream + done events), the fork /
// join events between the caller's stream and the lanes, gbnns_index_wait / _join, gbnns_search_batch.  Cut out of api.cpp in round 5.
// Also gbnns_index_tag_census and gbnns_search_tagged_auto (census, then per query the tagged walk or the exact scan): they run on lane 0
// in the caller's stream like a plain search call; their kernels are tag_census.hip's.

#include "api_internal.h"

using namespace gbnns;
using namespace gbnns_api;

namespace gbnns_api {

// A handle's workspace (projected queries, candidate lists, hand-over lists, control words) is shared by its
// calls and ordered by stream order.  When a call names another stream than the last one that left work in
// flight, the new stream first waits for that work (an event recorded on the old stream now covers everything
// enqueued there so far).  Should the old stream be gone, the device is synchronised instead.
int enter_stream(gbnns_index* ix, hipStream_t s) {
    int rc = flush_join(ix);  // deferred calls not yet joined: their streams first wait for their lanes
    if (rc) return rc;
    if (ix->in_flight && ix->last_stream != s) {
        hipError_t e = hipSuccess;
        if (!ix->order_ev) e = hipEventCreateWithFlags(&ix->order_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ix->order_ev, ix->last_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ix->order_ev, 0);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(hipDeviceSynchronize());
        }
    }
    ix->last_stream = s;
    ix->in_flight = true;
    return GBNNS_OK;
}

int ensure_lane(gbnns_index* ix, int i) {
    Lane& L = ix->lanes[i];
    if (!L.stream) HIP_TRY(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    if (!L.done_ev) HIP_TRY(hipEventCreateWithFlags(&L.done_ev, hipEventDisableTiming));
    if (!L.prev_ev) HIP_TRY(hipEventCreateWithFlags(&L.prev_ev, hipEventDisableTiming));
    if (!L.ctrl_ready) {
        int rc = L.ctrl.ensure(512);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(L.ctrl.p, 0, 512, L.stream));  // in the lane's stream order: first use follows it
        L.ctrl_ready = true;
    }
    return GBNNS_OK;
}

void plan_call(gbnns_index* ix, const gbnns_search_args* a, int& lanes, int& lane) {
    lanes = 1;
    lane = 0;
#ifdef GBNNS_STAMPS
    return;
#endif
    if ((a->flags & GBNNS_FLAG_SERIAL) || ix->profiling) return;
    if (!(a->flags & GBNNS_FLAG_DEFER_JOIN)) return;  // (HOST buffers: page-locked, checked by gbnns_search_ex)
    lanes = a->defer_depth ? (int)std::min<uint32_t>(std::max<uint32_t>(a->defer_depth, 2u), (uint32_t)kMaxLanes) : 3;  // measured best: 3
    lane = ix->next_lane % lanes;
    ix->next_lane = (lane + 1) % lanes;
}

// The callers' streams wait for deferred calls, oldest first, until at most `keep` of them remain unjoined.
int flush_joins(gbnns_index* ix, size_t keep) {
    while (ix->joins.size() > keep) {
        const std::pair<hipEvent_t, hipStream_t> j = ix->joins.front();
        ix->joins.pop_front();
        HIP_TRY(hipStreamWaitEvent(j.second, j.first, 0));
    }
    return GBNNS_OK;
}

int flush_join(gbnns_index* ix) { return flush_joins(ix, 0); }

// The refusals of a search call, in the order the tests pin, before anything touches a device (declared in api_internal.h).
int search_check(gbnns_index* ix, const gbnns_search_args* a, const TopkOut* topk, const TagIn* tag, const uint8_t* q_u8, bool* empty, bool routed) {
    *empty = false;
    if (!ix || !a) return fail(GBNNS_ERR_INVALID, "null argument");
    if (a->struct_size != sizeof(gbnns_search_args))
        return fail(GBNNS_ERR_INVALID, "gbnns_search_args.struct_size mismatch (%u != %zu)",
                    a->struct_size, sizeof(gbnns_search_args));
    if (a->mode < GBNNS_MODE_NET || a->mode > GBNNS_MODE_PLAIN) return fail(GBNNS_ERR_INVALID, "bad mode");
    if (a->ef <= 0) return fail(GBNNS_ERR_INVALID, "ef must be >= 1");
    if (a->mem_kind != GBNNS_MEM_HOST && a->mem_kind != GBNNS_MEM_DEVICE)
        return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", a->mem_kind);
    if (a->n_q == 0) {
        *empty = true;
        return GBNNS_OK;
    }
    if (a->n_q >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "n_q too large");
    if ((!a->queries && !q_u8) || !a->out_ids) return fail(GBNNS_ERR_INVALID, "queries / out_ids missing");
    if (a->mode == GBNNS_MODE_NET && !ix->has_net) return fail(GBNNS_ERR_INVALID, "NET mode needs a net");
    if (a->mode != GBNNS_MODE_PLAIN && !ix->db_low) return fail(GBNNS_ERR_INVALID, "mode needs db_low");
    if (a->flags & GBNNS_FLAG_HALF_WALK) {
        if (a->flags & GBNNS_FLAG_BYTE_WALK) return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_HALF_WALK together with GBNNS_FLAG_BYTE_WALK: a handle has one kind of rows");
        if (!ix->is(RowKind::F16)) return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_HALF_WALK needs a half-base handle (gbnns_index_create_half_base)");
        if (a->mode != GBNNS_MODE_PLAIN) return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_HALF_WALK: PLAIN only (NET / LOWQ walk db_low, which is float32)");
    }
    if (a->mode == GBNNS_MODE_PLAIN && ix->is(RowKind::U8) && !(a->flags & GBNNS_FLAG_BYTE_WALK))
        return fail(GBNNS_ERR_UNSUPPORTED, "GBNNS_MODE_PLAIN on a byte handle (gbnns_index_create_bytes) walks the uint8 rows: served with GBNNS_FLAG_BYTE_WALK only");
    if (a->flags & GBNNS_FLAG_BYTE_WALK) {
        if (ix->is(RowKind::F16)) return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_BYTE_WALK on a half-base handle (gbnns_index_create_half_base): it needs a byte handle (gbnns_index_create_bytes)");
        if (!ix->is(RowKind::U8)) return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_BYTE_WALK needs a byte handle (gbnns_index_create_bytes)");
        if (a->mode != GBNNS_MODE_PLAIN) return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_BYTE_WALK: PLAIN only (NET / LOWQ walk db_low, which is float32)");
    }
    if (a->mode == GBNNS_MODE_PLAIN && ix->is(RowKind::F16) && !(a->flags & GBNNS_FLAG_HALF_WALK))
        return fail(GBNNS_ERR_UNSUPPORTED, "GBNNS_MODE_PLAIN on a half-base handle (gbnns_index_create_half_base): there is no float table to walk; the half-row PLAIN walk is served with GBNNS_FLAG_HALF_WALK only");
    if (a->mode == GBNNS_MODE_LOWQ && !a->queries_low) return fail(GBNNS_ERR_INVALID, "queries_low missing");
    if ((a->flags & GBNNS_FLAG_LLF) && !(a->flags & GBNNS_FLAG_AUX_GRAPH))
        return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_LLF needs GBNNS_FLAG_AUX_GRAPH");
    if ((a->flags & GBNNS_FLAG_AUX_GRAPH) && !ix->has_aux)
        return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_AUX_GRAPH without gbnns_index_set_aux_graph");
    if (!tag && (a->flags & GBNNS_FLAG_TAG_BRIDGE))
        return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_TAG_BRIDGE has a meaning in gbnns_search_tagged only");
    if (!routed && (a->flags & GBNNS_FLAG_SCAN_GATHER))
        return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_SCAN_GATHER has a meaning in gbnns_search_tagged_auto only");
    if (tag) {
        if (a->flags & (GBNNS_FLAG_HALF_ROWS | GBNNS_FLAG_MFMA_PROJECTION))
            return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_search_tagged: GBNNS_FLAG_HALF_ROWS / GBNNS_FLAG_MFMA_PROJECTION are not served");
        if (!ix->tags.p) return fail(GBNNS_ERR_INVALID, "gbnns_search_tagged without gbnns_index_set_tags");
        if (!tag->qtags) return fail(GBNNS_ERR_INVALID, "gbnns_search_tagged: query_tags missing");
    }
    if (a->flags & GBNNS_FLAG_HALF_ROWS) {
        if (a->mode == GBNNS_MODE_PLAIN)
            return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_HALF_ROWS: NET / LOWQ only (a PLAIN walk's space is the answer space)");
        if (!ix->half_ready) return fail(GBNNS_ERR_INVALID, "GBNNS_FLAG_HALF_ROWS without gbnns_index_enable_half_rows");
    }
    if (a->hash_capacity != 0 && a->hash_capacity < 128)
        return fail(GBNNS_ERR_INVALID, "hash_capacity must be 0 (auto) or >= 128");
    const uint32_t n_ent = a->n_entries ? a->n_entries : 1u;
    if (n_ent > 1 && !a->entry_ids) return fail(GBNNS_ERR_INVALID, "n_entries > 1 needs entry_ids");
    if (n_ent > 4096) return fail(GBNNS_ERR_INVALID, "n_entries too large");
    if (topk) {
        if (a->mode == GBNNS_MODE_PLAIN)
            return fail(GBNNS_ERR_INVALID, "gbnns_search_topk: NET / LOWQ only (a PLAIN walk's out_cand / out_cand_dist are the answer in the walked space)");
        if (!topk->ids) return fail(GBNNS_ERR_INVALID, "gbnns_search_topk: out_top_ids missing");
        if (topk->k < 1 || topk->k > a->ef) return fail(GBNNS_ERR_INVALID, "gbnns_search_topk: k = %d outside 1 .. ef = %d", topk->k, a->ef);
        const size_t lds = rerank_topk_lds(ix->d_pad, (uint32_t)a->ef);
        if (lds > kMaxLds)
            return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_search_topk: query + %d candidates' keys and distances need %zu bytes of LDS (limit %zu)",
                        a->ef, lds, kMaxLds);
    }
    return GBNNS_OK;
}

// One search call: validation, the layout over the lanes, the batch (search_core).  `topk`: gbnns_search_topk's extra outputs.
int search_call(gbnns_index* ix, const gbnns_search_args* a, const TopkOut* topk, const TagIn* tag, const uint8_t* q_u8) {
    bool empty;
    if (int rc = search_check(ix, a, topk, tag, q_u8, &empty)) return rc;
    if (empty) return GBNNS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    int rc;
    int n_lanes = 1, lane = 0;
    g_slow.start();
    plan_call(ix, a, n_lanes, lane);
    if (n_lanes > 1 && a->mem_kind == GBNNS_MEM_HOST) {
        // a deferred call returns before its copies have run: every buffer has to be page-locked (a copy from or to
        // pageable memory is staged by the runtime, synchronously).  Pageable buffers: the flag is ignored, plain call.
        const size_t nq = (size_t)a->n_q, kk = (size_t)std::max(1, std::min(a->mode == GBNNS_MODE_PLAIN ? a->k : a->ef, a->ef));
        const struct { const void* p; size_t bytes; } bufs[] = {
            {a->queries, nq * ix->d * 4}, {a->queries_low, nq * ix->d_low * 4},
            {a->entry_ids, nq * std::max<size_t>(a->n_entries, 1) * 4}, {a->out_ids, nq * 4}, {a->out_hops, nq * 4},
            {a->out_dist_calc, nq * 4}, {a->out_edges, nq * 4}, {a->out_cand, nq * kk * 4}, {a->out_cand_dist, nq * kk * 4},
            {a->out_q_low, nq * ix->d_low * 4},
            {topk ? topk->ids : nullptr, nq * (topk ? (size_t)topk->k : 0) * 4}, {topk ? topk->dist : nullptr, nq * (topk ? (size_t)topk->k : 0) * 4},
            {tag ? tag->qtags : nullptr, nq * 4}, {q_u8, nq * ix->d}};
        for (const auto& b : bufs)
            if (b.p && !pinned_alias(static_cast<const char*>(b.p), b.bytes)) n_lanes = 1;
        if (n_lanes == 1) ix->next_lane = lane;  // (the rotation did not advance)
    }
    if (n_lanes <= 1) {
        if ((rc = enter_stream(ix, s))) return rc;
        return search_core(ix, ix->lanes[0], a, s, true, topk, tag, q_u8);
    }

    // ---- deferred join: the batch runs on lane `lane`'s internal stream ---------------------------------------
    if ((rc = ensure_lane(ix, lane))) return rc;
    Lane& L = ix->lanes[lane];
    if (!ix->fork_ev) HIP_TRY(hipEventCreateWithFlags(&ix->fork_ev, hipEventDisableTiming));
    bool same_stream = !ix->joins.empty() && ix->last_stream == s;
    for (const auto& j : ix->joins) same_stream = same_stream && j.second == s;
    if (same_stream) {
        // earlier calls' joins are still owed to this very stream: fork first, so that this batch is released beside
        // them, then let the stream wait for the oldest ones -- all but depth - 2, so that with this call at most
        // depth - 1 stay unjoined and `depth` batches are in flight
        HIP_TRY(hipEventRecord(ix->fork_ev, s));
        if ((rc = flush_joins(ix, (size_t)n_lanes - 2))) return rc;
    } else {
        if ((rc = enter_stream(ix, s))) return rc;
        HIP_TRY(hipEventRecord(ix->fork_ev, s));
    }
    ix->last_stream = s;
    ix->in_flight = true;
    HIP_TRY(hipStreamWaitEvent(L.stream, ix->fork_ev, 0));
    g_slow.mark("fork");
    if ((rc = search_core(ix, L, a, L.stream, false, topk, tag, q_u8))) {
        (void)hipDeviceSynchronize();  // leave nothing in flight behind an error
        ix->in_flight = false;
        return rc;
    }
    // (the join of the lane's batch before last -- the previous user of prev_ev -- has been enqueued by now: at most
    // depth - 1 joins stay owed, and that batch is at least depth calls old)
    std::swap(L.done_ev, L.prev_ev);
    L.prev_ticket = L.ticket;
    HIP_TRY(hipEventRecord(L.done_ev, L.stream));
    L.ticket = ++ix->issued;
    ix->joins.emplace_back(L.done_ev, s);
    g_slow.mark("recorded");
    g_slow.finish();
    return GBNNS_OK;
}

namespace {

// gbnns_search_tagged_auto's own outputs: k-answer rows, and per query the census count and the route taken (both optional)
struct AutoOut {
    int k;
    uint32_t* top_ids;
    float* top_dist;
    uint32_t* allowed;
    uint8_t* route;
};

// The routed call on DEVICE buffers, the caller's stream entered: census -> the routing on the host (the scan list, ascending) -> the walk of
// the whole batch, scan-routed queries under word 0 -> the exact scan of the listed queries, its rows scattered behind the walk.  Returns
// when the work has finished.
int auto_device(gbnns_index* ix, const gbnns_search_args* a, const uint8_t* q_u8, const uint32_t* qtags, uint64_t scan_below, const AutoOut& o,
                hipStream_t s) {
    Lane& L = ix->lanes[0];
    const uint32_t nq = (uint32_t)a->n_q, k = (uint32_t)o.k;
    int rc;
    if ((rc = L.census_ws.ensure(tag_census_ws_bytes(nq)))) return rc;
    if ((rc = L.auto_ws.ensure((size_t)nq * 20))) return rc;
    uint32_t* const allowed = L.auto_ws.as<uint32_t>();
    uint32_t *const first = allowed + nq, *const walk_tags = first + nq, *const entries = walk_tags + nq, *const list = entries + nq;
    HIP_TRY(launch_tag_census(ix->tags.as<uint32_t>(), ix->n, qtags, nq, L.census_ws.p, allowed, first, s));
    std::vector<uint32_t> h;
    try {
        h.resize(nq);
    } catch (...) {
        return fail(GBNNS_ERR_OOM, "host allocation failed");
    }
    if ((rc = host_copy_out(L, h.data(), allowed, (size_t)nq * 4, (size_t)nq * 4, 1, s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t m = 0;
    for (uint32_t i = 0; i < nq; ++i)
        if ((uint64_t)h[i] <= scan_below) h[m++] = i;  // (in place: m <= i)
    if (m && (rc = host_copy_in(L, list, h.data(), (size_t)m * 4, s))) return rc;
    HIP_TRY(launch_tag_route(allowed, first, qtags, nq, scan_below, walk_tags, a->entry_ids ? nullptr : entries, o.allowed, o.route, s));
    gbnns_search_args w = *a;
    if (!a->entry_ids) w.entry_ids = entries;  // every query enters at the lowest row it may see
    const TopkOut t{o.k, o.top_ids, o.top_dist};
    const TagIn g{walk_tags, (a->flags & GBNNS_FLAG_TAG_BRIDGE) != 0};
    if ((rc = search_core(ix, L, &w, s, false, &t, &g, q_u8))) return rc;
    if (m) {
        const size_t qbytes = ((size_t)m * ix->d * (q_u8 ? 1 : 4) + 15) & ~(size_t)15, rows = (size_t)m * k * 4;
        if ((rc = L.auto_scan.ensure(qbytes + (size_t)m * 4 + 2 * rows))) return rc;
        char* const gq = L.auto_scan.as<char>();
        uint32_t* const gtags = reinterpret_cast<uint32_t*>(gq + qbytes);
        uint32_t* const gids = gtags + m;
        float* const gdist = o.top_dist ? reinterpret_cast<float*>(gids + (size_t)m * k) : nullptr;
        HIP_TRY(launch_tag_gather(q_u8 ? static_cast<const void*>(q_u8) : a->queries, q_u8 ? 1 : 0, ix->d, qtags, list, m, gq, gtags, s));
        // (GBNNS_FLAG_SCAN_GATHER: the same rows from gbnns_index_exact_knn_gather's computation)
        const auto scan = (a->flags & GBNNS_FLAG_SCAN_GATHER) ? knn_gather_resident : knn_scan_resident;
        if ((rc = scan(ix, q_u8 ? nullptr : reinterpret_cast<const float*>(gq), q_u8 ? reinterpret_cast<const uint8_t*>(gq) : nullptr, m, gtags, o.k, gids,
                       gdist, s)))
            return rc;
        HIP_TRY(launch_tag_scatter(gids, gdist, list, m, k, o.top_ids, o.top_dist, a->out_ids, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    ix->in_flight = false;
    return GBNNS_OK;
}

// HOST buffers: every input uploaded, the same path, every output downloaded.
int auto_host(gbnns_index* ix, const gbnns_search_args* a, const uint8_t* q_u8, const uint32_t* qtags, uint64_t scan_below, const AutoOut& o,
              hipStream_t s) {
    Lane& L = ix->lanes[0];
    const size_t nq = (size_t)a->n_q, b4 = nq * 4, bc = b4 * (size_t)a->ef, bk = b4 * (size_t)o.k, bl = b4 * ix->d_low;
    const bool net = a->mode == GBNNS_MODE_NET;
    ScopedDevBuf q, qb, ql, ent, tg, ids, hops, dc, edges, cand, cdist, qlow, tids, tdist, allowed, route;
    int rc;
    auto up = [&](ScopedDevBuf& b, const void* src, size_t bytes) -> int {  // the device copy of an input (none: nullptr stays)
        if (!src) return GBNNS_OK;
        if (int r = b.ensure(bytes)) return r;
        return host_copy_in(L, b.p, src, bytes, s);
    };
    auto room = [&](ScopedDevBuf& b, const void* dst, size_t bytes) -> int { return dst ? b.ensure(bytes) : GBNNS_OK; };
    auto down = [&](const ScopedDevBuf& b, void* dst, size_t bytes) -> int { return dst ? host_copy_out(L, dst, b.p, bytes, bytes, 1, s) : GBNNS_OK; };
    if ((rc = up(q, a->queries, nq * ix->d * 4)) || (rc = up(qb, q_u8, nq * ix->d)) || (rc = up(ql, net ? nullptr : a->queries_low, bl)) ||
        (rc = up(ent, a->entry_ids, b4 * std::max<size_t>(a->n_entries, 1))) || (rc = up(tg, qtags, b4)))
        return rc;
    if ((rc = room(ids, a->out_ids, b4)) || (rc = room(hops, a->out_hops, b4)) || (rc = room(dc, a->out_dist_calc, b4)) ||
        (rc = room(edges, a->out_edges, b4)) || (rc = room(cand, a->out_cand, bc)) || (rc = room(cdist, a->out_cand_dist, bc)) ||
        (rc = room(qlow, net ? a->out_q_low : nullptr, bl)) || (rc = room(tids, o.top_ids, bk)) || (rc = room(tdist, o.top_dist, bk)) ||
        (rc = room(allowed, o.allowed, b4)) || (rc = room(route, o.route, nq)))
        return rc;
    gbnns_search_args w = *a;
    w.mem_kind = GBNNS_MEM_DEVICE;
    w.queries = q.as<float>(); w.queries_low = ql.as<float>(); w.entry_ids = ent.as<uint32_t>();
    w.out_ids = ids.as<uint32_t>(); w.out_hops = hops.as<int32_t>(); w.out_dist_calc = dc.as<int32_t>(); w.out_edges = edges.as<int32_t>();
    w.out_cand = cand.as<uint32_t>(); w.out_cand_dist = cdist.as<float>(); w.out_q_low = qlow.as<float>();
    const AutoOut od{o.k, tids.as<uint32_t>(), tdist.as<float>(), allowed.as<uint32_t>(), route.as<uint8_t>()};
    if ((rc = auto_device(ix, &w, qb.as<uint8_t>(), tg.as<uint32_t>(), scan_below, od, s))) return rc;
    if ((rc = down(ids, a->out_ids, b4)) || (rc = down(hops, a->out_hops, b4)) || (rc = down(dc, a->out_dist_calc, b4)) ||
        (rc = down(edges, a->out_edges, b4)) || (rc = down(cand, a->out_cand, bc)) || (rc = down(cdist, a->out_cand_dist, bc)) ||
        (rc = down(qlow, net ? a->out_q_low : nullptr, bl)) || (rc = down(tids, o.top_ids, bk)) || (rc = down(tdist, o.top_dist, bk)) ||
        (rc = down(allowed, o.allowed, b4)) || (rc = down(route, o.route, nq)))
        return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return GBNNS_OK;
}

}  // namespace

}  // namespace gbnns_api

extern "C" {

int gbnns_search_ex(gbnns_index* ix, const gbnns_search_args* a) { return search_call(ix, a, nullptr); }

int gbnns_search_topk(gbnns_index* ix, const gbnns_search_args* a, int k, uint32_t* out_top_ids, float* out_top_dist) {
    const TopkOut t{k, out_top_ids, out_top_dist};
    return search_call(ix, a, &t);
}

int gbnns_search_tagged(gbnns_index* ix, const gbnns_search_args* a, const uint32_t* query_tags, int k, uint32_t* out_top_ids, float* out_top_dist) {
    const TagIn g{query_tags, a && (a->flags & GBNNS_FLAG_TAG_BRIDGE) != 0};
    if (k == 0 && !out_top_ids && !out_top_dist) return search_call(ix, a, nullptr, &g);
    const TopkOut t{k, out_top_ids, out_top_dist};  // (k outside 1 .. ef, PLAIN mode, no out_top_ids: refused as for gbnns_search_topk)
    return search_call(ix, a, &t, &g);
}

int gbnns_search_byte_queries(gbnns_index* ix, const gbnns_search_args* a, const uint8_t* queries_u8, const uint32_t* query_tags, int k, uint32_t* out_top_ids,
                              float* out_top_dist) {
    if (!a) return fail(GBNNS_ERR_INVALID, "null argument");
    const bool sized = a->struct_size == sizeof(gbnns_search_args);  // (a mismatch: search_call's refusal)
    if (sized && a->queries) return fail(GBNNS_ERR_INVALID, "gbnns_search_byte_queries: args->queries must be NULL (the queries are queries_u8)");
    if (!ix) return fail(GBNNS_ERR_INVALID, "null argument");
    if (ix->is(RowKind::F16)) return fail(GBNNS_ERR_INVALID, "gbnns_search_byte_queries on a half-base handle (gbnns_index_create_half_base): it needs a byte handle (gbnns_index_create_bytes)");
    if (!ix->is(RowKind::U8)) return fail(GBNNS_ERR_INVALID, "gbnns_search_byte_queries needs a byte handle (gbnns_index_create_bytes)");
    if (sized && !queries_u8 && a->n_q) return fail(GBNNS_ERR_INVALID, "gbnns_search_byte_queries: queries_u8 missing");
    // the corresponding float call: gbnns_search_tagged with query_tags, else gbnns_search_topk with k-answer rows, else gbnns_search_ex
    const TagIn g{query_tags, (a->flags & GBNNS_FLAG_TAG_BRIDGE) != 0};
    const TagIn* gp = query_tags ? &g : nullptr;
    if (k == 0 && !out_top_ids && !out_top_dist) return search_call(ix, a, nullptr, gp, queries_u8);
    const TopkOut t{k, out_top_ids, out_top_dist};
    return search_call(ix, a, &t, gp, queries_u8);
}

int gbnns_index_tag_census(gbnns_index* ix, const uint32_t* query_tags, uint64_t n_q, uint32_t* out_allowed, uint32_t* out_first, int mem_kind,
                           void* stream) {
    if (!ix) return fail(GBNNS_ERR_INVALID, "null argument");
    if (!out_allowed && !out_first) return fail(GBNNS_ERR_INVALID, "gbnns_index_tag_census: out_allowed and out_first are both NULL");
    if (mem_kind != GBNNS_MEM_HOST && mem_kind != GBNNS_MEM_DEVICE) return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", mem_kind);
    if (!ix->tags.p) return fail(GBNNS_ERR_INVALID, "gbnns_index_tag_census without gbnns_index_set_tags");
    if (!query_tags && n_q) return fail(GBNNS_ERR_INVALID, "gbnns_index_tag_census: query_tags missing");
    if (n_q >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "n_q too large");
    if (n_q == 0) return GBNNS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    if ((rc = enter_stream(ix, s))) return rc;
    Lane& L = ix->lanes[0];
    const uint32_t nq = (uint32_t)n_q;
    const bool host = mem_kind == GBNNS_MEM_HOST;
    const size_t ws = (tag_census_ws_bytes(nq) + 15) & ~(size_t)15, b4 = (size_t)nq * 4;
    if ((rc = L.census_ws.ensure(ws + (host ? 3 * b4 : 0)))) return rc;
    uint32_t* const stage = reinterpret_cast<uint32_t*>(L.census_ws.as<char>() + ws);  // HOST buffers: the words, and the two results
    const uint32_t* q_dev = query_tags;
    uint32_t *a_dev = out_allowed, *f_dev = out_first;
    if (host) {
        if ((rc = host_copy_in(L, stage, query_tags, b4, s))) return rc;
        q_dev = stage;
        a_dev = out_allowed ? stage + nq : nullptr;
        f_dev = out_first ? stage + 2 * (size_t)nq : nullptr;
    }
    HIP_TRY(launch_tag_census(ix->tags.as<uint32_t>(), ix->n, q_dev, nq, L.census_ws.p, a_dev, f_dev, s));
    if (host) {
        if (out_allowed && (rc = host_copy_out(L, out_allowed, a_dev, b4, b4, 1, s))) return rc;
        if (out_first && (rc = host_copy_out(L, out_first, f_dev, b4, b4, 1, s))) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        ix->in_flight = false;
    }
    return GBNNS_OK;
}

int gbnns_debug_census_slot(uint32_t word, uint64_t n_q, uint32_t* slot, uint32_t* cap) {
    if (!slot || !cap) return fail(GBNNS_ERR_INVALID, "gbnns_debug_census_slot: null output");
    if (n_q == 0 || n_q > (1ull << 30)) return fail(GBNNS_ERR_INVALID, "gbnns_debug_census_slot: n_q must be in [1, 2^30] (the table's size is reported in 32 bits)");
    uint64_t c = 0;
    *slot = (uint32_t)tag_census_home_slot(word, n_q, &c);
    *cap = (uint32_t)c;
    return GBNNS_OK;
}

int gbnns_search_tagged_auto(gbnns_index* ix, const gbnns_search_args* a, const uint8_t* queries_u8, const uint32_t* query_tags, int k, uint64_t scan_below,
                             uint32_t* out_top_ids, float* out_top_dist, uint32_t* out_allowed, uint8_t* out_route) {
    // Every refusal before any work, none depending on the data: this call's own, then search_call's for the tagged top-k walk, then the scan's.
    if (!ix || !a) return fail(GBNNS_ERR_INVALID, "null argument");
    if (a->struct_size != sizeof(gbnns_search_args))
        return fail(GBNNS_ERR_INVALID, "gbnns_search_args.struct_size mismatch (%u != %zu)", a->struct_size, sizeof(gbnns_search_args));
    if (a->mode == GBNNS_MODE_PLAIN)
        return fail(GBNNS_ERR_INVALID, "gbnns_search_tagged_auto: NET / LOWQ only (a PLAIN walk's out_cand / out_cand_dist are the answer in the walked space)");
    if (a->flags & GBNNS_FLAG_DEFER_JOIN)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_search_tagged_auto: GBNNS_FLAG_DEFER_JOIN is not served (the call reads the census on the host)");
    if (ix->is(RowKind::F16))
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_search_tagged_auto on a half-base handle (gbnns_index_create_half_base): its scan route reads the resident table, and there is no exact scan over binary16 rows");
    if (ix->is(RowKind::U8)) {
        if (a->queries && queries_u8) return fail(GBNNS_ERR_INVALID, "gbnns_search_tagged_auto: args->queries must be NULL beside queries_u8");
        if (a->queries)
            return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_search_tagged_auto: float queries on a byte handle: there is no mixed-pair scan (uint8 rows against "
                        "float queries); pass queries_u8");
        if (ix->d > 256)
            return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_search_tagged_auto: d <= 256 on a byte handle (the byte scan's limit; got %u)", ix->d);
    } else {
        if (queries_u8) return fail(GBNNS_ERR_INVALID, "gbnns_search_tagged_auto: queries_u8 needs a byte handle (gbnns_index_create_bytes)");
        if (ix->d > 8192) return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_search_tagged_auto: d <= 8192 (the scan's limit; got %u)", ix->d);
    }
    if (ix->metric == GBNNS_METRIC_NEG_DOT && ix->d % 8 != 0)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_search_tagged_auto: the scan's negative-dot form needs d %% 8 == 0 (got %u)", ix->d);
    if (k < 1 || k > std::min(a->ef, 4096))
        return fail(GBNNS_ERR_INVALID, "gbnns_search_tagged_auto: k = %d outside 1 .. min(ef = %d, 4096)", k, a->ef);
    const TopkOut t{k, out_top_ids, out_top_dist};
    const TagIn g{query_tags, (a->flags & GBNNS_FLAG_TAG_BRIDGE) != 0};
    bool empty;
    if (int rc = search_check(ix, a, &t, &g, queries_u8, &empty, true)) return rc;
    if (empty) return GBNNS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    if (int rc = enter_stream(ix, s)) return rc;
    const AutoOut o{k, out_top_ids, out_top_dist, out_allowed, out_route};
    if (a->mem_kind == GBNNS_MEM_HOST) return auto_host(ix, a, queries_u8, query_tags, scan_below, o, s);
    return auto_device(ix, a, queries_u8, query_tags, scan_below, o, s);
}

int gbnns_index_wait(gbnns_index* ix, uint32_t keep) {
    if (!ix) return fail(GBNNS_ERR_INVALID, "null index");
    HIP_TRY(hipSetDevice(ix->device));
    const uint64_t upto = ix->issued > keep ? ix->issued - keep : 0;
    // a lane's stream runs its batches in order: its newest batch within the range covers the older ones
    for (Lane& L : ix->lanes) {
        if (L.ticket && L.ticket <= upto) HIP_TRY(hipEventSynchronize(L.done_ev));
        else if (L.prev_ticket && L.prev_ticket <= upto) HIP_TRY(hipEventSynchronize(L.prev_ev));
    }
    return GBNNS_OK;
}

int gbnns_index_join(gbnns_index* ix) {
    if (!ix) return fail(GBNNS_ERR_INVALID, "null index");
    HIP_TRY(hipSetDevice(ix->device));
    return flush_join(ix);
}

// The registrations made here: whole pages, never overlapping one another (two small heap buffers often share a page, and
// page-locking a page twice / releasing it under a neighbour is what the runtime's tables are not built for), counted per
// user buffer -- so that gbnns_host_unpin releases exactly what gbnns_host_pin registered and never a registration the
// caller made itself.
int gbnns_search_batch(gbnns_index* index, const float* queries, size_t n_q, int ef,
                       const uint32_t* entry_ids, uint32_t* out_ids, int32_t* out_hops,
                       int32_t* out_dist_calc, uint32_t* out_cand) {
    gbnns_search_args a{};
    a.struct_size = sizeof a;
    a.mode = GBNNS_MODE_NET;
    a.ef = ef;
    a.k = ef;
    a.mem_kind = GBNNS_MEM_HOST;
    a.n_q = n_q;
    a.queries = queries;
    a.entry_ids = entry_ids;
    a.out_ids = out_ids;
    a.out_hops = out_hops;
    a.out_dist_calc = out_dist_calc;
    a.out_cand = out_cand;
    return gbnns_search_ex(index, &a);
}

}  // extern "C"
