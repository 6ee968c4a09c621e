// api_internal.h -- what the translation units of the C-ABI host layer share (round 5: api.cpp, 1 760 lines, was cut into
// handle.cpp / graph_api.cpp / lanes.cpp / search_core.cpp / sizing.cpp / pin.cpp; no behaviour change).
//   handle.cpp      the index handle: creation (uploads, layouts), destruction, projection / re-rank entry points, profiling,
//                   the diagnostic knobs, error text
//   graph_api.cpp   graph preparation: gbnns_exact_knn (heaps / matrix-core filter / pools), gbnns_exact_knn_bytes (uint8 rows), their tagged forms and gbnns_index_exact_knn, gbnns_build_graph_gd_device
//                   and gbnns_index_exact_knn_gather (the gathered exact scan: knn_gather.hip) with its two diagnostics
//   lanes.cpp       gbnns_search_ex and the batches-in-flight machinery (lanes, fork / join events), gbnns_index_wait / _join
//                   gbnns_index_tag_census and gbnns_search_tagged_auto (the census and the routing kernels: tag_census.hip)
//   search_core.cpp one batch on one lane, as a sequence of stages: workspaces, copies, the launches the call's plan names, statistics feedback
//   call_plan.cpp   which kernels a search call launches, on which visited set: a value decided from const facts (call_plan.h; no HIP calls)
//   sizing.cpp      the visited-set sizing rule of the first pass (capacity, form, wavefronts per CU), called by the plan
//   walk_plan.cpp   which walk kernel instance serves a pass over a shape, and its LDS layout (walk_plan.h; no HIP calls)
//   pin.cpp         gbnns_host_pin / gbnns_host_unpin and the page registry
//   row_kind.h      RowKind: float32 / uint8 / binary16 original-space rows -- the one statement of a handle's kind (gbnns_index::rows)
#pragma once

#include "../../include/gbnns.h"
#include "call_plan.h"
#include "row_kind.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>
#include <deque>
#include <new>
#include <mutex>
#include <set>
#include <string>
#include <vector>


namespace gbnns_api {

using namespace gbnns;

extern thread_local std::string g_err;
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? GBNNS_ERR_OOM : GBNNS_ERR_HIP,           \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,     \
                        __LINE__);                                                           \
    } while (0)

inline uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return GBNNS_OK;
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            bytes = 0;
            if (e != hipSuccess) return fail(GBNNS_ERR_HIP, "hipFree: %s", hipGetErrorString(e));
        }
        const size_t want = need + need / 8;  // slack so slightly larger batches do not realloc
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(GBNNS_ERR_OOM, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
        }
        bytes = want;
        return GBNNS_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// A call's own temporary: released where it goes out of scope.  (Index and lane members stay DevBuf: they are copied by value and
// released by gbnns_index_destroy.)
struct ScopedDevBuf : DevBuf {
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf&) = delete;
    ScopedDevBuf& operator=(const ScopedDevBuf&) = delete;
    ~ScopedDevBuf() { release(); }
};

struct ProfCall {
    hipEvent_t ev[5];  // begin, after project, after walk, after general, after rerank
    uint64_t queries;
    bool has_project, has_rerank;
};

constexpr int kMaxLanes = 4;

// GBNNS_SLOW_US=<microseconds>: a search call whose HOST side (enqueueing; no waiting in a deferred call) takes longer
// is reported on stderr with the time spent before each checkpoint.  Diagnostic; off by default.
struct SlowLog {
    using clock = std::chrono::steady_clock;
    long limit_us;
    clock::time_point t0;
    int n = 0;
    const char* name[24];
    long us[24];
    SlowLog() : limit_us(getenv("GBNNS_SLOW_US") ? atol(getenv("GBNNS_SLOW_US")) : 0) {}
    void start() { if (limit_us) { t0 = clock::now(); n = 0; } }
    void mark(const char* what) {
        if (limit_us && n < 24) { name[n] = what; us[n++] = (long)std::chrono::duration_cast<std::chrono::microseconds>(clock::now() - t0).count(); }
    }
    void finish() {
        if (!limit_us || n == 0 || us[n - 1] < limit_us) return;
        std::fprintf(stderr, "gbnns slow call:");
        for (int i = 0; i < n; ++i) std::fprintf(stderr, " %s@%ld", name[i], us[i]);
        std::fprintf(stderr, " us\n");
    }
};
extern thread_local SlowLog g_slow;

// One workspace of per-batch buffers + control words.  A handle has several so that consecutive batches can be
// in flight side by side on internal streams (the tail of one batch's walk -- a 10 k batch is < 2 "rounds" of
// resident wavefronts -- then runs beside the projection and the first round of the next one).
struct Lane {
    hipStream_t stream = nullptr;      // internal stream (created on the lane's first deferred call)
    hipEvent_t done_ev = nullptr;      // recorded after the lane's batch of a deferred call
    hipEvent_t prev_ev = nullptr;      // ... and the one of the lane's batch before (the two alternate)
    uint64_t ticket = 0, prev_ticket = 0;  // serial numbers of those two batches (0 = none), for gbnns_index_wait
    DevBuf q_in, q_low, h1, h2, cand, cand_dist, cnt, hops, dc, edges, out, entries, ovf_list, ovf2_list, ctrl;
    DevBuf g_bitmap, g_keys, fp_bitmap, order, order_hist;
    DevBuf top_ids, top_dist;          // the k-answer rows of a HOST call (gbnns_rerank_topk / gbnns_search_topk)
    DevBuf qtags;                      // the query tag words of a HOST call (gbnns_search_tagged)
    DevBuf q_in_b;                     // the byte queries of a HOST call (gbnns_search_byte_queries; their widening goes to q_in)
    DevBuf census_ws;                  // gbnns_index_tag_census: the dedupe table, the per-word counters and lists (and a HOST call's arrays)
    DevBuf auto_ws, auto_scan;         // gbnns_search_tagged_auto: census results, walk words, entries, scan list / the scan's gathered queries and rows
    // visited-set sizing feedback: stats of an earlier call arrive asynchronously in pinned memory
    uint32_t* h_stats = nullptr;       // [4] copy of ctrl after the walk kernels
    hipEvent_t stats_ev = nullptr;
    bool stats_pending = false;
    int stats_ef = 0;
    uint32_t stats_cap = 0;
    // which of the two control-word blocks the next call uses, and whether each is known to be zero
    int ctrl_phase = 0;
    bool ctrl_clean[2] = {true, true};
    bool ctrl_ready = false;
    uint32_t last_general = 0;
    // page-locked staging for a caller's PAGEABLE host buffers (host_copy_in / host_copy_out, handle.cpp)
    void* stage = nullptr;             // two halves, used alternately
    hipEvent_t stage_ev[2] = {nullptr, nullptr};  // recorded behind the last copy that reads / writes a half
    bool stage_busy[2] = {false, false};
    int stage_next = 0;
    DevBuf* bufs(int i) {
        DevBuf* b[] = {&q_in, &q_low, &h1, &h2, &cand, &cand_dist, &cnt, &hops, &dc, &edges, &out, &entries,
                       &ovf_list, &ovf2_list, &ctrl, &g_bitmap, &g_keys, &fp_bitmap, &order, &order_hist, &top_ids, &top_dist, &qtags, &q_in_b,
                       &census_ws, &auto_ws, &auto_scan};
        return i < (int)(sizeof b / sizeof b[0]) ? b[i] : nullptr;
    }
};

// the diagnostic knobs: struct Knobs, call_plan.h (defined and documented in handle.cpp)
Knobs knob_defaults();                                    // the process-wide defaults as they stand now
bool knob_set(Knobs& k, const char* name, int value);     // clamps like the environment does; false = no such handle knob
extern std::atomic<int> g_knob_knn_chunk, g_knob_knn_pool_min_k, g_knob_knn_filter, g_knob_knn_slab;

}  // namespace gbnns_api

struct gbnns_index {
    using DevBuf = gbnns_api::DevBuf;
    using Lane = gbnns_api::Lane;
    using ProfCall = gbnns_api::ProfCall;
    int device = 0;
    int metric = 0;
    uint64_t n = 0;
    uint32_t d = 0, d_low = 0, d_hidden = 0;
    uint32_t d_pad = 0, dl_pad = 0;
    // The original-space table [n x d_pad]: rows of `rows` elements (row_kind.h: float32, uint8 -- gbnns_index_create_bytes --, or binary16 --
    // gbnns_index_create_half_base), d_pad = row_pad(d, rows) elements a row (= the floats of a staged re-rank query), zero padded, 16-byte
    // aligned; borrowed or base_own's.  One table, one kind: no float copy of a byte or half table exists.  (Not low_half: that is the WALKED
    // table of GBNNS_FLAG_HALF_ROWS, which a handle of any kind may have as well.)
    gbnns::RowKind rows = gbnns::RowKind::F32;
    const void* base = nullptr;
    template <typename T>
    const T* base_as() const {  // the table for a launcher of the kind whose element is T
        assert(sizeof(T) == gbnns::row_elem_bytes(rows));
        return static_cast<const T*>(base);
    }
    bool is(gbnns::RowKind k) const { return rows == k; }
    const float* db_low = nullptr;  // [n x dl_pad]
    DevBuf base_own, db_low_own, ell, net, aux_ell;
    DevBuf net_mfma;                // the net repacked for the one-launch matrix-core projection (filled on the option's first use)
    // GBNNS_FLAG_HALF_ROWS (gbnns_index_enable_half_rows): R = float32(float16(db_low)) as binary16 rows [n x round_up(d_low, 8)], zero padded,
    // and as float32 rows in db_low's own layout [n x dl_pad]; db_low itself stays, for the searches without the flag
    DevBuf low_half, low_r;
    bool half_ready = false;
    DevBuf tags;                    // gbnns_index_set_tags: [n] tag words, all ones until written (empty: no table)
    bool net_mfma_ready = false;
    int net_form = -1;              // form of the last one-launch exact projection (kernels.h: kNetWholeCu / kNetHalfCu; -1: none yet)
    gbnns::ProjPlan proj_last{};    // the kernel instances the last projection launched, in launch order (gbnns_index_project_last)
    uint32_t ell_stride = 0, aux_stride = 0;
    bool has_aux = false;
    bool has_net = false;
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
    uint32_t ws1 = 0, ws2 = 0, ws3 = 0;
    const float* net_img[2][3] = {};   // [form][layer]: the weights in the one-launch projection's staged order (kernels.h pack_net_image; in `net`)
    int cus = 0;                   // compute units of the device (sizes the one-launch projection's query strips)
    size_t cu_count() const { return cus > 0 ? (size_t)cus : 256; }   // ... for the walk's residency rules (unknown: an MI355X's)
    gbnns_api::Knobs knob{};        // this handle's diagnostic knobs (gbnns_index_knob; start: the process defaults at creation)
    // workspaces: lane 0 serves plain calls on the caller's stream; the batches of deferred calls rotate over
    // lanes 0 .. n_lanes-1, each on its own internal stream (see gbnns_search_ex)
    Lane lanes[gbnns_api::kMaxLanes];
    hipEvent_t fork_ev = nullptr;      // caller's stream -> lanes
    // profiling
    bool profiling = false;
    std::vector<ProfCall> pending;
    gbnns_profile acc{};
    uint32_t* prof_ctrl = nullptr;     // [4] page-locked copy of the last profiled call's control words (hand-over counts), made behind its general kernel
    bool prof_ctrl_pending = false;    // ... a copy is under way or done and not yet read; prof_ctrl_direct: that call's first pass appended to list B itself
    bool prof_ctrl_direct = false;
    gbnns_api::SizingHistory history;  // visited-set sizing feedback, shared by the lanes (call_plan.h)
    uint32_t stats_tick = 0;
    std::deque<std::pair<hipEvent_t, hipStream_t>> joins;  // (batch's event, caller's stream) of the deferred calls not yet joined, oldest first
    int next_lane = 0;
    uint64_t issued = 0;               // deferred calls so far
    // stream of the last call that left work in flight (the workspace and the control words are ordered by
    // stream order only: a call on another stream first waits for that work, see enter_stream)
    hipStream_t last_stream = nullptr;
    bool in_flight = false;
    hipEvent_t order_ev = nullptr;
    // locality order (search_core.cpp; knobs "order_min" / "order_bits"): queries the last search call walked in it (0: none -- the knob
    // "order_last"), and the lane and batch size of the last call that was ordered (gbnns_index_order_last reads that lane's permutation)
    uint32_t order_last = 0, order_perm_n = 0;
    int order_perm_lane = -1;
    // gbnns_index_exact_knn_gather with the knob "gather_timing": the last call's census / fill / scan microseconds and its rounds (gbnns_index_knob_get)
    int gather_us[3] = {0, 0, 0};
    int gather_rounds = 0;
};

namespace gbnns_api {

// handle.cpp
int h2d_staged(void* dst, const void* src, size_t bytes);
int d2h_staged(void* dst, const void* src_dev, size_t bytes, hipStream_t s);   // (waits for s; returns with the bytes in dst)
// Copies between a caller's HOST buffer and device memory for the per-call entry points (gbnns_search_ex, gbnns_project,
// gbnns_rerank), enqueued on `s`.  Page-locked caller memory is handed to the runtime as it is (asynchronous, as before); pageable
// memory passes through the lane's own page-locked staging buffer in pieces, for the reason given at h2d_staged -- host_copy_out
// then returns with the data in place.  host_copy_out: `rows` rows of `width` bytes, `spitch` bytes apart on the device, packed at dst.
struct Lane;
int host_copy_in(Lane& L, void* dst_dev, const void* src, size_t bytes, hipStream_t s);
int host_copy_out(Lane& L, void* dst, const void* src_dev, size_t spitch, size_t width, size_t rows, hipStream_t s);
int upload(DevBuf& dst, const void* src, size_t rows, size_t row_floats, size_t pad_floats, int mem_kind);
int build_ell(const uint64_t* off, const uint32_t* nbr, uint64_t n, std::vector<uint32_t>& ell, uint32_t& stride);
int run_project(gbnns_index* ix, Lane& L, const float* x, uint32_t xstride, uint32_t nx, float* out, hipStream_t s, bool in_flight = false,
                bool mfma = false);
int prof_flush(gbnns_index* ix);
// the stand-alone re-rank over the handle's original-space table, by the kernels of its row kind (rerank.hip / rerank_bytes.hip / rerank_half.hip);
// the table and its row stride are the handle's, whatever the caller put into r.db / r.dstride.  P: RerankParams (the best of every list) or
// RerankTopkParams (its k best)
template <class P>
hipError_t rerank_launch(const gbnns_index* ix, const P& r, hipStream_t s);

// lanes.cpp
int enter_stream(gbnns_index* ix, hipStream_t s);
int ensure_lane(gbnns_index* ix, int i);
void plan_call(gbnns_index* ix, const gbnns_search_args* a, int& lanes, int& lane);
int flush_joins(gbnns_index* ix, size_t keep);
int flush_join(gbnns_index* ix);

// The k best of each query's candidates beside a search's answers (gbnns_search_topk): ids [n_q x k], dist likewise or nullptr;
// buffers of args->mem_kind.
struct TopkOut {
    int k;
    uint32_t* ids;
    float* dist;
};

// gbnns_search_tagged's extra input: the queries' tag words [n_q], a buffer of args->mem_kind
struct TagIn {
    const uint32_t* qtags;
    bool bridge;  // GBNNS_FLAG_TAG_BRIDGE: disallowed neighbours are looked through
};

// lanes.cpp: the body of gbnns_search_ex / gbnns_search_topk / gbnns_search_tagged / gbnns_search_byte_queries (topk == nullptr: no k-answer rows;
// tag == nullptr: untagged; q_u8 != nullptr: the queries as bytes, a->queries is nullptr)
int search_call(gbnns_index* ix, const gbnns_search_args* a, const TopkOut* topk, const TagIn* tag = nullptr, const uint8_t* q_u8 = nullptr);

// lanes.cpp: search_call's refusals, in its order, before anything touches a device; *empty: a valid call without queries, nothing to do;
// routed: the call is gbnns_search_tagged_auto, the one call GBNNS_FLAG_SCAN_GATHER belongs to
int search_check(gbnns_index* ix, const gbnns_search_args* a, const TopkOut* topk, const TagIn* tag, const uint8_t* q_u8, bool* empty, bool routed = false);

// graph_api.cpp: gbnns_index_exact_knn's computation (self_offset -1) for a caller that has entered the stream itself: DEVICE buffers,
// exactly one of queries / queries_u8 (the handle's kind); returns behind a synchronisation of `s`
int knn_scan_resident(gbnns_index* ix, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags, int k,
                      uint32_t* out_ids, float* out_dist, hipStream_t s);

// graph_api.cpp: the same for gbnns_index_exact_knn_gather's computation (GBNNS_FLAG_SCAN_GATHER); query_tags required
int knn_gather_resident(gbnns_index* ix, const float* queries, const uint8_t* queries_u8, uint64_t n_q, const uint32_t* query_tags, int k,
                        uint32_t* out_ids, float* out_dist, hipStream_t s);

// search_core.cpp
int search_core(gbnns_index* ix, Lane& L, const gbnns_search_args* a, hipStream_t s, bool sync_host, const TopkOut* topk = nullptr,
                const TagIn* tag = nullptr, const uint8_t* q_u8 = nullptr);


// How one call is laid out over the handle's lanes (workspace + internal stream each).
//   * default: lane 0 in the caller's stream -- kernels back to back.
//   * GBNNS_FLAG_DEFER_JOIN (DEVICE buffers, or HOST buffers that are all page-locked): the whole batch on the next of
//     `defer_depth` lanes, consecutive calls rotating, so that the projection (and, for HOST buffers, the copy-in) of
//     batch i+1 runs in the half-empty tail of batch i's walk kernel.
// Measured and NOT done (profiles/r03_split_timelines.txt): cutting one batch into sub-batches on two streams.  A walk
// kernel of 2 500 queries lasts 0.14 ms -- the latency chain of its longest walk -- where 10 000 queries take 0.33 ms,
// and the projection blocks of the next piece (4 wavefronts, 14 KB of LDS) are not scheduled while a walk kernel still
// has workgroups to dispatch (its single wavefronts take the LDS as it frees up), so the pieces queue behind one
// another: 0.43 ms (halves) ... 0.52 ms (quarters) against 0.40 ms undivided.  The same holds with page-locked HOST
// buffers, where the halves' copies do overlap: 0.55 against 0.52 ms.
// The device-visible alias of a page-locked host buffer of `bytes` bytes (hipHostMalloc / hipHostRegister memory); nullptr
// for pageable memory -- and for a buffer whose page-locked range ends before its last byte (a partly registered array, an
// interior pointer near the end of a registration): both ends must be page-locked and map to one contiguous device range.
// Stores through the alias are visible to the host once the storing stream's work has completed.
template <class T>
T* pinned_alias(const T* host_ptr, size_t bytes) {
    if (!host_ptr || bytes == 0) return nullptr;
    auto probe = [](const void* p) -> void* {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess) {
            (void)hipGetLastError();  // (unregistered memory is an error for some runtimes, a type for others)
            return nullptr;
        }
        return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
    };
    char* const first = static_cast<char*>(probe(host_ptr));
    if (!first) return nullptr;
    if (bytes > 1) {
        char* const last = static_cast<char*>(probe(reinterpret_cast<const char*>(host_ptr) + (bytes - 1)));
        if (last != first + (bytes - 1)) return nullptr;
        // both ends page-locked and contiguous on the device side; two separate registrations with an unregistered hole
        // between them would pass that too: where the runtime reports the extent of the mapping the first byte belongs to,
        // the whole buffer has to lie inside it
        hipDeviceptr_t rbase = nullptr;
        size_t rsize = 0;
        if (hipMemGetAddressRange(&rbase, &rsize, first) == hipSuccess && rbase && rsize) {
            if (first < static_cast<char*>(rbase) || first + bytes > static_cast<char*>(rbase) + rsize) return nullptr;
        } else {
            (void)hipGetLastError();
        }
    }
    return reinterpret_cast<T*>(first);
}

}  // namespace gbnns_api

// tag_census.hip: the census of a tag table and the routing kernels of gbnns_search_tagged_auto (documented there)
namespace gbnns {
size_t tag_census_ws_bytes(uint64_t nq);
uint64_t tag_census_home_slot(uint32_t word, uint64_t nq, uint64_t* cap);
hipError_t launch_tag_census(const uint32_t* tags, uint64_t n, const uint32_t* qtags, uint32_t nq, void* ws, uint32_t* out_allowed,
                             uint32_t* out_first, hipStream_t s);
hipError_t launch_tag_route(const uint32_t* allowed, const uint32_t* first, const uint32_t* qtags, uint32_t nq, uint64_t scan_below, uint32_t* walk_tags,
                            uint32_t* entries, uint32_t* out_allowed, uint8_t* out_route, hipStream_t s);
hipError_t launch_tag_gather(const void* queries, int bytes, uint32_t d, const uint32_t* qtags, const uint32_t* list, uint32_t m, void* dst,
                             uint32_t* dst_tags, hipStream_t s);
hipError_t launch_tag_scatter(const uint32_t* ids, const float* dist, const uint32_t* list, uint32_t m, uint32_t k, uint32_t* top_ids, float* top_dist,
                              uint32_t* out_ids, hipStream_t s);
}  // namespace gbnns
