// call_plan.h -- the kernel sequence of one search call, decided as a value: call_plan (call_plan.cpp) reads the facts of the handle, of the
// walked space and of the call, and the sizing history of the call's statistics class, and returns what the launches need.  Plain host code like
// walk_plan.cpp: no handle, no lane, no stream, no HIP runtime call -- it runs without a device (tests/cpp/call_plan_units.cpp).
// search_core.cpp gathers the facts, applies the plan to its WalkParams and launches; sizing.cpp is the visited-set rule the plan calls.
#pragma once

#include "../../include/gbnns.h"
#include "row_kind.h"
#include "walk_plan.h"

#include <map>

namespace gbnns_api {

using namespace gbnns;

// The diagnostic knobs (defined and documented in handle.cpp).  Round 6: the eleven that steer a handle's searches live IN the handle
// (gbnns_index::knob, set with gbnns_index_knob); the process-wide values (environment, gbnns_debug_knob) are only the defaults a handle
// starts from, so a test or an A/B run that flips one no longer changes every other handle of the process.  The three knobs of
// gbnns_exact_knn -- a function without a handle -- stay process-wide.
struct Knobs {
    int quotient, vs_disp, max_waves, spec_min_nq, spec_any_form, mlp_small, mlp_net, mlp_slab, late_rows, spec_tail, coop, hot, byte_query_int, gather_budget, gather_timing, order_min, order_bits, half_walk_fast;
};

constexpr size_t kMaxLds = 160 * 1024;
// LDS is handed out in granules of 1 280 bytes (measured, tools/ubench/occupancy_census.hip: one-wavefront workgroups of
// 5 120 B -> 32 per CU, 5 121 .. 6 400 B -> 25, 6 401 .. 7 680 B -> 21): a wavefront's share is a multiple of it.
#ifndef GBNNS_LDS_GRAN
#define GBNNS_LDS_GRAN 1280
#endif
constexpr size_t kLdsGran = GBNNS_LDS_GRAN;

// general-kernel slots and the bitmap first pass: words of one visited bitmap; a multiple of 4 words: slots stay 16-B aligned (the bitmap pass clears with 16-B stores)
inline uint32_t bitmap_words_of(uint64_t n) { return ((uint32_t)((n + 31) / 32) + 3u) & ~3u; }

// Visited-set sizing feedback of a handle, shared by its lanes (host-side bookkeeping; the statistics of a call arrive asynchronously in the
// lane's pinned block and search_core.cpp folds them in before the next plan reads them).  Keyed by CallPlan::skey.
struct SizingHistory {
    std::map<int, uint32_t> cap_for_ef;
    std::map<int, uint32_t> maxdc_for_ef;  // largest dist_calc seen per (ef, mode, aux, wide): the raw figure behind cap_for_ef
    std::map<int, int> calm_streak;        // per (ef, mode): consecutive observed batches without hand-over / resize
    int calm(int skey) const {
        const auto it = calm_streak.find(skey);
        return it == calm_streak.end() ? 0 : it->second;
    }
    bool operator==(const SizingHistory& o) const { return cap_for_ef == o.cap_for_ef && maxdc_for_ef == o.maxdc_for_ef && calm_streak == o.calm_streak; }
};

// What the decision reads.
struct CallFacts {
    // the handle
    int metric;
    uint64_t n;
    uint32_t d, d_pad;        // original space (d_pad: the elements of a row, row_pad(d, rows))
    uint32_t ell_stride;
    uint32_t aux_stride;      // of the auxiliary graph a GBNNS_FLAG_AUX_GRAPH call walks; 0: none
    RowKind rows;             // the kind of the original-space rows (row_kind.h).  U8: the re-rank is fused only into the byte instances; F16: only a
                              // GBNNS_FLAG_HALF_WALK call's walk kernels read the rows, the re-rank is never fused
    size_t cus;               // compute units of the device
    Knobs knob;
    // the walked space
    uint32_t dim, dstride;
    bool half_rows;           // GBNNS_FLAG_HALF_ROWS
    RowKind walked;           // the kind of the WALKED rows: F32 but for a PLAIN call on a U8 / F16 handle (GBNNS_FLAG_BYTE_WALK / GBNNS_FLAG_HALF_WALK), which
                              // walks the handle's own rows (F16 with knob.half_walk_fast = 0: the general instance takes the whole batch)
    bool byte_queries;        // gbnns_search_byte_queries
    // the call
    int mode, ef;
    uint32_t n_entries;       // >= 1
    uint32_t flags;
    int32_t hash_capacity;
    uint32_t nq;
    bool tagged, bridged;     // gbnns_search_tagged (GBNNS_FLAG_TAG_BRIDGE)
    bool in_flight;           // on a lane's own stream: a batch of a deferred call
    bool sync_host;           // the call runs alone and is waited for
    bool stamps_on;           // diagnostic builds (GBNNS_STAMPS)
};

// sizing.cpp: the first pass's visited set for this batch -- sets w.vs_shr / hash_cap / hash_limit / spec_rows / spec_from
struct FirstPassSizing {
    bool auto_cap;                // capacity chosen by the library (hash_capacity == 0)
    int form;                     // 0 = 4-byte slots, 1 = packed, 2 = quotient
    uint32_t cap;                 // entries
};
FirstPassSizing size_first_pass(const CallFacts& f, const SizingHistory& h, int skey, WalkParams& w, const WalkPlan& plan);

enum class RetryAction { None, Launch, Copy };  // the retry pass: nothing / its kernel / list A copied to list B (nothing to gain)

struct CallPlan {
    int skey;                     // statistics class of the call (SizingHistory's key)
    // the decision fields of WalkParams (apply)
    int32_t coop, late_rows, spec_rows, all_general, force_wide, generic_only;
    uint32_t spec_from, vs_shr, hash_cap, hash_limit, rr_reserve, bytes_dim;
    WalkPlan first;               // the first pass: with the visited set in LDS, or (bitmap_pass) as bitmaps in HBM on bitmap_per_cu wavefronts per CU
    bool bitmap_pass;
    size_t bitmap_per_cu;
    bool fuse;                    // every walk kernel re-ranks its own query: no re-rank launch
    bool skip_retry;              // the first pass appends its hand-overs to list B itself
    RetryAction retry_action;
    WalkPlan retry;               // (RetryAction::Launch) with its visited set
    uint32_t retry_hash_cap, retry_hash_limit;
    FirstPassSizing sizing;
    void apply(WalkParams& w) const;  // the decision fields into a call's parameters
};

// The fields of a WalkParams that say what is walked and by which kind of call: everything plan_walk reads but the decisions above.  The tables
// plan_walk only asks the presence of (aux_ell, q_b) get a placeholder that is not null: a caller that launches puts its pointers there.
void set_walk_shape(WalkParams& w, const CallFacts& f);
// RowKind into the kernels' parameter fields, all of it (with set_walk_shape's walk_bytes / walk_half above): the table a call walks into
// db / db_b / db_h, the table its walk kernels re-rank from into rr_db / rr_db_b (F16: no walk kernel re-ranks)
void set_walked_table(WalkParams& w, RowKind walked, const void* table);
void set_fused_rerank_table(WalkParams& w, RowKind rows, const void* table);

CallPlan call_plan(const CallFacts& f, const SizingHistory& h);

}  // namespace gbnns_api
