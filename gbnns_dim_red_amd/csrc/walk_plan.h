// walk_plan.h -- which walk kernel instance serves a pass over a shape, and the LDS layout that instance uses: decided in ONE place, plan_walk
// (walk_plan.cpp: plain host code).  The host layer (call_plan.cpp, sizing.cpp) sizes the visited set, the re-rank room and the retry pass from
// the plan; launch_walk (walk_l2.hip) launches the very instance the plan names: the LDS a kernel runs on is always the LDS of its own layout.
#pragma once

#include "kernels.h"

namespace gbnns {

// Layout constants the plan shares with the kernels.  Layout of the one-register hot instances (ef <= 64), A/B switches: GBNNS_HOT1_QLDS = the query is re-read from LDS every
// hop (64 vector registers: 8 wavefronts per SIMD) instead of living in 16 registers (72: 7 per SIMD); GBNNS_HOT1_SPEC = the
// rows are requested before the visited test (speculatively, for every valid slot) instead of after it (new ids only).
#ifndef GBNNS_HOT1_QLDS
#define GBNNS_HOT1_QLDS 1
#endif
#ifndef GBNNS_HOT1_SPEC
#define GBNNS_HOT1_SPEC 0
#endif
constexpr int kRegTieCap = 16;       // tie list of the register kernel (LDS, 128 B)
constexpr int kRegListMaxEf = 1024;  // largest ef served by the register-list / two-list kernels (beyond: result list as one sorted LDS array)
constexpr int kRegStageSlots = 66;   // merge scatter buffer: ranks 0..ef (ef <= 64), padded to 16 B
constexpr int kBigMaxEf = kRegListMaxEf;  // (the two-list structure itself reaches 64 chunks = 4 096 entries: one mask lane per chunk)
#ifndef GBNNS_HOT2_MAX
#define GBNNS_HOT2_MAX 128  // (64: experiments with the two-list kernels from ef = 65 on)
#endif
constexpr int kHot2MaxEf = GBNNS_HOT2_MAX;  // up to here the two-register lists (walk_hot_one<2>, walk_reg_one<2>) are the faster ones
constexpr int kPlain512PairMinEf = 200;  // 512-byte rows (PLAIN walks over sift vectors): beams beyond this take the pair-form two-list instance
constexpr int kBridgeStageIds = 64;  // walk_bridge.hip: ids of a bridged adjacency row staged in LDS between two runs of the hop step (two 32-slot chunks)
constexpr size_t kCoopExtraLds = 1280;  // the two-wavefront walk's two 64-word result buffers + three 64-word slots of adjacency words requested ahead (its mailbox lives in the query area)

// LDS of a two-list instance besides the visited set: [tie list][front-merge buffer: 66 keys][base list: ef_pad keys]
// [flush flags: ef_pad + 64 bytes], ef_pad = ef rounded up to 64.  The flush flags live inside the front-merge buffer
// when they fit (ef <= 448: the two are never in use at the same time) -- at ef = 140 .. 180 those 256 bytes are what
// separates 14 / 13 / 12 resident wavefronts per CU from 15 / 14 / 13.
__host__ __device__ __forceinline__ constexpr bool big_list_flags_in_stage(int ef) {
    return (size_t)((ef + 63) / 64 * 64) + 64 <= (size_t)kRegStageSlots * 8;
}
__host__ __device__ __forceinline__ constexpr size_t big_list_fixed_bytes(int ef) {
    return (size_t)kRegTieCap * 8 + (size_t)kRegStageSlots * 8 + (size_t)((ef + 63) / 64 * 64) * 8 +
           (big_list_flags_in_stage(ef) ? 0 : (size_t)((ef + 63) / 64 * 64) + 64);
}

enum class WalkPass { First, Bitmap, Retry };  // first pass with the visited set in LDS / as bitmaps in HBM; retry pass over the hand-overs
enum class WalkFamily : uint8_t {
    None,       // no instance serves what was asked for (the two-wavefront walk on a shape it has no instance for): launching it is an error
    Coop,       // walk_coop_kernel<STEPS, LATE>                                     (walk_coop.hip)
    Hot,        // walk_hot* / walk_hotw* / walk_hot_dot*: hand-laid-out, 128-byte rows (walk_hot.hip)
    RegWide,    // walk_reg_wide_kernel<STEPS, LATE>: 192- / 256-byte rows, ef <= 64  (walk_wide.hip)
    RegList,    // walk_reg_kernel<METRIC, STEPS, OFF32, RETRY, R, ONE_CHUNK, AUX>   (walk_l2 / walk_dot / walk_wide / walk_wide3)
                // half: walk_reg_half_kernel<METRIC, STEPS, R, ONE_CHUNK>          (walk_half.hip)
    TwoList,    // walk_reg_big_kernel<METRIC, STEPS, OFF32, RETRY, AUX, ONE_PASS, LATE> (walk_l2 / walk_dot / walk_wide / walk_wide2)
                // half: walk_reg_big_half_kernel<METRIC, STEPS, ONE_PASS, LATE>    (walk_half.hip)
                // tag (either family): walk_reg_tag_kernel<METRIC, STEPS, R, ONE_CHUNK> / walk_reg_big_tag_kernel<METRIC, STEPS, ONE_PASS, LATE> (walk_tag.hip)
                // bridge (register lists): walk_bridge_kernel<METRIC, STEPS, R>                (walk_bridge.hip)
                // byte walk (either family): walk_reg_bytes_kernel<R, ONE_CHUNK> / walk_reg_big_bytes_kernel<ONE_PASS> (walk_bytes.hip)
                // ... with byte queries: beam_u8_kernel<R, ONE_CHUNK> / beam_u8_big_kernel<ONE_PASS> (walk_bytes_q.hip)
                // half walk (either family): walk_reg_hwalk_kernel<STEPS, R, ONE_CHUNK> / walk_reg_big_hwalk_kernel<STEPS, ONE_PASS> (walk_half_base.hip)
    LdsList,    // walk_fast_kernel<METRIC, STEPS, RETRY, PACKED>                    (walk_l2 / walk_dot / walk_wide)
    BitmapReg,  // walk_bitmap_reg_kernel<METRIC, R>                                 (walk_bitmap.hip)
    BitmapBig,  // walk_bitmap_big_kernel<METRIC, STEPS, ONE_PASS, LATE>
    BitmapLds,  // walk_bitmap_kernel<METRIC, STEPS>
};

// The switches of a walk kernel instance, one bit each: the one vocabulary of plan_walk, the units' instance tables and the device templates
// (walk_reg_one / walk_reg_big_one take them as one mask, walk_generic.h).  A switch the family does not have stays clear.
enum WalkFlag : uint32_t {
    kOff32 = 1u << 0,       // compact index: 32-bit byte offsets, 24-bit ids
    kRetry = 1u << 1,       // the retry pass over the hand-overs
    kOne = 1u << 2,         // adjacency rows of one 32-slot pass (ONE_PASS / ONE_CHUNK; the hot family: its one-pass instances, else walk_hotw*)
    kAux = 1u << 3,         // auxiliary-graph hop
    kLate = 1u << 4,        // rows requested after the visited test (WalkParams::late_rows)
    kSpec = 1u << 5,        // walk_hot_spec_kernel: rows requested before the visited test (spec_rows)
    kPacked = 1u << 6,      // LDS-list family: visited set of 24-bit ids
    kHalf = 1u << 7,        // the hop's rows come from the 2-byte table (WalkParams::db_h): walk_reg_half_kernel / walk_reg_big_half_kernel (walk_half.hip)
    kTag = 1u << 8,         // the hop tests every neighbour's tag word against the query's (WalkParams::tags / qtags): walk_reg_tag_kernel / walk_reg_big_tag_kernel (walk_tag.hip)
    kBridge = 1u << 9,      // (with kTag) a disallowed neighbour is looked through, its allowed neighbours staged in LDS in its place: walk_bridge_kernel (walk_bridge.hip)
    kRrBytes = 1u << 10,    // the fused re-rank reads uint8 rows (WalkParams::rr_db_b, a byte handle): walk_hot_bytes_kernel / walk_hot2_bytes_kernel (walk_hot.hip)
    kByteWalk = 1u << 11,   // the WALKED rows are uint8 (WalkParams::db_b, GBNNS_FLAG_BYTE_WALK): walk_reg_bytes_kernel / walk_reg_big_bytes_kernel (walk_bytes.hip)
    kByteQuery = 1u << 12,  // (with kByteWalk) the queries are uint8 too (WalkParams::q_b, gbnns_search_byte_queries), the distance is integer: beam_u8_kernel / beam_u8_big_kernel (walk_bytes_q.hip)
    kBitmap = 1u << 13,     // from here on the device templates only, never in a WalkInstance (its family says as much): visited set = one bit per node in HBM (walk_bitmap_*_kernel)
    kQueryLds = 1u << 14,   // walk_reg_one: the lane's query pieces are re-read from LDS every hop (walk_reg_wide_kernel)
    kNeverLate = 1u << 15,  // walk_reg_one: rows never requested after the visited test (without it and without kLate: by WalkParams::late_rows)
    kHalfWalk = 1u << 16,   // (a WalkInstance flag again) the WALKED rows are a half-base handle's binary16 rows (WalkParams::db_h, GBNNS_FLAG_HALF_WALK), the entry row's included: walk_reg_hwalk_kernel / walk_reg_big_hwalk_kernel (walk_half_base.hip)
};
__host__ __device__ constexpr uint32_t flag_if(bool on, uint32_t flag) { return on ? flag : 0u; }

// One kernel instance, named completely: its family and every template argument.  An argument the family does not have stays 0 / clear.
struct WalkInstance {
    WalkFamily family;
    int metric;      // 0 = L2, 1 = negative dot
    int steps;       // 16-byte steps of a row the distance is unrolled for (0: run-time length)
    int regs;        // list registers per lane: 1 (ef <= 64), 2 (ef <= 128); 4 = the two-list structure
    uint32_t flags;  // WalkFlag bits
};
inline bool operator==(const WalkInstance& a, const WalkInstance& b) { return a.family == b.family && a.metric == b.metric && a.steps == b.steps && a.regs == b.regs && a.flags == b.flags; }

struct WalkPlan {
    WalkPass pass;
    WalkInstance inst;
    // layout facts of that instance (none of them depends on the visited set's size or form)
    size_t lds_fixed;      // LDS bytes of a wavefront (two-wavefront walk: of a query) without the visited set
    bool packed;           // visited set without the quotient form: five 24-bit ids per 16-byte bucket (else 4-byte slots)
    bool knows_quotient;   // the instance reads WalkParams::vs_shr
    bool lds_list;         // result list in LDS as one sorted array: no fused re-rank
    bool coop_serves;      // the two-wavefront walk has an instance for this shape (whether or not this plan is it)
    bool general_only;     // several entry points per query, or a tagged / bridged / byte-walk / half-walk call outside its instances' domain: the general kernel takes the whole batch
    size_t rr_base;        // room of the fused re-rank's query = rr_base (+ the visited set's bytes when rr_in_table)
    bool rr_in_table;      // (rr_room below)
    // form of the visited set (walk_hash_bytes, kernels.h); vs_shr is set only where the instance knows the quotient form
    int hash_form(uint32_t vs_shr) const { return vs_shr ? 2 : (packed ? 1 : 0); }
    size_t rr_room(size_t hash_bytes) const { return rr_base + (rr_in_table ? hash_bytes : 0); }
};

// Environment switches, read once: GBNNS_WIDE2=0 sends the 384- / 512-byte rows to the run-time-length instances at every beam (A/B runs);
// GBNNS_STAMPS_GENERIC keeps diagnostic (GBNNS_STAMPS) builds off the hot two-list instances.
struct WalkEnv { bool wide2, stamps_generic; };
const WalkEnv& walk_env();
// Reads the shape (dim, dstride, n, ell_stride, aux_ell / aux_stride), ef, n_entries, force_wide, coop, late_rows, spec_rows, stamps_on, half_rows, tagged, bridged, generic_only, bytes_dim, walk_bytes, walk_half, half_general, half_unkept,
// q_b (whether the call brought byte queries), bq_classes and rr_reserve -- nothing the sizing rule writes (hash_cap, hash_limit, vs_shr), so the layout is known before the visited set is sized.
WalkPlan plan_walk(const WalkParams& p, int metric, WalkPass pass, const WalkEnv& env = walk_env());

}  // namespace gbnns
