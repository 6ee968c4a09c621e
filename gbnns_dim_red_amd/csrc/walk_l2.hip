// walk_l2.hip -- the L2 walks over generic and 128-byte rows, and the one launch path of every walk pass: launch_walk looks the plan's
// instance (walk_plan.h) up in the units' tables and launches it on the LDS of the plan's layout.  Also the visited-set forms' byte counts.
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

static const WalkEntry kEntries[] = {
    WALK_GENERIC_SET(0, 8),
    WALK_GENERIC_SET(0, 0),
};
const WalkEntry* walk_l2_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

// Visited set of `entries` ids: 4-byte slots in 4-slot buckets; the hot kernel packs five 24-bit ids and a
// counter byte into each 16-byte bucket (3.2 bytes per id).
// The quotient form (hot first pass, small enough n: GBNNS_VS_ASM) packs seven 16-bit entries per bucket (2.29 bytes per id).
size_t walk_hash_bytes(uint32_t entries, int form) {
    return form == 2 ? (size_t)(entries / 7u) * 16 : form == 1 ? (size_t)(entries / 5u) * 16 : (size_t)entries * 4;
}
uint32_t walk_hash_entries(size_t bytes, int form) {
    return form == 2 ? (uint32_t)(bytes / 16) * 7u : form == 1 ? (uint32_t)(bytes / 16) * 5u : ((uint32_t)(bytes / 4) & ~3u);
}

static const WalkEntry* walk_entry(const WalkInstance& k) {
    for (auto unit : {walk_hot_entry, walk_l2_entry, walk_dot_entry, walk_wide_entry, walk_wide2_entry, walk_wide3_entry, walk_coop_entry, walk_bitmap_entry, walk_half_entry, walk_tag_entry, walk_bridge_entry, walk_bytes_entry, walk_bytes_q_entry, walk_half_base_entry})
        if (const WalkEntry* e = unit(k)) return e;
    return nullptr;
}

const char* walk_plan_name(const WalkPlan& pl) { const WalkEntry* e = walk_entry(pl.inst); return e ? e->name : nullptr; }

// Host function of the last first-pass walk kernel this thread launched (profiling: gbnns_profile.walk_kernel)
static thread_local const void* g_walk_first_fn = nullptr;
const char* walk_first_pass_name(hipStream_t s) {
    return g_walk_first_fn ? hipKernelNameRefByPtr(g_walk_first_fn, s) : nullptr;
}
// ... and of the last retry-pass kernel (gbnns_profile.retry_kernel)
static thread_local const void* g_walk_retry_fn = nullptr;
const char* walk_retry_pass_name(hipStream_t s) {
    return g_walk_retry_fn ? hipKernelNameRefByPtr(g_walk_retry_fn, s) : nullptr;
}

// First pass: a workgroup per query (the two-wavefront walk: of two wavefronts); retry: a wavefront per CU; bitmap pass: `slots` wavefronts, no LDS visited set
hipError_t launch_walk(const WalkPlan& pl, const WalkParams& p, unsigned slots, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    const WalkEntry* e = walk_entry(pl.inst);
    if (!e) return hipErrorInvalidValue;  // never another instance in its place: the LDS is laid out for this one
    const bool bitmap = pl.pass == WalkPass::Bitmap, retry = pl.pass == WalkPass::Retry;
    const size_t lds = pl.lds_fixed + (bitmap ? 0 : walk_hash_bytes(p.hash_cap, pl.hash_form(p.vs_shr)));
    const hipError_t err = set_lds(e->fn, lds);
    if (err != hipSuccess) return err;
    (retry ? g_walk_retry_fn : g_walk_first_fn) = e->fn;
    void* args[] = {const_cast<WalkParams*>(&p)};
    (void)hipLaunchKernel(e->fn, dim3(bitmap ? slots : retry ? (unsigned)kRetrySlots : p.nq), dim3(pl.inst.family == WalkFamily::Coop ? 128 : 64), args, lds, s);
    return hipGetLastError();
}

}  // namespace gbnns
