// walk_tag.hip -- gbnns_search_tagged: first-pass walks restricted to the rows a query may see.  Row j carries a 32-bit tag word T[j], query i a
// word Q[i]; j is allowed for i when (T[j] & Q[i]) != 0, and a tagged search of query i is the reference's search on the graph whose adjacency
// rows keep the allowed neighbours only, in their order.  The kernels here are walk_reg_one / walk_reg_big_one (walk_generic.h) with TAG set:
// a hop loads the tag word of every live adjacency slot -- ahead of the rows, which the one-chunk / one-pass instances issue beside them
// (walk_generic.h says what each class of instance compiles to) -- and treats a disallowed slot as an empty one from there on; the end of an adjacency row is still decided before the tag test.  The entry row enters untested, as in the
// reference; a query whose entry it may not see gets the row of an entry id outside the index.  Visited set, lists, merge, hand-over and the
// fused re-rank are the untagged instances'.  There is no tagged retry pass: what the first pass hands over goes to the general kernel, whose
// tagged instance (walk_general.hip) also takes every batch outside the domain below.
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

namespace {

constexpr uint32_t tag_flags(bool one, bool late = false) { return kOff32 | kTag | flag_if(one, kOne) | flag_if(late, kLate); }  // (a kernel and its table row both take their flags from here)

// (kNeverLate: the rows always requested before the visited test -- with both orders in one kernel the wait ahead of the tag test covers the rows too)
template <int METRIC, int STEPS, int R, bool ONE_CHUNK>
__global__ __launch_bounds__(64) void walk_reg_tag_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_one<METRIC, STEPS, R, tag_flags(ONE_CHUNK) | kNeverLate>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

template <int METRIC, int STEPS, bool ONE_PASS, bool LATE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void walk_reg_big_tag_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_big_one<METRIC, STEPS, tag_flags(ONE_PASS, LATE)>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

#define WALK_REG_TAG(M, S, R, ONE) {{WalkFamily::RegList, M, S, R, tag_flags(ONE)}, WALK_KERNEL(walk_reg_tag_kernel<M, S, R, ONE>)}
#define WALK_BIG_TAG(M, S, ONE, LATE) {{WalkFamily::TwoList, M, S, 4, tag_flags(ONE, LATE)}, WALK_KERNEL(walk_reg_big_tag_kernel<M, S, ONE, LATE>)}
// one list register (loop-free expansion over one-pass adjacency rows, and the pass loop), two list registers, the two-list kernel
#define WALK_TAG_SET(M, S) \
    WALK_REG_TAG(M, S, 1, true), WALK_REG_TAG(M, S, 1, false), WALK_REG_TAG(M, S, 2, false), WALK_BIG_TAG(M, S, true, false), WALK_BIG_TAG(M, S, false, false)

const WalkEntry kEntries[] = {
    WALK_TAG_SET(0, 8),  WALK_TAG_SET(1, 8), WALK_TAG_SET(0, 12), WALK_TAG_SET(0, 16),
    // 576-byte rows: the two-list kernel only, rows requested before / after the visited test
    WALK_BIG_TAG(0, 36, true, false), WALK_BIG_TAG(0, 36, false, false), WALK_BIG_TAG(0, 36, true, true), WALK_BIG_TAG(0, 36, false, true),
};

}  // namespace

const WalkEntry* walk_tag_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
