// walk_half_base.hip -- GBNNS_FLAG_HALF_WALK: first-pass PLAIN walks over the binary16 rows of a half-base handle (gbnns_index_create_half_base).
// The walked table is float32(db_half) -- every binary16 value is a binary32 value, widening rounds nothing -- and the walk is the reference's
// on it: float32 arithmetic in the reference's order (l2_ordered, walk_common.h), the query never rounded, no float copy of the table anywhere.
// The kernels here are walk_reg_one / walk_reg_big_one (walk_generic.h) with kHalfWalk set, which changes only where a hop's rows and the
// entry row come from and, for the long rows, how the distance consumes them:
//   STEPS = 24  d = 96 with L2 (deep's row, 192 bytes as halves): the pair form of the float instances -- a lane's share is six 16-byte loads,
//               kept packed until widen_row; the entry row is loaded the same way.  The two-list kernel re-reads the query from LDS every hop
//               (kQLds, as its half-rows twin), the register-list kernels keep it in registers (the register counts: DESIGN.md 5.1).
//   STEPS = 0   d >= 128, d % 4 == 0, L2 (sift's 128, glove's 300 in rows of 304 halves, gist's 960): the run-time-length walks with
//               l2_pair_rows_half (walk_lists.h) -- two lanes per row, 32 new rows per round, the chunk-pair arithmetic of the half re-rank.
// Visited set, lists, tie list, merge, hand-over and write_results are the float instances'.  There is no half-walk retry pass: what these
// hand over goes to the general kernel's half-walk instance (walk_general.hip), which also takes every flagged batch outside the domain
// (walk_plan.cpp).
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

namespace {

constexpr uint32_t hwalk_flags(bool one) { return kOff32 | kHalfWalk | flag_if(one, kOne); }  // (a kernel and its table row both take their flags from here)

template <int STEPS, int R, bool ONE_CHUNK>
__global__ __launch_bounds__(64) void walk_reg_hwalk_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_one<0, STEPS, R, hwalk_flags(ONE_CHUNK)>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

template <int STEPS, bool ONE_PASS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void walk_reg_big_hwalk_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_big_one<0, STEPS, hwalk_flags(ONE_PASS)>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

#define WALK_REG_HWALK(S, R, ONE) {{WalkFamily::RegList, 0, S, R, hwalk_flags(ONE)}, WALK_KERNEL(walk_reg_hwalk_kernel<S, R, ONE>)}
#define WALK_BIG_HWALK(S, ONE) {{WalkFamily::TwoList, 0, S, 4, hwalk_flags(ONE)}, WALK_KERNEL(walk_reg_big_hwalk_kernel<S, ONE>)}

const WalkEntry kEntries[] = {
    // 192-byte rows, the float path's instance set for 24 steps: one list register over one-pass and over two-pass adjacency rows, two list
    // registers over one-pass rows, the two-list kernel without and with the pass loop
    WALK_REG_HWALK(24, 1, true), WALK_REG_HWALK(24, 1, false), WALK_REG_HWALK(24, 2, true), WALK_BIG_HWALK(24, true), WALK_BIG_HWALK(24, false),
    // long rows, the float path's run-time-length set of a compact index's first pass: one list register (loop-free expansion over rows of
    // one 64-slot pass, and the pass loop), two list registers, the two-list kernel without and with the pass loop
    WALK_REG_HWALK(0, 1, true), WALK_REG_HWALK(0, 1, false), WALK_REG_HWALK(0, 2, false), WALK_BIG_HWALK(0, true), WALK_BIG_HWALK(0, false),
};

}  // namespace

const WalkEntry* walk_half_base_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
