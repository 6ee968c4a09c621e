// walk_bytes.hip -- GBNNS_FLAG_BYTE_WALK: first-pass PLAIN walks over the uint8 rows of a byte handle (gbnns_index_create_bytes).  The walked
// table is float32(db_bytes) -- every byte value is a binary32 value, widening rounds nothing -- and the walk is the reference's on it:
// float32 arithmetic in the reference's order (l2_ordered, walk_common.h), no float copy of the table anywhere.  The kernels here are
// walk_reg_one / walk_reg_big_one (walk_generic.h) with BYTES set, which changes only where a hop's rows (and the entry row) come from and how
// the distance consumes them: L2 over rows of d = 128 = eight 16-byte chunks, two lanes per neighbour, the even lane the chunks 0, 2, 4, 6
// and the odd lane 1, 3, 5, 7 -- four 16-byte loads per lane, all in flight, kept packed (16 registers) until byte_chunk_add widens and
// consumes them chunk by chunk; the 128-float query lives in LDS and is re-read every hop in the shadow of the row loads.  Visited set,
// lists, tie list, merge, hand-over and write_results are the float instances'.  There is no byte-walk retry pass: what these hand over goes
// to the general kernel's byte-walk instance (walk_general.hip), which also takes every flagged batch outside the domain (walk_plan.cpp).
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

namespace {

constexpr uint32_t bytes_flags(bool one) { return kOff32 | kByteWalk | flag_if(one, kOne); }  // (a kernel and its table row both take their flags from here)

template <int R, bool ONE_CHUNK>
__global__ __launch_bounds__(64) void walk_reg_bytes_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_one<0, 8, R, bytes_flags(ONE_CHUNK) | kNeverLate>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

template <bool ONE_PASS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void walk_reg_big_bytes_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_big_one<0, 8, bytes_flags(ONE_PASS)>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

#define WALK_REG_BYTES(R, ONE) {{WalkFamily::RegList, 0, 8, R, bytes_flags(ONE)}, WALK_KERNEL(walk_reg_bytes_kernel<R, ONE>)}
#define WALK_BIG_BYTES(ONE) {{WalkFamily::TwoList, 0, 8, 4, bytes_flags(ONE)}, WALK_KERNEL(walk_reg_big_bytes_kernel<ONE>)}

// one / two list registers and the two-list kernel, each over one-pass adjacency rows (no pass loop) and with the pass loop
const WalkEntry kEntries[] = {
    WALK_REG_BYTES(1, true), WALK_REG_BYTES(1, false), WALK_REG_BYTES(2, true), WALK_REG_BYTES(2, false), WALK_BIG_BYTES(true), WALK_BIG_BYTES(false),
};

}  // namespace

const WalkEntry* walk_bytes_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
