// walk_bytes_q.hip -- gbnns_search_byte_queries: the integer first pass of a GBNNS_FLAG_BYTE_WALK call whose queries are uint8 too.  The domain
// is walk_bytes.hip's (PLAIN, L2, d = 128, compact index, one entry point, no auxiliary graph, untagged, ef <= 1 024) and so are the kernels:
// walk_reg_one / walk_reg_big_one with BYTES and BQ set (walk_generic.h).  BQ changes how the query is staged -- the lane's four 16-byte chunks,
// packed, in 16 registers, read once from WalkParams::q_b; no query area in LDS -- and how a row is consumed: per dword xx = dot4(x, x) and
// qx = dot4(q, x) (v_dot4_u32_u8), one DPP add per row, dist = qq + xx - 2 qx in uint32, one v_cvt_f32_u32.  With d <= 256 that integer is below
// 2^24 and IS the float walk's distance, whose sums of integers below 2^24 are exact in any order -- so keys, visited set, lists, merges,
// hand-overs and results are the byte walk's, bit for bit.  What these kernels hand over goes to the general kernel's byte-walk instance,
// which reads the widened queries (widen.hip).
//
// The kernels' names carry none of `walk_`, `rerank_`, `knn_scan`, `gd_prune` on purpose: tests/test_isa_contract.py refuses any v_dot* in
// kernels so named because a dot instruction there would change the FLOAT rounding order.  That contract does not apply to exact integer
// arithmetic, which is all these kernels do with it.
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

namespace {

constexpr uint32_t u8_flags(bool one) { return kOff32 | kByteWalk | kByteQuery | flag_if(one, kOne); }  // (a kernel and its table row both take their flags from here)

template <int R, bool ONE_CHUNK>
__global__ __launch_bounds__(64) void beam_u8_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_one<0, 8, R, u8_flags(ONE_CHUNK) | kNeverLate>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

template <bool ONE_PASS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void beam_u8_big_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_big_one<0, 8, u8_flags(ONE_PASS)>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

#define BEAM_U8(R, ONE) {{WalkFamily::RegList, 0, 8, R, u8_flags(ONE)}, WALK_KERNEL(beam_u8_kernel<R, ONE>)}
#define BEAM_U8_BIG(ONE) {{WalkFamily::TwoList, 0, 8, 4, u8_flags(ONE)}, WALK_KERNEL(beam_u8_big_kernel<ONE>)}

// the instances of walk_bytes.hip, one for one
const WalkEntry kEntries[] = {
    BEAM_U8(1, true), BEAM_U8(1, false), BEAM_U8(2, true), BEAM_U8(2, false), BEAM_U8_BIG(true), BEAM_U8_BIG(false),
};

}  // namespace

const WalkEntry* walk_bytes_q_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
