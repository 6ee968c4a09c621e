// walk_half.hip -- GBNNS_FLAG_HALF_ROWS: first-pass walks whose hops gather the walked rows from a 2-byte table.  The walked table is
// R = float32(float16(db_low)) -- every coordinate rounded once to nearest-even binary16 and widened back, which is exact -- and a search
// with half rows is the reference's search on R: float32 arithmetic in the reference's order, the query never rounded.  The kernels here are
// walk_reg_one / walk_reg_big_one (walk_generic.h) with HALF set, which changes only where a lane's row pieces come from: 16-byte (negative
// dot: 8-byte) pieces of the binary16 row, kept packed until the distance widens them (v_cvt_f32_f16) into the very float4 pieces the
// float32 pair form loads.  Visited set, lists, merge, hand-over and the fused re-rank are the float32 instances'; the retry pass, the
// general kernel and every instance outside half_serves (walk_plan.cpp) read the float32 copy of R instead.  Also the conversion kernel
// that builds both tables from db_low.
#include "launch_util.h"
#include "walk_generic.h"

#include <hip/hip_fp16.h>

#include <algorithm>

namespace gbnns {

namespace {

constexpr uint32_t half_flags(bool one, bool late = false) { return kOff32 | kHalf | flag_if(one, kOne) | flag_if(late, kLate); }  // (a kernel and its table row both take their flags from here)

template <int METRIC, int STEPS, int R, bool ONE_CHUNK>
__global__ __launch_bounds__(64) void walk_reg_half_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_one<METRIC, STEPS, R, half_flags(ONE_CHUNK)>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

template <int METRIC, int STEPS, bool ONE_PASS, bool LATE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void walk_reg_big_half_kernel(WalkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    walk_reg_big_one<METRIC, STEPS, half_flags(ONE_PASS, LATE)>(p, walk_query_of(p, blockIdx.x), smem, p.ovf_count, p.ovf_list);
}

// float32 -> binary16 (round to nearest even, subnormals kept) and back: one thread per coordinate of the 2-byte table, whose rows are
// hstride >= fstride halves (zero padded).  A coordinate that is not finite or rounds out of the binary16 range reports its row.
__global__ __launch_bounds__(256) void half_rows_convert_kernel(const float* src, uint32_t sstride, uint32_t dim, uint64_t n, unsigned short* out_h,
                                                                uint32_t hstride, float* out_f, uint32_t fstride, uint32_t* bad_row) {
    const uint64_t total = n * hstride;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        const uint64_t row = i / hstride;
        const uint32_t col = (uint32_t)(i - row * hstride);
        const float v = col < dim ? src[row * sstride + col] : 0.f;
        if (!(__builtin_fabsf(v) < 65520.f)) atomicMin(bad_row, (uint32_t)row);  // (NaN compares false)
        const __half h = __float2half_rn(v);
        out_h[i] = __half_as_ushort(h);
        if (col < fstride) out_f[row * fstride + col] = __half2float(h);
    }
}

#define WALK_REG_HALF(M, S, R, ONE) {{WalkFamily::RegList, M, S, R, half_flags(ONE)}, WALK_KERNEL(walk_reg_half_kernel<M, S, R, ONE>)}
#define WALK_BIG_HALF(M, S, ONE, LATE) {{WalkFamily::TwoList, M, S, 4, half_flags(ONE, LATE)}, WALK_KERNEL(walk_reg_big_half_kernel<M, S, ONE, LATE>)}
// one list register (loop-free expansion over one-pass adjacency rows, and the pass loop), two list registers, the two-list kernel
#define WALK_HALF_SET(M, S) \
    WALK_REG_HALF(M, S, 1, true), WALK_REG_HALF(M, S, 1, false), WALK_REG_HALF(M, S, 2, false), WALK_BIG_HALF(M, S, true, false), WALK_BIG_HALF(M, S, false, false)

const WalkEntry kEntries[] = {
    WALK_HALF_SET(0, 8),  WALK_HALF_SET(1, 8), WALK_HALF_SET(0, 12), WALK_HALF_SET(0, 16),
    // 576-byte rows (288 as halves): the two-list kernel only, rows requested before / after the visited test
    WALK_BIG_HALF(0, 36, true, false), WALK_BIG_HALF(0, 36, false, false), WALK_BIG_HALF(0, 36, true, true), WALK_BIG_HALF(0, 36, false, true),
};

}  // namespace

const WalkEntry* walk_half_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

hipError_t launch_half_rows_convert(const float* src, uint32_t sstride, uint32_t dim, uint64_t n, uint16_t* out_h, uint32_t hstride, float* out_f,
                                    uint32_t fstride, uint32_t* bad_row, hipStream_t s) {
    if (n == 0 || hstride == 0) return hipSuccess;
    const uint64_t blocks = (n * hstride + 255u) / 256u;
    hipLaunchKernelGGL(half_rows_convert_kernel, dim3((unsigned)std::min<uint64_t>(blocks, 1u << 20)), dim3(256), 0, s, src, sstride, dim, n,
                       reinterpret_cast<unsigned short*>(out_h), hstride, out_f, fstride, bad_row);
    return hipGetLastError();
}

}  // namespace gbnns
