// knn_scan_dist.h -- the distance half of the narrow exact-scan kernels (knn.hip: knn_scan_kernel; knn_gather.hip: knn_gather_kernel): the
// distances of ONE staged base row to the QPT queries a thread holds in registers, in the reference's own arithmetic (L2Metric::Dist /
// Angular::Dist, support_func.h:107-163: same running sums, same order, one rounding per operation).  Device code shared by inclusion, so
// that the two kernels cannot drift apart: whoever stages the row -- the table in order, or rows picked through an id list -- the operations
// per distance and their order are these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gbnns {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kKnnThreads = 128;
constexpr int kKnnTile = 64;  // base rows per LDS tile

// The loop itself is knn_scan_row.inc, included as text inside both kernels' row loops: the compiler then sees in knn_scan_kernel the very
// statements it saw before the loop was shared (an inlined function gave the same sums with the operands of some additions swapped).

}  // namespace

}  // namespace gbnns
