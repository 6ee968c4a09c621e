// rerank_plan.h -- which distance form re-ranks rows of a given length: the one place that decides it.  The launchers of rerank.hip,
// rerank_bytes.hip and rerank_half.hip pick their kernel from it, the pair kernels of rerank.hip their main loop, search_core.cpp whether a walk kernel may
// re-rank its own query (the fused re-rank runs the pair cores only), and gbnns_debug_rerank_plan reports it.  Host and device code, no
// device needed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gbnns {

enum class RerankForm : uint8_t {
    LanePerRow,   // metric_dist: a lane streams a row alone (float rows and byte rows)
    Pairs,        // rerank_pairs_core: two lanes share a float row
    ChunkPairs,   // rerank_bytes_core: two lanes share a byte row
    HalfChunkPairs,   // rerank_half_core: two lanes share a binary16 row (a half-base handle, gbnns_index_create_half_base)
};

struct RerankPlan {
    RerankForm form;
    // 16-byte row loads a lane has in flight in the first loop of its ladder: 24 (wide float rows, L2) or 8 in the pair form -- the template
    // argument DEEP of rerank_pairs_core --, 4 in the chunk-pair form, rerank_half_deep in the half chunk-pair form, 0 a lane per row (it
    // loads as it goes)
    int deep;
    // a search that walks another space may leave the re-rank to its walk kernels (fused_rerank: the pair cores); false: always a launch of its own
    bool fuses;
};

constexpr uint32_t kRerankDeepMinDim = 384;   // L2 rows from this length on: 24 loads in flight (GIST's 960; walk_common.h has the timing)

// DEEP of the float pair form at a length that takes it (the pair kernels of rerank.hip pick their core with it)
__host__ __device__ constexpr int rerank_pairs_deep(int metric, uint32_t dim) { return (metric == 0 && dim >= kRerankDeepMinDim) ? 24 : 8; }

// metric: 0 L2, 1 negative dot (GBNNS_METRIC_*).  bytes: the rows are a byte handle's.  dim == 0 is no row: a lane per row, never fused.
//   float rows: the pair form for both metrics at dim % 8 == 0, for L2 at dim % 8 == 4 too (the last 16-byte step is the even lane's alone)
//   byte rows:  the chunk-pair form for L2 at dim % 16 == 0
__host__ __device__ constexpr RerankPlan rerank_plan(int metric, uint32_t dim, bool bytes) {
    if (dim == 0) return {RerankForm::LanePerRow, 0, false};
    if (bytes) return (metric == 0 && dim % 16 == 0) ? RerankPlan{RerankForm::ChunkPairs, 4, true} : RerankPlan{RerankForm::LanePerRow, 0, false};
    if (dim % 8 == 0 || (metric == 0 && dim % 4 == 0))
        return {RerankForm::Pairs, rerank_pairs_deep(metric, dim), true};
    return {RerankForm::LanePerRow, 0, false};
}

// A half-base handle's rows (gbnns_index_create_half_base: binary16, round_up(dim, 8) halves, zero padded).  A 16-byte chunk is eight halves,
// two of the reference's 4-wide steps: the chunk-pair form serves L2 at every dim % 4 == 0 (dim % 8 == 4: the last chunk's second step is
// zero padding against a zero-staged query); the negative dot and L2 with a dim % 4 tail take a lane per row.  Never fused: no walk kernel
// reads such rows, a launch of rerank_half.hip always follows the first pass.
// DEEP of rerank_half_core: 16-byte loads a lane has in flight in the first loop of its ladder.  A half row has half the chunks of the float
// row, so the float core's 24 is not a given: tools/half_base_timing.py measured the ladder on the gist row (200 x 960: 60 chunks a lane) --
// 0.118 / 0.093 / 0.083 - 0.092 / 0.089 / 0.089 / 0.082 / 0.088 / 0.083 ms at 4 / 8 / 12 / 15 / 16 / 20 / 24 / 30, the float kernel 0.141 - 0.148;
// DESIGN.md section 5.1 "Half base rows" has the table.  (GBNNS_HALF_RERANK_DEEP: those experiment builds.)
#ifndef GBNNS_HALF_RERANK_DEEP
#define GBNNS_HALF_RERANK_DEEP 20
#endif
__host__ __device__ constexpr int rerank_half_deep(uint32_t dim) { return dim >= kRerankDeepMinDim ? GBNNS_HALF_RERANK_DEEP : 4; }
__host__ __device__ constexpr RerankPlan rerank_half_plan(int metric, uint32_t dim) {
    if (dim != 0 && metric == 0 && dim % 4 == 0) return {RerankForm::HalfChunkPairs, rerank_half_deep(dim), false};
    return {RerankForm::LanePerRow, 0, false};
}

// The fused re-rank of the generic wide-row walk instances and of the two-wavefront walk takes DEEP from the WALKED row (16-byte steps): wide walked
// rows are the wide original rows of GIST, and those instances have the registers for 24 loads.  The others run DEEP = 8 at every length.
constexpr int rerank_fused_deep(int walked_steps) { return walked_steps >= 12 ? 24 : 8; }

}  // namespace gbnns
