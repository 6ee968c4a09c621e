// tag_census.hip -- the census of a handle's tag table (gbnns_index_tag_census) and the small kernels of the routed tagged search built on it
// (gbnns_search_tagged_auto; lanes.cpp drives both).  For every query word Q[i]: allowed[i] = |{ j : (T[j] & Q[i]) != 0 }| and first[i] = the
// lowest such j (0xFFFFFFFF: none), exact.  Real batches carry a handful of distinct words, so the device work is n x U for the U DISTINCT
// words of the batch, never n x n_q:
//   1. census_dedupe_kernel   every query claims the slot of its word in an open-addressing table (64-bit slots: a used bit beside the word,
//                             so that every 32-bit value is a key) with atomicCAS and remembers the slot;
//   2. census_compact_kernel  the used slots become a list (word, slot) in any order -- results are per word -- and U, in device memory;
//   3. census_rows_kernel     a workgroup holds a tile of 1 024 tag words in registers (16-byte loads, 4 words a lane) and runs the U words
//                             over it: AND, compare, ballot; the ballot's population count adds to the wavefront's count, its lowest lane gives
//                             the candidate for `first`.  The four wavefronts' figures meet in LDS, a chunk of 256 words at a time, and one
//                             atomicAdd / atomicMin per (workgroup, word) with a hit goes to the slot's counters.  Integer sums and minima do
//                             not depend on arrival order: the result is exact and reproducible;
//   4. census_finish_kernel   every query reads the counters of its slot.
// No host round trip anywhere: U is read from device memory.  Every global write is an ordinary vector store or a vector atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace gbnns {

namespace {

constexpr uint32_t kCensusThreads = 256;                                  // four wavefronts
// 16-byte loads a lane.  Measured on an MI355X, 10^6 rows against 10^4 DISTINCT words (the worst case): 4 loads (4 096 rows a workgroup, one
// wavefront per SIMD) 4.0 ms, 2 loads 2.9 ms, 1 load 2.4 ms -- the word loop is a chain of scalar operations that a wavefront cannot hide
// from itself, so the smaller tile's four wavefronts per SIMD win; with 1 or 13 words the three are within 10 us of one another.  (Tiles
// kept over several word chunks, word chunks shared between workgroups, the per-word figures kept in registers by lane: measured too,
// no gain.)
constexpr uint32_t kCensusRegs = 1;
constexpr uint32_t kCensusTile = kCensusThreads * kCensusRegs * 4;        // 1 024 rows a workgroup
constexpr uint32_t kCensusChunk = 256;                                    // words between two meetings in LDS
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr unsigned long long kUsed = 1ull << 32;

__host__ __device__ inline uint32_t census_hash(uint32_t w) {
    w ^= w >> 16; w *= 0x7FEB352Du; w ^= w >> 15; w *= 0x846CA68Bu; w ^= w >> 16;
    return w;
}

// (the table holds at least 2 n_q slots and at most n_q keys: every probe sequence ends)
__global__ __launch_bounds__(256) void census_dedupe_kernel(const uint32_t* __restrict__ qtags, uint32_t nq, unsigned long long* table, uint32_t mask,
                                                           uint32_t* __restrict__ slot_of) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint32_t w = qtags[i];
    // (a batch of one tenant: the lanes that carry the word of the wavefront's first lane leave the claim to that lane)
    const int leader = __ffsll(__ballot(1)) - 1;
    const bool mine = w != (uint32_t)__shfl((int)w, leader) || (int)(threadIdx.x & 63u) == leader;
    const unsigned long long key = kUsed | w;
    uint32_t h = census_hash(w) & mask;
    while (mine) {
        const unsigned long long old = atomicCAS(&table[h], 0ull, key);
        if (old == 0ull || old == key) break;
        h = (h + 1) & mask;
    }
    const uint32_t h0 = (uint32_t)__shfl((int)h, leader);
    if (!mine) h = h0;
    slot_of[i] = h;
}

__global__ __launch_bounds__(256) void census_compact_kernel(const unsigned long long* __restrict__ table, uint64_t cap, uint32_t* __restrict__ words,
                                                            uint32_t* __restrict__ slots, uint32_t* u_count) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < cap; h += step) {
        const unsigned long long e = table[h];
        if (e == 0ull) continue;
        const uint32_t u = atomicAdd(u_count, 1u);
        words[u] = (uint32_t)e;
        slots[u] = (uint32_t)h;
    }
}

// Lane l of wavefront v holds, in register 4 r + e, the tag word of row tile0 + r * 1024 + v * 256 + l * 4 + e; the minimum over the ballots'
// lowest lanes, each taken as its row, is the wavefront's lowest allowed row.  Rows behind n read as 0, which no word allows.
__global__ __launch_bounds__(kCensusThreads) void census_rows_kernel(const uint32_t* __restrict__ tags, uint64_t n, const uint32_t* __restrict__ words,
                                                                    const uint32_t* __restrict__ slots, const uint32_t* __restrict__ u_count,
                                                                    uint32_t* count, uint32_t* first) {
    __shared__ uint32_t s_cnt[kCensusChunk][4], s_min[kCensusChunk][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t tile0 = (uint64_t)blockIdx.x * kCensusTile;
    uint32_t v[kCensusRegs * 4];
#pragma unroll
    for (uint32_t r = 0; r < kCensusRegs; ++r) {
        const uint64_t j = tile0 + ((uint64_t)r * kCensusThreads + threadIdx.x) * 4;
        if (j + 4 <= n) {
            const uint4 t = *reinterpret_cast<const uint4*>(tags + j);
            v[4 * r] = t.x; v[4 * r + 1] = t.y; v[4 * r + 2] = t.z; v[4 * r + 3] = t.w;
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) v[4 * r + e] = j + e < n ? tags[j + e] : 0u;
        }
    }
    const uint32_t U = *u_count;
    for (uint32_t u0 = 0; u0 < U; u0 += kCensusChunk) {
        const uint32_t m = min(kCensusChunk, U - u0);
        // the chunk's words, one per lane and register: a word then comes out of a register by its lane number, not out of memory
        uint32_t wv[kCensusChunk / 64];
#pragma unroll
        for (uint32_t q = 0; q < kCensusChunk / 64; ++q) wv[q] = q * 64 + lane < m ? words[u0 + q * 64 + lane] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < kCensusChunk / 64; ++q) {
            const uint32_t mq = q * 64 < m ? min(64u, m - q * 64) : 0u;
            for (uint32_t l = 0; l < mq; ++l) {   // (l, and with it the word, is the same in every lane of the workgroup)
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)wv[q], (int)l);
                uint32_t cnt = 0, lo = kNone;
#pragma unroll
                for (uint32_t r = 0; r < kCensusRegs; ++r) {
#pragma unroll
                    for (uint32_t e = 0; e < 4; ++e) {
                        const unsigned long long b = __ballot((v[4 * r + e] & w) != 0u);
                        cnt += (uint32_t)__popcll(b);
                        if (b) lo = min(lo, r * (kCensusThreads * 4) + wave * 256u + (uint32_t)(__ffsll(b) - 1) * 4u + e);
                    }
                }
                if (lane == 0) { s_cnt[q * 64 + l][wave] = cnt; s_min[q * 64 + l][wave] = lo; }
            }
        }
        __syncthreads();
        if (threadIdx.x < m) {
            const uint32_t c = threadIdx.x;
            const uint32_t sum = s_cnt[c][0] + s_cnt[c][1] + s_cnt[c][2] + s_cnt[c][3];
            if (sum) {
                const uint32_t lo = min(min(s_min[c][0], s_min[c][1]), min(s_min[c][2], s_min[c][3]));
                const uint32_t slot = slots[u0 + c];
                atomicAdd(&count[slot], sum);
                atomicMin(&first[slot], (uint32_t)tile0 + lo);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void census_finish_kernel(const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ count,
                                                           const uint32_t* __restrict__ first, uint32_t nq, uint32_t* __restrict__ out_allowed,
                                                           uint32_t* __restrict__ out_first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint32_t slot = slot_of[i];
    if (out_allowed) out_allowed[i] = count[slot];
    if (out_first) out_first[i] = first[slot];
}

// slots of the dedupe table for n_q queries: a power of two >= 2 n_q
uint64_t census_cap(uint64_t nq) {
    uint64_t cap = 64;
    while (cap < 2 * nq) cap <<= 1;
    return cap;
}

// ---- gbnns_search_tagged_auto ---------------------------------------------------------------------------------------------------------
// The routing rule on the device: query i scans when allowed[i] <= scan_below.  A scan-routed query walks with word 0 -- the walk gives it
// the bad-entry row at once --, and where the call names no entry points every query enters at the lowest row it may see.
__global__ __launch_bounds__(256) void route_kernel(const uint32_t* __restrict__ allowed, const uint32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ qtags, uint32_t nq, unsigned long long scan_below,
                                                   uint32_t* __restrict__ walk_tags, uint32_t* __restrict__ entries, uint32_t* __restrict__ out_allowed,
                                                   uint8_t* __restrict__ out_route) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint32_t a = allowed[i];
    const bool scan = (unsigned long long)a <= scan_below;
    walk_tags[i] = scan ? 0u : qtags[i];
    if (entries) entries[i] = first[i];
    if (out_allowed) out_allowed[i] = a;
    if (out_route) out_route[i] = scan ? 1 : 0;
}

// rows list[j] of `src` (rows of `row_units` units of type U) and their tag words, packed in list order
template <class U>
__global__ __launch_bounds__(256) void gather_kernel(const U* __restrict__ src, uint32_t row_units, const uint32_t* __restrict__ qtags,
                                                    const uint32_t* __restrict__ list, uint32_t m, U* __restrict__ dst, uint32_t* __restrict__ dst_tags) {
    const uint64_t total = (uint64_t)m * row_units, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        const uint32_t j = (uint32_t)(t / row_units), c = (uint32_t)(t % row_units);
        const uint32_t i = list[j];
        dst[t] = src[(uint64_t)i * row_units + c];
        if (c == 0) dst_tags[j] = qtags[i];
    }
}

// the scan's rows back to their queries: k-answer rows, and column 0 as the answer
__global__ __launch_bounds__(256) void scatter_kernel(const uint32_t* __restrict__ ids, const float* __restrict__ dist, const uint32_t* __restrict__ list,
                                                     uint32_t m, uint32_t k, uint32_t* __restrict__ top_ids, float* __restrict__ top_dist,
                                                     uint32_t* __restrict__ out_ids) {
    const uint64_t total = (uint64_t)m * k, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        const uint32_t j = (uint32_t)(t / k), c = (uint32_t)(t % k);
        const uint64_t o = (uint64_t)list[j] * k + c;
        const uint32_t id = ids[t];
        top_ids[o] = id;
        if (top_dist) top_dist[o] = dist[t];
        if (c == 0) out_ids[list[j]] = id;
    }
}

unsigned blocks_for(uint64_t threads) { return (unsigned)std::min<uint64_t>((threads + 255) / 256, 65536); }

}  // namespace

// Workspace of one census over n_q queries: the table, the per-slot counters, the queries' slots, the word list and U.
size_t tag_census_ws_bytes(uint64_t nq) { return (size_t)(census_cap(nq) * 16 + nq * 12 + 16); }

// Host only: the slots of the dedupe table of a census over nq queries, and the slot a word's probe sequence starts at (gbnns_debug_census_slot).
uint64_t tag_census_home_slot(uint32_t word, uint64_t nq, uint64_t* cap) {
    *cap = census_cap(nq);
    return census_hash(word) & (*cap - 1);
}

// T = tags [n] (16-byte aligned), Q = qtags [nq]; out_allowed / out_first [nq] or nullptr; everything device memory; ws: tag_census_ws_bytes(nq)
// bytes, 16-byte aligned.  Enqueued on s.
hipError_t launch_tag_census(const uint32_t* tags, uint64_t n, const uint32_t* qtags, uint32_t nq, void* ws, uint32_t* out_allowed,
                             uint32_t* out_first, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    if (!tags || !qtags || !ws || n == 0 || n >= 0xFFFFFFFFull || (reinterpret_cast<uintptr_t>(tags) & 15u) || (reinterpret_cast<uintptr_t>(ws) & 15u))
        return hipErrorInvalidValue;
    const uint64_t cap = census_cap(nq);
    unsigned long long* table = static_cast<unsigned long long*>(ws);
    uint32_t* count = reinterpret_cast<uint32_t*>(table + cap);
    uint32_t* first = count + cap;
    uint32_t* slot_of = first + cap;
    uint32_t* words = slot_of + nq;
    uint32_t* slots = words + nq;
    uint32_t* u_count = slots + nq;
    hipError_t e;
    if ((e = hipMemsetAsync(table, 0, cap * 12, s)) != hipSuccess) return e;   // the table and the counts
    if ((e = hipMemsetAsync(first, 0xFF, cap * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(u_count, 0, 4, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(census_dedupe_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, qtags, nq, table, (uint32_t)(cap - 1), slot_of);
    hipLaunchKernelGGL(census_compact_kernel, dim3(blocks_for(cap)), dim3(256), 0, s, table, cap, words, slots, u_count);
    hipLaunchKernelGGL(census_rows_kernel, dim3((unsigned)((n + kCensusTile - 1) / kCensusTile)), dim3(kCensusThreads), 0, s, tags, n, words, slots,
                       u_count, count, first);
    hipLaunchKernelGGL(census_finish_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, slot_of, count, first, nq, out_allowed, out_first);
    return hipGetLastError();
}

hipError_t launch_tag_route(const uint32_t* allowed, const uint32_t* first, const uint32_t* qtags, uint32_t nq, uint64_t scan_below, uint32_t* walk_tags,
                            uint32_t* entries, uint32_t* out_allowed, uint8_t* out_route, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(route_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, allowed, first, qtags, nq, (unsigned long long)scan_below, walk_tags, entries,
                       out_allowed, out_route);
    return hipGetLastError();
}

// rows list[0 .. m) of the queries ([. x d] float32, or uint8 with bytes != 0) and of qtags -> dst [m x d], dst_tags [m]
hipError_t launch_tag_gather(const void* queries, int bytes, uint32_t d, const uint32_t* qtags, const uint32_t* list, uint32_t m, void* dst,
                             uint32_t* dst_tags, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const unsigned blocks = blocks_for((uint64_t)m * d);
    if (bytes)
        hipLaunchKernelGGL(gather_kernel<uint8_t>, dim3(blocks), dim3(256), 0, s, static_cast<const uint8_t*>(queries), d, qtags, list, m,
                           static_cast<uint8_t*>(dst), dst_tags);
    else
        hipLaunchKernelGGL(gather_kernel<uint32_t>, dim3(blocks), dim3(256), 0, s, static_cast<const uint32_t*>(queries), d, qtags, list, m,
                           static_cast<uint32_t*>(dst), dst_tags);
    return hipGetLastError();
}

// ids / dist [m x k] (dist and top_dist: both or neither) -> rows list[j] of top_ids / top_dist, column 0 -> out_ids[list[j]]
hipError_t launch_tag_scatter(const uint32_t* ids, const float* dist, const uint32_t* list, uint32_t m, uint32_t k, uint32_t* top_ids, float* top_dist,
                              uint32_t* out_ids, hipStream_t s) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks_for((uint64_t)m * k)), dim3(256), 0, s, ids, dist, list, m, k, top_ids, dist ? top_dist : nullptr, out_ids);
    return hipGetLastError();
}

}  // namespace gbnns
