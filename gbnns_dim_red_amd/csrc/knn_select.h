// knn_select.h -- the selection half of the exact kNN units (knn.hip: float rows; knn_bytes.hip: uint8 rows): the
// order-preserving distance keys, the binary heap of short lists and the radix select of long ones.  Device code shared
// by inclusion; both units hold (distance key << 32 | id) keys of the same form, so they select with the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gbnns {

namespace {

__device__ __forceinline__ uint32_t knn_fkey(float x) {  // order-preserving map float -> u32 (-0 == +0)
    x = x + 0.0f;
    const uint32_t b = __float_as_uint(x);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float knn_fkey_inv(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    return __uint_as_float(b);
}

// Replaces the root of the max-heap h[0..k) (stride `st` elements between levels) by `key` and restores the
// heap; returns the new root.
__device__ __forceinline__ uint64_t heap_replace_root(uint64_t* h, size_t st, int k, uint64_t key) {
    int i = 0;
    while (true) {
        const int l = 2 * i + 1;
        if (l >= k) break;
        uint64_t cv = h[(size_t)l * st];
        int c = l;
        if (l + 1 < k) {
            const uint64_t cr = h[(size_t)(l + 1) * st];
            if (cr > cv) { cv = cr; c = l + 1; }
        }
        if (cv <= key) break;
        h[(size_t)i * st] = cv;
        i = c;
    }
    h[(size_t)i * st] = key;
    return h[0];
}

constexpr int kPoolNew = 1024;  // appended keys per selection round

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, d);
        v += lane >= d ? t : 0u;
    }
    return v;
}

// k-th smallest (1-based) of keys[0 .. M), M > k; afterwards keys[0 .. k) hold the k smallest (any order; all-ones keys
// are "no entry" and may repeat, every other key is distinct).  Returns the largest of them.
__device__ __forceinline__ uint64_t pool_select(uint64_t* keys, int k, int M, uint32_t* hist, int lane) {
    uint64_t prefix = 0, mask = 0;
    uint32_t need = (uint32_t)k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int j = lane; j < 256; j += 64) hist[j] = 0u;
        __syncthreads();
        for (int i = lane; i < M; i += 64) {
            const uint64_t key = keys[i];
            if ((key & mask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        const uint32_t sum = c0 + c1 + c2 + c3;
        const uint32_t incl = wave_incl_scan_u32(sum, lane), excl = incl - sum;
        const bool has = excl < need && need <= incl;  // exactly one lane
        const uint32_t r = need - excl;
        uint32_t b = 3, below = c0 + c1 + c2, cb = c3;
        if (r <= c0) { b = 0; below = 0; cb = c0; }
        else if (r <= c0 + c1) { b = 1; below = c0; cb = c1; }
        else if (r <= c0 + c1 + c2) { b = 2; below = c0 + c1; cb = c2; }
        const int src = __ffsll((unsigned long long)__ballot(has)) - 1;
        const uint32_t bin = (uint32_t)__shfl((int)(4u * (uint32_t)lane + b), src);
        const uint32_t skipped = (uint32_t)__shfl((int)(excl + below), src);
        const uint32_t in_bin = (uint32_t)__shfl((int)cb, src);
        need -= skipped;
        prefix |= (uint64_t)bin << shift;
        mask |= 255ull << shift;
        if (in_bin == 1u) break;
    }
    uint64_t tau = prefix;  // every digit fixed (only all-ones keys repeat), or: the one key under the prefix
    if (mask != ~0ull) {
        uint64_t found = 0;
        for (int i = lane; i < M; i += 64) {
            const uint64_t key = keys[i];
            if ((key & mask) == prefix) found = key;
        }
        const int src = __ffsll((unsigned long long)__ballot(found != 0)) - 1;  // (a key is never 0: distance keys have a bit set)
        tau = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(found >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)found, src);
    }
    int c = 0;  // keys below tau to the front, in place (a key moves to a position at or below its own)
    for (int i0 = 0; i0 < M; i0 += 64) {
        const int i = i0 + lane;
        const uint64_t key = i < M ? keys[i] : ~0ull;
        const bool keep = i < M && key < tau;
        const uint64_t m = __ballot(keep);
        const int pos = c + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        __syncthreads();
        if (keep) keys[pos] = key;
        c += __popcll(m);
        __syncthreads();
    }
    for (int i = c + lane; i < k; i += 64) keys[i] = tau;  // the k-th itself (all-ones: every free place)
    __syncthreads();
    return tau;
}

}  // namespace

}  // namespace gbnns
