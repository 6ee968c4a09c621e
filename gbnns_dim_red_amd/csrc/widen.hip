// widen.hip -- uint8 -> float32 for the queries of gbnns_search_byte_queries.  Every byte value is a binary32 value, so the widened copy IS
// float32(queries_u8): the projection, every walk, every re-rank and the general kernel run unchanged on it, which is what makes a byte-query
// call equal the float-query call bit for bit.  Only the integer byte-walk instances (walk_bytes_q.hip) read the bytes themselves.
#include "kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace gbnns {

namespace {

// four values a thread and step: byte loads (the source may start at any address), one 16-byte store (the destination is the lane's own
// buffer); the last, partial group is written value by value
__global__ __launch_bounds__(256) void widen_u8_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, size_t count) {
    const size_t groups = (count + 3) / 4, step = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += step) {
        const size_t i = 4 * g;
        if (i + 4 <= count) {
            const float4 v = make_float4((float)src[i], (float)src[i + 1], (float)src[i + 2], (float)src[i + 3]);
            *reinterpret_cast<float4*>(dst + i) = v;
        } else {
            for (size_t j = i; j < count; ++j) dst[j] = (float)src[j];
        }
    }
}

}  // namespace

hipError_t launch_widen_u8(const uint8_t* src, float* dst, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (!src || !dst || (reinterpret_cast<uintptr_t>(dst) & 15u)) return hipErrorInvalidValue;
    const size_t groups = (count + 3) / 4;
    const unsigned blocks = (unsigned)std::min<size_t>((groups + 255) / 256, 65536);
    hipLaunchKernelGGL(widen_u8_kernel, dim3(blocks), dim3(256), 0, s, src, dst, count);
    return hipGetLastError();
}

}  // namespace gbnns
