// block_scan.hpp -- the exclusive prefix sum of one dword per lane over a workgroup, for the kernels that turn a running
// bit or byte position into count -> scan -> write (jpeg_encode.hip, png_deflate.hip, webp_encode.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ifhip {

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= static_cast<uint32_t>(d)) v += u;
    }
    return v;
}

// exclusive scan over the T lanes of a workgroup (T a multiple of 64, <= 1024); *total = the sum.  `scratch`: T / 64 dwords.
template <uint32_t T>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* scratch, uint32_t* total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t incl = wave_inclusive_scan(v, lane);
    __syncthreads();                                       // (scratch may still be read from a previous call)
    if (lane == 63u) scratch[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < T / 64u; ++w) {
        const uint32_t t = scratch[w];
        if (w < wave) before += t;
        sum += t;
    }
    *total = sum;
    return before + incl - v;
}

}  // namespace ifhip
