// jpeg_huff_wave.hpp -- jpeg_gen_optimal_table's merge loop by one wave (the lane-sized pieces are in
// jpeg_encode_progressive_core.hpp), for the kernels that build optimal tables on the device: the progressive coder's
// tables (csrc/jpeg_encode_progressive.hip) and the trellis stage's rate model (csrc/jpeg_trellis.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_encode_progressive_core.hpp"

namespace ifhip {

__device__ __forceinline__ uint64_t wave_min64(uint64_t k) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(static_cast<unsigned long long>(k), d, 64);
        k = o < k ? o : k;
    }
    return k;
}

// A workgroup of one wave; freq / codesize / others (LDS, 257 entries) as huff_init left them, synchronised.  Merges the two
// least frequent trees until one is left; the arrays are synchronised on return.
__device__ __forceinline__ void huff_wave_merge(uint32_t lane, uint32_t* freq, uint32_t* codesize, int32_t* others) {
    for (;;) {
        const uint64_t k1 = wave_min64(huff_lane_key(freq, lane, 0xFFFFFFFFu));
        const uint32_t c1 = huff_key_index(k1);
        const uint64_t k2 = wave_min64(huff_lane_key(freq, lane, c1));
        if (k2 == ~0ull) break;                            // (uniform) one tree left
        if (lane == 0u) huff_merge(c1, huff_key_index(k2), freq, codesize, others);
        __syncthreads();
    }
}

}  // namespace ifhip
