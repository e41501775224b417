// png_frame_device.hpp -- device code shared by the kernels that frame a zlib body of png_deflate.hip as an IDAT chunk:
// the finish kernels of the truecolour coder (png_encode.hip) and of the palette coder (png_quantize.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "png_deflate.hpp"
#include "png_encode_core.hpp"

namespace ifhip {

// XOR of v over the workgroup, valid in thread 0.  `scratch`: T / 64 dwords.
template <uint32_t T>
__device__ __forceinline__ uint32_t png_block_xor(uint32_t v, uint32_t* scratch) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v ^= __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (uint32_t w = 0; w < T / 64u; ++w) r ^= scratch[w];
    return r;
}

// The IDAT chunk around image img's body of `body` bytes, which lies (or is being copied) at idat + 10, and IEND behind
// it, by a workgroup of T lanes: the chunk's CRC is folded from the deflate chunks' CRCs, each shifted behind the bytes
// that follow it.  Returns the chunk's data size (lane 0 has written the CRC by then).  `scratch`: T / 64 dwords.
template <uint32_t T>
__device__ __forceinline__ uint32_t png_frame_idat(uint8_t* idat, uint32_t body, uint32_t adler, uint32_t zlib_header, const PngDeflateArgs& a, uint32_t img,
                                                   uint32_t* scratch) {
    const uint32_t tid = threadIdx.x, zlen = 2u + body + 4u;
    uint32_t crc = 0;
    for (uint32_t c = tid; c < a.n_chunks; c += T)
        crc ^= png_crc_shift(*chunk_word(a, kCrc, img, c), static_cast<uint64_t>(body) - *chunk_word(a, kOffset, img, c) - *chunk_word(a, kBytes, img, c) + 4u);
    if (tid == T - 1u) {                                     // the chunk type and the zlib header in front, the Adler-32 behind
        png_be32(idat, zlen);
        png_be32(idat + 4, kPngIDAT);
        idat[8] = static_cast<uint8_t>(zlib_header >> 8); idat[9] = static_cast<uint8_t>(zlib_header);
        png_be32(idat + 10u + body, adler);
        crc ^= png_crc_shift(png_crc32(idat + 4, 6), static_cast<uint64_t>(body) + 4u) ^ png_crc32(idat + 10u + body, 4);
    }
    crc = png_block_xor<T>(crc, scratch);
    if (tid == 0u) {
        png_be32(idat + 8u + zlen, crc);
        png_close_chunk(idat + 12u + zlen, kPngIEND, 0);
    }
    return zlen;
}

}  // namespace ifhip
