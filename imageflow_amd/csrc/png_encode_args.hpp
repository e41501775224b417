// png_encode_args.hpp -- what the kernels of png_encode.hip take, for the translation units that feed them a filtered
// stream: the truecolour coder itself (png_encode.hip) and the palette coder (png_quantize.hip), which writes its stream of
// one byte per pixel and hands it to the same match / codes / layout / emit kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ifhip {

struct PngArgs {
    const uint8_t* images;
    size_t image_bytes;
    uint32_t stride, w, h, bpp, pitch, color_type;
    uint32_t stream_bytes, n_chunks;    // per image
    size_t stream_pitch;                // bytes between the filtered streams of two images (a multiple of 16, 16 to spare)
    uint8_t* streams;
    uint32_t* tokens;                   // [n_images][n_chunks][kPngChunk]
    uint32_t* counts;                   // [n_images][n_chunks][320]
    uint32_t* tabs;                     // [n_images][n_chunks][320]
    uint32_t* prefix;                   // [n_images][n_chunks][kPngPrefixWords]
    uint32_t* chunk;                    // [kChunkWords][n_images][n_chunks]: the per-chunk words below
    uint32_t* image;                    // [3][n_images]: total chunk bytes, Adler-32, overflow
    uint32_t n_images, stored_only, zlib_header;
    uint8_t* files;
    size_t file_pitch;
    uint32_t* lengths;
    uint32_t* status_out;
};
enum { kNtok = 0, kAdler, kType, kPrefixBits, kBytes, kOffset, kCrc, kChunkWords };
__device__ __forceinline__ uint32_t* chunk_word(const PngArgs& a, uint32_t which, uint32_t img, uint32_t c) {
    return a.chunk + (static_cast<size_t>(which) * a.n_images + img) * a.n_chunks + c;
}
__device__ __forceinline__ size_t chunk_index(const PngArgs& a, uint32_t img, uint32_t c) { return static_cast<size_t>(img) * a.n_chunks + c; }

// match -> codes -> layout -> emit over a.streams (a.bpp, a.pitch, a.stream_bytes, a.n_chunks, a.n_images): the zlib body of
// image i lands at a.files + i * a.file_pitch + kPngHeadBytes + 10, its size in a.image[i], its Adler-32 in
// a.image[n_images + i], "does not fit a.file_pitch" in a.image[2 * n_images + i], the chunk words in a.chunk.
void png_launch_deflate(const PngArgs& a, hipStream_t stream);

}  // namespace ifhip
