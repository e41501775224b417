// png_deflate.hpp -- the deflate back end of the device PNG coders (png_deflate.hip): a filtered stream per image in, a
// zlib body per image out.  The truecolour coder (png_encode.hip) and the palette coder (png_quantize.hip) write the
// streams, say where the bodies land and frame them (png_frame_device.hpp); their stages embed the scratch's one owner.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "stage_scratch.hpp"

namespace ifhip {

struct PngDeflateArgs {
    uint8_t* streams;                   // the filtered streams, written by the coder's own kernel in front
    size_t stream_pitch;                // bytes between the streams of two images (a multiple of 16, 16 to spare)
    uint32_t stream_bytes, pitch, bpp;  // per image; `pitch`: bytes per row with its filter byte
    uint32_t n_chunks, n_images, stored_only;
    uint32_t* tokens;                   // [n_images][n_chunks][kPngChunk]
    uint32_t* counts;                   // [n_images][n_chunks][320]
    uint32_t* tabs;                     // [n_images][n_chunks][320]
    uint32_t* prefix;                   // [n_images][n_chunks][kPngPrefixWords]
    uint32_t* chunk;                    // [kChunkWords][n_images][n_chunks]: the per-chunk words below
    uint32_t* image;                    // [3][n_images]: total chunk bytes, Adler-32, overflow
    uint8_t* body;                      // image i's deflate blocks land at body + i * body_pitch when they are at most body_cap
    size_t body_pitch;                  // bytes; else the image's overflow word is set and nothing is written
    uint32_t body_cap;
};
enum { kNtok = 0, kAdler, kType, kPrefixBits, kBytes, kOffset, kCrc, kChunkWords };
__device__ __forceinline__ uint32_t* chunk_word(const PngDeflateArgs& a, uint32_t which, uint32_t img, uint32_t c) {
    return a.chunk + (static_cast<size_t>(which) * a.n_images + img) * a.n_chunks + c;
}
__device__ __forceinline__ size_t chunk_index(const PngDeflateArgs& a, uint32_t img, uint32_t c) { return static_cast<size_t>(img) * a.n_chunks + c; }

// match -> codes -> layout -> emit over a.streams: the size of image i's body in a.image[i], the stream's Adler-32 in
// a.image[n_images + i], "larger than a.body_cap" in a.image[2 * n_images + i], the chunk words in a.chunk.
void png_launch_deflate(const PngDeflateArgs& a, hipStream_t stream);

// The streams and the scratch of a stage of up to max_images images of one geometry.
struct PngDeflateScratch {
    uint32_t bpp = 0, pitch = 0, stream_bytes = 0, n_chunks = 0;
    size_t stream_pitch = 0;
    uint8_t* d_streams = nullptr;
    uint32_t *d_tokens = nullptr, *d_counts = nullptr, *d_tabs = nullptr, *d_prefix = nullptr, *d_chunk = nullptr, *d_image = nullptr;
    StageScratch blocks{&d_streams, &d_tokens, &d_counts, &d_tabs, &d_prefix, &d_chunk, &d_image};   // allocated by the first batch, behind the argument checks
    void shape(uint32_t width, uint32_t bytes_per_pixel, uint32_t height);   // (the caller has checked that the stream is below 2^31 bytes)
    size_t max_body_bytes() const { return static_cast<size_t>(stream_bytes) + 5u * n_chunks + 6u; }   // every chunk stored (+ 5), zlib header, Adler-32
    int allocate(uint32_t max_images);  // the first call allocates on the current device, later ones check that it still is the current one
    PngDeflateArgs args(uint32_t n_images, int zlib_level, uint8_t* body, size_t body_pitch, uint32_t body_cap) const;
};

}  // namespace ifhip
