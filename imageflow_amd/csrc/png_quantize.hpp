// png_quantize.hpp -- what the palette stages of csrc/png_quantize.hip take and leave, for the coders that quantise with
// them: the palette PNG coder itself and the GIF coder (csrc/gif_encode.hip).  The kernels stay in png_quantize.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "png_quantize_core.hpp"

namespace ifhip {

constexpr uint32_t kPqStateWords = 16;       // per image: overflow[kPqLevels], entries[kPqLevels]
constexpr uint32_t kPqResultWords = 8 + kPqMaxColors;   // count, transparent entries, too low, level, entries, -, error (2 words), keys in file order

struct QuantArgs {
    const uint8_t* images;
    size_t image_bytes;
    uint32_t stride, w, h, n_images;
    uint32_t alpha, max_colors, dither, iterations, max_entries, zlib_header;
    uint32_t key_rule;                  // kPqKeyPng (what a memset leaves) or kPqKeyGif
    uint64_t bound_target, bound_min;
    uint32_t* tables;                   // [n_images][kPqLevels][2][kPqSlots]: slots, counts
    uint32_t* state;                    // [n_images][kPqStateWords]
    uint32_t *ekey, *ew;                // [n_images][kPqMaxEntries]: the packed histogram
    uint64_t* edmin;                    // [n_images][kPqMaxEntries]: distance to the nearest entry so far
    uint32_t* result;                   // [n_images][kPqResultWords]
    uint8_t* palettes;                  // taps (nullable)
    uint8_t* indices;
    double* mse;
    uint8_t* files;
    size_t file_pitch;
    uint32_t* lengths;
    uint32_t* status_out;
};

inline size_t quant_table_words(size_t n) { return n * kPqLevels * 2u * kPqSlots; }

// The clear of the tables and state words of the images in use, the histogram launches (one per posterise level) and the
// palette launch: q.result then holds every image's palette.  Asynchronous on st.
int pq_launch_palette(const QuantArgs& q, hipStream_t st);

}  // namespace ifhip
