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

// The scratch of the palette stages for a stage of up to max_images images.  The five blocks belong to the one owner of the
// stage that embeds this (StageScratch: all of a stage's blocks or none), which lists them and calls allocate() in its turn.
struct QuantScratch {
    uint32_t *d_tables = nullptr, *d_ekey = nullptr, *d_ew = nullptr, *d_result = nullptr;   // (the state words lie behind the tables)
    uint64_t* d_edmin = nullptr;
    size_t max_images = 0;
    int allocate(size_t n);             // for n images, one checked allocation per block: IFHIP_OK, or the status of the one that failed
    // A zeroed QuantArgs with the scratch, the batch's geometry and the bounds of speed 1..10, target 0..100 and minimum 0..target.
    void fill(QuantArgs* q, const uint8_t* images, size_t image_bytes, uint32_t stride, uint32_t w, uint32_t h, uint32_t n_images,
              int alpha_meaningful, uint32_t max_colors, uint32_t speed, uint32_t target, uint32_t minimum) const;
};

// The clear of the tables and state words of the images in use, the histogram launches (one per posterise level) and the
// palette launch: q.result then holds every image's palette.  Asynchronous on st.
int pq_launch_palette(const QuantArgs& q, hipStream_t st);

}  // namespace ifhip
