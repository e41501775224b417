// jpeg_encode_progressive.hpp -- what csrc/jpeg_encode.hip (the stage and its C entry points) needs of
// csrc/jpeg_encode_progressive.hip (the kernels of the optimised-table and progressive forms and their scratch).
#pragma once
#include <cstddef>
#include <cstdint>

#include "jpeg_encode_core.hpp"

namespace ifhip {

struct ProgScratch;

struct ProgCall {
    const int16_t* coef[3];
    size_t plane_blocks[3];
    uint32_t n_images;
    const uint8_t* d_header;        // the baseline marker segments of the call's quality (SOI .. SOF are taken from them)
    uint8_t* files;
    size_t file_pitch;
    uint32_t* lengths;
    uint32_t* status_out;
};

// The scratch of both flagged forms for up to max_images images (allocated on the current device).
int prog_scratch_create(ProgScratch** out, const EncGeom& g, uint32_t width, uint32_t height, uint32_t max_images, size_t scan_capacity);
void prog_scratch_destroy(ProgScratch* s);
int prog_scratch_check_device(const ProgScratch* s);
// Arithmetic: no file of these flags is longer (0: the geometry is refused -- more than 2^32 bit positions).
size_t prog_max_file_bytes(const EncGeom& g, uint32_t width, uint32_t height, int flags, size_t scan_capacity);
int prog_encode(ProgScratch* s, const ProgCall& call, int flags, void* hip_stream);

}  // namespace ifhip
