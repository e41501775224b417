// vp8_encode_args.hpp -- what the kernels of the device lossy WebP coder are launched with: csrc/vp8_encode.hip (the six
// launches of a batch) and csrc/vp8_encode_intra4.hip (the code kernel of a stage with IFHIP_VP8_ENC_INTRA4) share it.
#pragma once
#include <hip/hip_runtime.h>

#include "vp8_encode_core.hpp"

namespace ifhip {

constexpr uint32_t kVp8eWaves = 8u;              // waves of the one workgroup an image's wavefront runs in
constexpr uint32_t kVp8eCountWords = 2u * kVp8eProbs + 8u;       // branch counts, then [0] skipped macroblocks, [1] any alpha below 255
constexpr uint32_t kVp8eProbBytes = 2u * kVp8eProbs + 16u;       // probabilities, update flags, then the skip probability
constexpr uint32_t kVp8eStreams = 9u;            // the first partition and at most eight token partitions

struct Vp8eArgs {
    const uint8_t* images;
    size_t image_bytes;
    uint32_t stride, w, h, mbw, mbh, alpha, n_images;
    Vp8eParams p;
    const Vp8eTables* T;
    uint8_t* planes;                    // [n][6 planes]: source Y, U, V and reconstruction Y, U, V, 768 bytes a macroblock
    uint32_t* grey;                     // [n][h * w] (null without alpha)
    Vp8Mb* mbs;                         // [n][mbw * mbh]
    int16_t* levels;                    // [n][mbw * mbh][400]
    uint32_t* counts;                   // [n][kVp8eCountWords], zeroed per batch
    uint8_t* probs;                     // [n][kVp8eProbBytes]
    uint8_t* streams;                   // [n][stream_pitch]: the first partition's room, then each token partition's
    size_t stream_pitch;
    uint32_t first_cap, part_cap;
    uint32_t* stream_len;               // [n][kVp8eStreams]
    const uint8_t* inner_files;         // the inner lossless coder's files of the grey frames
    size_t inner_pitch;
    const uint32_t *inner_len, *inner_status;
    uint8_t* files;
    size_t file_pitch;
    uint32_t *lengths, *status_out;
    uint32_t flags;                     // kVp8eIntra4
};

__device__ __forceinline__ size_t vp8e_mb_count(const Vp8eArgs& a) { return static_cast<size_t>(a.mbw) * a.mbh; }
__device__ __forceinline__ Vp8Planes vp8e_planes(const Vp8eArgs& a, uint32_t img, bool rec) {
    const size_t n = vp8e_mb_count(a);
    uint8_t* base = a.planes + (static_cast<size_t>(img) * 2u + (rec ? 1u : 0u)) * n * 384u;
    return Vp8Planes{base, base + n * 256u, base + n * 320u, a.mbw * 16u, a.mbw * 8u, a.mbw, a.mbh};
}

// csrc/vp8_encode_intra4.hip: vp8e_code4_kernel in vp8e_code_kernel's place, one workgroup per image
void vp8e_launch_code4(const Vp8eArgs& a, hipStream_t stream);

}  // namespace ifhip
