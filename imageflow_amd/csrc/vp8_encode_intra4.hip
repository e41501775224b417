// vp8_encode_intra4.hip -- the code kernel of a lossy WebP stage with IFHIP_VP8_ENC_INTRA4: vp8e_code_kernel's work plus, per
// macroblock, the trial of the sixteen 4x4 luma sub-blocks with their ten modes, and B_PRED where that is cheaper.
// The other five launches of a batch are csrc/vp8_encode.hip's, which learn the B_PRED macroblock from its record.
//
// ONE WORKGROUP OF 8 WAVES PER IMAGE.  A 4x4 sub-block in a macroblock's last column predicts from the bottom row of the
// macroblock above and to the RIGHT, so the skew is 2, as in the decoder's vp8_predict_kernel: macroblock (x, y) runs in step
// x + 2y, the macroblocks of a step dealt to the waves, a workgroup barrier between steps (mbw + 2 (mbh - 1) of them).
// Inside a wave (vp8e_code_mb4): the 16x16 and the chroma trials as in vp8e_code_kernel; then the ten anti-diagonals
// bx + 2 by of the sub-blocks, the (sub-block, mode) pairs of one -- twenty at most -- a lane each: the decoder's own
// prediction from an LDS tile of the macroblock under construction with its edge, forward DCT, dead-zone quantisation, the
// decoder's dequantisation and inverse DCT, squared error + lambda * (level bits + the mode's exact price under
// kVp8BModesProba[above][left]); the cheapest candidate of each sub-block goes into the tile.  Candidates and tile stay in
// LDS; the winner of the macroblock is stored once: planes, levels, record.
// No wave waits for another by polling; all control flow around a barrier is uniform in the workgroup (the step count depends
// on the geometry alone).  Integer arithmetic only: the same pixels give the same bytes on every run and in every batch position.
#include <hip/hip_runtime.h>

#include "vp8_encode_args.hpp"

namespace ifhip {

__global__ __launch_bounds__(64 * kVp8eWaves) void vp8e_code4_kernel(const Vp8eArgs a) {
    __shared__ Vp8eMb4Work work[kVp8eWaves];
    const uint32_t img = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    Vp8eFrame F;
    F.src = vp8e_planes(a, img, false); F.rec = vp8e_planes(a, img, true);
    F.mbs = a.mbs + static_cast<size_t>(img) * vp8e_mb_count(a);
    F.levels = a.levels + static_cast<size_t>(img) * vp8e_mb_count(a) * kVp8MbLevels;
    F.p = a.p;
    Vp8eMb4Work& W = work[wave];
    auto sync = [] {                                                      // the wave's own LDS stores, before its other lanes read them
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    const uint32_t steps = a.mbw + 2u * (a.mbh - 1u);
    for (uint32_t s = 0; s < steps; ++s) {
        // the rows with 0 <= s - 2y < mbw
        const uint32_t lo = s >= a.mbw ? (s - a.mbw + 2u) >> 1 : 0u, hi = min(a.mbh - 1u, s >> 1);
        for (uint32_t y = lo + wave; y <= hi; y += kVp8eWaves) vp8e_code_mb4(*a.T, F, W, s - 2u * y, y, lane, 64u, sync);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");            // this step's pixels and records, before another wave's next step reads them
        __syncthreads();
    }
}

void vp8e_launch_code4(const Vp8eArgs& a, hipStream_t stream) { hipLaunchKernelGGL(vp8e_code4_kernel, dim3(a.n_images), dim3(64u * kVp8eWaves), 0, stream, a); }

}  // namespace ifhip
