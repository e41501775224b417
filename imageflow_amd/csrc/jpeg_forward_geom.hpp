// jpeg_forward_geom.hpp -- the block geometry of the encode-side JPEG pixel stage, shared by the forward stage
// (csrc/jpeg_forward.hip) and the trellis stage behind it (csrc/jpeg_trellis.hip): host code.
#pragma once
#include <cstdint>
#include <cstring>

#include "common.hpp"

namespace ifhip {

struct FwdGeom {
    uint32_t width, height;
    uint32_t hs[3], vs[3], hmax, vmax;
    uint32_t bw[3], bh[3];          // coefficient blocks per row / column, MCU padded
    uint32_t rbw[3], rbh[3];        // real blocks (ceil(downsampled size / 8)); the rest are dummy blocks
    uint32_t dw[3], dh[3];          // downsampled component size
};

inline int make_fwd_geom(uint32_t width, uint32_t height, const uint8_t* hs, const uint8_t* vs, FwdGeom* g) {
    if (width == 0 || height == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (!hs || !vs) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null sampling factors");
    std::memset(g, 0, sizeof *g);
    g->width = width; g->height = height;
    for (int c = 0; c < 3; ++c) { g->hs[c] = hs[c]; g->vs[c] = vs[c]; }
    g->hmax = hs[0]; g->vmax = vs[0];
    const bool ok = hs[1] == 1 && vs[1] == 1 && hs[2] == 1 && vs[2] == 1 && (g->hmax == 1 || g->hmax == 2) &&
                    (g->vmax == 1 || g->vmax == 2) && !(g->hmax == 1 && g->vmax == 2);
    if (!ok) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: only 4:4:4, 4:2:2 (h2v1) and 4:2:0 sampling");
    const uint32_t mw = (width + 8u * g->hmax - 1u) / (8u * g->hmax), mh = (height + 8u * g->vmax - 1u) / (8u * g->vmax);
    for (int c = 0; c < 3; ++c) {
        g->bw[c] = mw * g->hs[c]; g->bh[c] = mh * g->vs[c];
        g->dw[c] = (width * g->hs[c] + g->hmax - 1u) / g->hmax;
        g->dh[c] = (height * g->vs[c] + g->vmax - 1u) / g->vmax;
        g->rbw[c] = (g->dw[c] + 7u) / 8u; g->rbh[c] = (g->dh[c] + 7u) / 8u;
    }
    return IFHIP_OK;
}

// jpeg_dummy_dc_kernel (csrc/jpeg_forward.hip) on luma planes whose real blocks are written: jccoefct.c's dummy DC values
int launch_dummy_dc(const FwdGeom& g, int16_t* d_coef0, uint32_t n_images, void* hip_stream);

}  // namespace ifhip
