// color_profile_core.hpp -- the arithmetic of one pixel's conversion to sRGB, shared by the kernel (csrc/color_profile.hip)
// and its CPU emulation (tests/color_profile_emulate.cpp), so that the two agree byte for byte.  Compiles for host and
// device; no libm call is evaluated here (the tables come from the host: csrc/color_profile.cpp, csrc/color.cpp).
//
// The order is fixed and written down: per output channel c (R, G, B), with m = matrix row c and r, g, b the source's
// linear light from the plan's tables,
//     v = fma(m[2], b, fma(m[1], g, m[0] * r))                         three roundings, f32
//     byte = l2s[(uint32) min(max(v * 16383, 0), 16383)]              (lut.rs:4-8: NaN -> index 0; max/min drop a NaN)
// which is how csrc/round_corners.hip indexes the same 16384-entry table.  The pixel's fourth byte is carried over.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IFHIP_CP_HD __host__ __device__ __forceinline__
#else
#define IFHIP_CP_HD inline
#endif

namespace ifhip {

IFHIP_CP_HD float color_mix(const float* m, float r, float g, float b) {
    return __builtin_fmaf(m[2], b, __builtin_fmaf(m[1], g, m[0] * r));
}
IFHIP_CP_HD uint32_t color_l2s_index(float v) {
    const float s = __builtin_fminf(__builtin_fmaxf(v * 16383.0f, 0.0f), 16383.0f);
    return static_cast<uint32_t>(s);
}
// px: a BGRA dword (B in the low byte).  lr / lg / lb: the source's linear light of the pixel's R, G and B bytes.
template <typename L2S>
IFHIP_CP_HD uint32_t color_pixel(uint32_t px, float lr, float lg, float lb, const float* matrix, const L2S& l2s) {
    const uint32_t r = l2s[color_l2s_index(color_mix(matrix, lr, lg, lb))];
    const uint32_t g = l2s[color_l2s_index(color_mix(matrix + 3, lr, lg, lb))];
    const uint32_t b = l2s[color_l2s_index(color_mix(matrix + 6, lr, lg, lb))];
    return (px & 0xFF000000u) | (r << 16) | (g << 8) | b;
}

}  // namespace ifhip
