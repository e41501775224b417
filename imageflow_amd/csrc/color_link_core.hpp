// color_link_core.hpp -- the arithmetic of one pixel through a colour link, shared by the kernel (csrc/color_link.hip), the
// host builder (csrc/color_link.cpp, which walks a profile's own tables with the same interpolation) and the CPU emulation
// (tests/color_link_emulate.cpp), so that the three agree byte for byte.  Integers only; compiles for host and device.
//
// An RGB link is lcms2's device link for 8-bit pixels (cmsopt.c PrelinEval8 over a 33 x 33 x 33 table of 16-bit nodes, the
// R index slowest).  Per channel, byte -> v16 = 257 * byte -> the 16.16 grid position p = v16 * 32 brought to the fixed
// domain (p + (p + 0x7FFF) / 0xFFFF: 0xFFFF lands on node 32 with no remainder).  The cell is cut into six tetrahedra by the
// order of the three remainders: from the cell's low corner the walk takes the axis of the largest remainder first, and each
// step's difference of nodes is weighted by that axis's remainder,
//     rest = d1 * ra + d2 * rb + d3 * rc + 0x8001          (32 bits, wrapping as lcms2's int does)
//     out  = c0 + ((rest + (rest >> 16)) >> 16)             (arithmetic shifts, 16 bits kept)
// Every product is exact, so which way a tie between remainders goes changes nothing.  An axis with no remainder takes no
// step: the walk never reads a node past the table (byte 255 sits on node 32).  16 bits go to 8 as lcms2's FROM_16_TO_8,
// (v * 65281 + 8388608) >> 24.  The pixel's fourth byte is carried over.
//
// A grey link is 256 bytes: the pixel's B byte looked up, the result written to B, G and R.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IFHIP_CL_HD __host__ __device__ inline __attribute__((always_inline))      // (also where hip_runtime.h is not included)
#else
#define IFHIP_CL_HD inline
#endif

namespace ifhip {

constexpr uint32_t kLinkGrid = 33u;
constexpr uint32_t kLinkNodes = kLinkGrid * kLinkGrid * kLinkGrid;

// a 16-bit value times `domain` (grid points - 1) as a 16.16 position: lcms2's _cmsToFixedDomain
IFHIP_CL_HD uint32_t link_fixed_domain(uint32_t v) { return v + (v + 0x7FFFu) / 0xFFFFu; }
IFHIP_CL_HD uint32_t link_position(uint32_t byte) { return link_fixed_domain(byte * 257u * (kLinkGrid - 1u)); }

// c0..c3: one channel of the four nodes along the walk; ra >= rb >= rc: the remainders of the axes in the walk's order
IFHIP_CL_HD uint32_t link_interp(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t ra, uint32_t rb, uint32_t rc) {
    const uint32_t rest = (c1 - c0) * ra + (c2 - c1) * rb + (c3 - c2) * rc + 0x8001u;
    const uint32_t t = rest + static_cast<uint32_t>(static_cast<int32_t>(rest) >> 16);
    return (c0 + static_cast<uint32_t>(static_cast<int32_t>(t) >> 16)) & 0xFFFFu;
}
IFHIP_CL_HD uint32_t link_to_byte(uint32_t v16) { return (v16 * 65281u + 8388608u) >> 24; }

// the walk through one cell: remainders and node strides of the three axes, sorted so that ra >= rb >= rc; an axis without
// a remainder has stride 0
struct LinkWalk { uint32_t ra, rb, rc, da, db, dc; };
IFHIP_CL_HD LinkWalk link_walk(uint32_t rx, uint32_t ry, uint32_t rz, uint32_t sx, uint32_t sy, uint32_t sz) {
    LinkWalk k{rx, ry, rz, rx ? sx : 0u, ry ? sy : 0u, rz ? sz : 0u};
    uint32_t t;
    if (k.ra < k.rb) { t = k.ra; k.ra = k.rb; k.rb = t; t = k.da; k.da = k.db; k.db = t; }
    if (k.rb < k.rc) { t = k.rb; k.rb = k.rc; k.rc = t; t = k.db; k.db = k.dc; k.dc = t; }
    if (k.ra < k.rb) { t = k.ra; k.ra = k.rb; k.rb = t; t = k.da; k.da = k.db; k.db = t; }
    return k;
}

// px: a BGRA dword (B in the low byte).  nodes(i): node i as 64 bits, R in bits 0..15, G in 16..31, B in 32..47.
template <typename Nodes>
IFHIP_CL_HD uint32_t link_pixel(uint32_t px, const Nodes& nodes) {
    const uint32_t pr = link_position((px >> 16) & 255u), pg = link_position((px >> 8) & 255u), pb = link_position(px & 255u);
    const uint32_t base = ((pr >> 16) * kLinkGrid + (pg >> 16)) * kLinkGrid + (pb >> 16);
    const LinkWalk k = link_walk(pr & 0xFFFFu, pg & 0xFFFFu, pb & 0xFFFFu, kLinkGrid * kLinkGrid, kLinkGrid, 1u);
    const uint64_t n0 = nodes(base), n1 = nodes(base + k.da), n2 = nodes(base + k.da + k.db), n3 = nodes(base + k.da + k.db + k.dc);
    uint32_t out = px & 0xFF000000u;
    for (uint32_t c = 0; c < 3u; ++c) {                                          // c = 0: R -> bits 16..23
        const uint32_t s = 16u * c;
        const uint32_t v = link_interp(static_cast<uint32_t>(n0 >> s) & 0xFFFFu, static_cast<uint32_t>(n1 >> s) & 0xFFFFu,
                                       static_cast<uint32_t>(n2 >> s) & 0xFFFFu, static_cast<uint32_t>(n3 >> s) & 0xFFFFu, k.ra, k.rb, k.rc);
        out |= link_to_byte(v) << (16u - 8u * c);
    }
    return out;
}

template <typename Table>
IFHIP_CL_HD uint32_t link_gray_pixel(uint32_t px, const Table& table) {
    const uint32_t g = table[px & 255u];
    return (px & 0xFF000000u) | g * 0x010101u;
}

}  // namespace ifhip
