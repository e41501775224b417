// vp8_decode_core.hpp -- the one statement of the pixel side of a VP8 key frame (RFC 6386, with the bits libwebp 1.6.0 settles:
// WebPDecode into MODE_BGRA with the default options -- fancy upsampling, loop filter honoured, no dithering, alpha not
// premultiplied) for the device lossy WebP decoder.  The kernels of csrc/vp8_decode.hip and the CPU emulation of the tests
// (tests/vp8_decode_emulate.cpp) are built from the same functions: dequantisation with the inverse WHT and the inverse DCT,
// the 4 + 4 + 10 intra predictors with libwebp's border rules, the simple and the normal loop filter, the fancy chroma
// upsampler, YUV -> BGRA and the alpha plane's predictors.  What is serial -- the bool decoder, the header, the modes and
// the coefficient tokens -- is the host's (csrc/vp8_read.cpp) and hands over the records below.
//
// Block numbering inside a macroblock: 0..15 luma in raster order, 16..19 U, 20..23 V, 24 the Y2 block of a 16x16-mode
// macroblock.  A block's sixteen levels lie at their raster positions (the host has undone the zigzag), 400 int16 a macroblock.
#pragma once
#include <cstddef>
#include <cstdint>

#include "prefix_code_core.hpp"      // IFHIP_HD

#if defined(__HIP_DEVICE_COMPILE__)
#define VP8_UNROLL _Pragma("unroll")       // the small arrays below live in registers only where their loops are unrolled
#else
#define VP8_UNROLL
#endif

namespace ifhip {

enum : uint32_t {                    // include/imageflow_hip.h IFHIP_VP8_DEC_*
    kVp8DecOk = 0,
    kVp8DecContainer = 1,
    kVp8DecNotLossy = 2,
    kVp8DecFrameHeader = 3,
    kVp8DecPartitions = 4,
    kVp8DecEndOfModes = 5,
    kVp8DecEndOfTokens = 6,
    kVp8DecAlphaHeader = 7,
    kVp8DecAlphaStream = 8,
};

constexpr uint32_t kVp8MbLevels = 400;   // int16 per macroblock: 25 blocks of 16
constexpr uint32_t kVp8ModeB = 4;        // Vp8Mb::ymode: sixteen 4x4 modes; 0..3 are DC, TM, V, H for the whole macroblock
enum : uint32_t { kVp8FilterNone = 0, kVp8FilterSimple = 1, kVp8FilterNormal = 2 };
enum : uint32_t { kVp8AlphaNone = 0, kVp8AlphaRaw = 1, kVp8AlphaVp8l = 2 };

struct Vp8Mb {                       // 36 bytes a macroblock
    uint8_t ymode, uvmode, segment;
    uint8_t inner;                   // the inner edges are filtered: a 4x4-mode macroblock, or any non-zero coefficient
    uint8_t limit, ilevel, hev;      // libwebp's PrecomputeFilterStrengths: 2 * level + ilevel (0: not filtered), interior limit, hev threshold
    uint8_t pad;
    uint32_t nz;                     // bit b: block b holds a non-zero level
    uint32_t dc_only;                // bit b: the block takes the DC-only transform
    uint32_t ac3;                    // bit b: a luma block whose levels end within the first three of the zigzag (see vp8_residual_block)
    uint8_t imodes[16];              // the 4x4 modes in libwebp's numbering: DC TM VE HE RD VR LD VL HD HU
};
struct Vp8Quant { uint16_t y1[2], y2[2], uv[2]; };   // [0] DC, [1] AC
struct Vp8Planes {
    uint8_t* y; uint8_t* u; uint8_t* v;  // whole macroblocks: 16 * mbw x 16 * mbh, and 8 * mbw x 8 * mbh
    uint32_t ypitch, uvpitch;
    uint32_t mbw, mbh;
};

IFHIP_HD int vp8_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
IFHIP_HD int vp8_abs(int v) { return v < 0 ? -v : v; }
IFHIP_HD int vp8_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// libwebp keeps dequantised coefficients in int16_t: the product wraps there
IFHIP_HD int vp8_dequant(int level, int q) { return static_cast<int16_t>(level * q); }

// ---- the inverse WHT: one output of the sixteen (the DC of luma block b), RFC 6386 14.3 with libwebp's rounding --------------------------
IFHIP_HD int vp8_wht_one(const int16_t* y2, int qdc, int qac, uint32_t b) {
    const uint32_t i = b >> 2, k = b & 3u;
    int t[4];                                                             // tmp[4 * i + j], j = 0..3
    VP8_UNROLL
    for (uint32_t j = 0; j < 4u; ++j) {
        const int c0 = vp8_dequant(y2[j], j ? qac : qdc), c1 = vp8_dequant(y2[4u + j], qac), c2 = vp8_dequant(y2[8u + j], qac), c3 = vp8_dequant(y2[12u + j], qac);
        const int a0 = c0 + c3, a1 = c1 + c2, a2 = c1 - c2, a3 = c0 - c3;
        t[j] = i == 0u ? a0 + a1 : i == 1u ? a3 + a2 : i == 2u ? a0 - a1 : a3 - a2;
    }
    const int dc = t[0] + 3;
    const int a0 = dc + t[3], a1 = t[1] + t[2], a2 = t[1] - t[2], a3 = dc - t[3];
    const int v = k == 0u ? a0 + a1 : k == 1u ? a3 + a2 : k == 2u ? a0 - a1 : a3 - a2;
    return static_cast<int16_t>(v >> 3);
}

// ---- the inverse DCT (libwebp's TransformOne): the block's levels -> what is added to the prediction, in place -----------------------------
// dc: the block's first coefficient already dequantised (the WHT's output for a 16x16-mode luma block).  The result of
// TransformOne is clip(prediction + (v >> 3)); v >> 3 is kept, limited to +-255 (beyond that the clip decides alone).
// Coefficients beyond +-2048 are outside what an encoder may write, and there libwebp's answer depends on the routine a
// block is given: the full transform is its 16-bit SIMD form, whose sums wrap at 16 bits (`wrap`), while a DC-only block
// and a luma block with at most three levels (TransformDC, TransformAC3) are computed in plain ints.  Chroma takes the full
// transform for all four blocks of a plane as soon as one of them has a second level.  Inside the legal range all agree.
IFHIP_HD int vp8_mul1(int a) { return ((a * 20091) >> 16) + a; }
IFHIP_HD int vp8_mul2(int a) { return (a * 35468) >> 16; }
IFHIP_HD int vp8_wrap16(int v, bool wrap) { return wrap ? static_cast<int16_t>(v) : v; }
IFHIP_HD void vp8_residual_block(int16_t* blk, int dc, int qac, bool dc_only, bool wrap) {
    if (dc_only) {
        const int16_t r = static_cast<int16_t>(vp8_clamp((dc + 4) >> 3, -255, 255));
    VP8_UNROLL
        for (uint32_t i = 0; i < 16u; ++i) blk[i] = r;
        return;
    }
    int tmp[16];
    VP8_UNROLL
    for (uint32_t i = 0; i < 4u; ++i) {                                   // the vertical pass
        const int c0 = i ? vp8_dequant(blk[i], qac) : dc, c4 = vp8_dequant(blk[4u + i], qac), c8 = vp8_dequant(blk[8u + i], qac), c12 = vp8_dequant(blk[12u + i], qac);
        const int a = vp8_wrap16(c0 + c8, wrap), b = vp8_wrap16(c0 - c8, wrap);
        const int c = vp8_wrap16(vp8_mul2(c4) - vp8_mul1(c12), wrap), d = vp8_wrap16(vp8_mul1(c4) + vp8_mul2(c12), wrap);
        tmp[4u * i + 0u] = vp8_wrap16(a + d, wrap); tmp[4u * i + 1u] = vp8_wrap16(b + c, wrap); tmp[4u * i + 2u] = vp8_wrap16(b - c, wrap); tmp[4u * i + 3u] = vp8_wrap16(a - d, wrap);
    }
    VP8_UNROLL
    for (uint32_t i = 0; i < 4u; ++i) {                                   // the horizontal pass: row i
        const int dcr = vp8_wrap16(tmp[i] + 4, wrap);
        const int a = vp8_wrap16(dcr + tmp[8u + i], wrap), b = vp8_wrap16(dcr - tmp[8u + i], wrap);
        const int c = vp8_wrap16(vp8_mul2(tmp[4u + i]) - vp8_mul1(tmp[12u + i]), wrap), d = vp8_wrap16(vp8_mul1(tmp[4u + i]) + vp8_mul2(tmp[12u + i]), wrap);
        blk[4u * i + 0u] = static_cast<int16_t>(vp8_clamp(vp8_wrap16(a + d, wrap) >> 3, -255, 255));
        blk[4u * i + 1u] = static_cast<int16_t>(vp8_clamp(vp8_wrap16(b + c, wrap) >> 3, -255, 255));
        blk[4u * i + 2u] = static_cast<int16_t>(vp8_clamp(vp8_wrap16(b - c, wrap) >> 3, -255, 255));
        blk[4u * i + 3u] = static_cast<int16_t>(vp8_clamp(vp8_wrap16(a - d, wrap) >> 3, -255, 255));
    }
}
// Block b (0..23) of a macroblock: levels -> residuals in place.  Block 24 (Y2) is read by the sixteen luma blocks, written by none.
IFHIP_HD void vp8_residual_mb_block(int16_t* levels, const Vp8Mb& mb, const Vp8Quant& q, uint32_t b) {
    int16_t* blk = levels + 16u * b;
    const bool i16 = mb.ymode != kVp8ModeB;
    const bool any = ((mb.nz >> b) & 1u) != 0u;
    const bool dc_only = ((mb.dc_only >> b) & 1u) != 0u, wrap = ((mb.ac3 >> b) & 1u) == 0u;
    if (b < 16u && i16) {
        const bool y2 = ((mb.nz >> 24) & 1u) != 0u;
        if (!any && !y2) return;                                          // (zero levels are zero residuals)
        const int dc = y2 ? vp8_wht_one(levels + 16u * 24u, q.y2[0], q.y2[1], b) : 0;
        vp8_residual_block(blk, dc, q.y1[1], dc_only, wrap);
        return;
    }
    if (!any) return;
    const uint16_t* m = b < 16u ? q.y1 : q.uv;
    vp8_residual_block(blk, vp8_dequant(blk[0], m[0]), m[1], dc_only, wrap);
}

// ---- intra prediction: libwebp's borders -- 127 above the frame, 129 to its left, the corner 127 on the first row and 129 below ------------
IFHIP_HD int vp8_top(const uint8_t* p, uint32_t pitch, uint32_t x, uint32_t y0) { return y0 ? p[static_cast<size_t>(y0 - 1u) * pitch + x] : 127; }
IFHIP_HD int vp8_left(const uint8_t* p, uint32_t pitch, uint32_t x0, uint32_t y) { return x0 ? p[static_cast<size_t>(y) * pitch + x0 - 1u] : 129; }
IFHIP_HD int vp8_corner(const uint8_t* p, uint32_t pitch, uint32_t x0, uint32_t y0) {
    return x0 && y0 ? p[static_cast<size_t>(y0 - 1u) * pitch + x0 - 1u] : y0 ? 129 : 127;
}
// the DC of a whole-macroblock prediction (size 16 luma, 8 chroma) at plane position x0, y0
IFHIP_HD int vp8_dc_large(const uint8_t* p, uint32_t pitch, uint32_t x0, uint32_t y0, uint32_t size) {
    const uint32_t shift = size == 16u ? 4u : 3u;
    if (!x0 && !y0) return 128;
    int top = 0, left = 0;
    if (y0) for (uint32_t i = 0; i < size; ++i) top += p[static_cast<size_t>(y0 - 1u) * pitch + x0 + i];
    if (x0) for (uint32_t i = 0; i < size; ++i) left += p[static_cast<size_t>(y0 + i) * pitch + x0 - 1u];
    if (!y0) top = left;
    if (!x0) left = top;
    return (top + left + static_cast<int>(size)) >> (shift + 1u);
}
// one pixel of a whole-macroblock prediction: mode 0 DC (dc from vp8_dc_large), 1 TM, 2 V, 3 H
IFHIP_HD int vp8_pred_large(const uint8_t* p, uint32_t pitch, uint32_t x0, uint32_t y0, uint32_t mode, uint32_t px, uint32_t py, int dc) {
    if (mode == 0u) return dc;
    if (mode == 2u) return vp8_top(p, pitch, x0 + px, y0);
    if (mode == 3u) return vp8_left(p, pitch, x0, y0 + py);
    return vp8_clip8(vp8_top(p, pitch, x0 + px, y0) + vp8_left(p, pitch, x0, y0 + py) - vp8_corner(p, pitch, x0, y0));
}

IFHIP_HD int vp8_avg2(int a, int b) { return (a + b + 1) >> 1; }
IFHIP_HD int vp8_avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
// The sixteen predicted values of a 4x4 sub-block in raster order from its edge: T the four pixels above and the four above-right,
// L the four to the left, X the corner.  Modes in libwebp's numbering: DC TM VE HE RD VR LD VL HD HU.  The decoder
// (vp8_predict_sub) and the coder's 4x4 search (vp8_encode_core.hpp) both predict with this function.
// (the edge and the result are copied through locals: arrays reached through the pointers of an inlined call are not promoted to
// registers by the gfx950 build, locals are)
IFHIP_HD void vp8_pred_sub16(uint32_t mode, const int* edge_above, const int* edge_left, int X, int* out) {
    const int A = edge_above[0], B = edge_above[1], C = edge_above[2], D = edge_above[3], E = edge_above[4], F = edge_above[5], G = edge_above[6], H = edge_above[7];
    const int I = edge_left[0], J = edge_left[1], K = edge_left[2], M = edge_left[3];
    const int T[4] = {A, B, C, D}, L[4] = {I, J, K, M};
    int o[16];
#define VP8_DST(x, y) o[(x) + 4 * (y)]
    switch (mode) {
    case 0: {                                                             // DC
        const int dc = (A + B + C + D + I + J + K + M + 4) >> 3;
        VP8_UNROLL
        for (int i = 0; i < 16; ++i) o[i] = dc;
        break; }
    case 1:                                                               // TM
        VP8_UNROLL
        for (int i = 0; i < 16; ++i) o[i] = vp8_clip8(T[i & 3] + L[i >> 2] - X);
        break;
    case 2: {                                                             // VE
        const int v0 = vp8_avg3(X, A, B), v1 = vp8_avg3(A, B, C), v2 = vp8_avg3(B, C, D), v3 = vp8_avg3(C, D, E);
        VP8_UNROLL
        for (int y = 0; y < 4; ++y) { VP8_DST(0, y) = v0; VP8_DST(1, y) = v1; VP8_DST(2, y) = v2; VP8_DST(3, y) = v3; }
        break; }
    case 3: {                                                             // HE
        const int h0 = vp8_avg3(X, I, J), h1 = vp8_avg3(I, J, K), h2 = vp8_avg3(J, K, M), h3 = vp8_avg3(K, M, M);
        VP8_UNROLL
        for (int x = 0; x < 4; ++x) { VP8_DST(x, 0) = h0; VP8_DST(x, 1) = h1; VP8_DST(x, 2) = h2; VP8_DST(x, 3) = h3; }
        break; }
    case 4:                                                               // RD
        VP8_DST(0, 3) = vp8_avg3(J, K, M);
        VP8_DST(1, 3) = VP8_DST(0, 2) = vp8_avg3(I, J, K);
        VP8_DST(2, 3) = VP8_DST(1, 2) = VP8_DST(0, 1) = vp8_avg3(X, I, J);
        VP8_DST(3, 3) = VP8_DST(2, 2) = VP8_DST(1, 1) = VP8_DST(0, 0) = vp8_avg3(A, X, I);
        VP8_DST(3, 2) = VP8_DST(2, 1) = VP8_DST(1, 0) = vp8_avg3(B, A, X);
        VP8_DST(3, 1) = VP8_DST(2, 0) = vp8_avg3(C, B, A);
        VP8_DST(3, 0) = vp8_avg3(D, C, B);
        break;
    case 5:                                                               // VR
        VP8_DST(0, 0) = VP8_DST(1, 2) = vp8_avg2(X, A);
        VP8_DST(1, 0) = VP8_DST(2, 2) = vp8_avg2(A, B);
        VP8_DST(2, 0) = VP8_DST(3, 2) = vp8_avg2(B, C);
        VP8_DST(3, 0) = vp8_avg2(C, D);
        VP8_DST(0, 3) = vp8_avg3(K, J, I);
        VP8_DST(0, 2) = vp8_avg3(J, I, X);
        VP8_DST(0, 1) = VP8_DST(1, 3) = vp8_avg3(I, X, A);
        VP8_DST(1, 1) = VP8_DST(2, 3) = vp8_avg3(X, A, B);
        VP8_DST(2, 1) = VP8_DST(3, 3) = vp8_avg3(A, B, C);
        VP8_DST(3, 1) = vp8_avg3(B, C, D);
        break;
    case 6:                                                               // LD
        VP8_DST(0, 0) = vp8_avg3(A, B, C);
        VP8_DST(1, 0) = VP8_DST(0, 1) = vp8_avg3(B, C, D);
        VP8_DST(2, 0) = VP8_DST(1, 1) = VP8_DST(0, 2) = vp8_avg3(C, D, E);
        VP8_DST(3, 0) = VP8_DST(2, 1) = VP8_DST(1, 2) = VP8_DST(0, 3) = vp8_avg3(D, E, F);
        VP8_DST(3, 1) = VP8_DST(2, 2) = VP8_DST(1, 3) = vp8_avg3(E, F, G);
        VP8_DST(3, 2) = VP8_DST(2, 3) = vp8_avg3(F, G, H);
        VP8_DST(3, 3) = vp8_avg3(G, H, H);
        break;
    case 7:                                                               // VL
        VP8_DST(0, 0) = vp8_avg2(A, B);
        VP8_DST(1, 0) = VP8_DST(0, 2) = vp8_avg2(B, C);
        VP8_DST(2, 0) = VP8_DST(1, 2) = vp8_avg2(C, D);
        VP8_DST(3, 0) = VP8_DST(2, 2) = vp8_avg2(D, E);
        VP8_DST(0, 1) = vp8_avg3(A, B, C);
        VP8_DST(1, 1) = VP8_DST(0, 3) = vp8_avg3(B, C, D);
        VP8_DST(2, 1) = VP8_DST(1, 3) = vp8_avg3(C, D, E);
        VP8_DST(3, 1) = VP8_DST(2, 3) = vp8_avg3(D, E, F);
        VP8_DST(3, 2) = vp8_avg3(E, F, G);
        VP8_DST(3, 3) = vp8_avg3(F, G, H);
        break;
    case 8:                                                               // HD
        VP8_DST(0, 0) = VP8_DST(2, 1) = vp8_avg2(I, X);
        VP8_DST(0, 1) = VP8_DST(2, 2) = vp8_avg2(J, I);
        VP8_DST(0, 2) = VP8_DST(2, 3) = vp8_avg2(K, J);
        VP8_DST(0, 3) = vp8_avg2(M, K);
        VP8_DST(3, 0) = vp8_avg3(A, B, C);
        VP8_DST(2, 0) = vp8_avg3(X, A, B);
        VP8_DST(1, 0) = VP8_DST(3, 1) = vp8_avg3(I, X, A);
        VP8_DST(1, 1) = VP8_DST(3, 2) = vp8_avg3(J, I, X);
        VP8_DST(1, 2) = VP8_DST(3, 3) = vp8_avg3(K, J, I);
        VP8_DST(1, 3) = vp8_avg3(M, K, J);
        break;
    default:                                                              // HU
        VP8_DST(0, 0) = vp8_avg2(I, J);
        VP8_DST(2, 0) = VP8_DST(0, 1) = vp8_avg2(J, K);
        VP8_DST(2, 1) = VP8_DST(0, 2) = vp8_avg2(K, M);
        VP8_DST(1, 0) = vp8_avg3(I, J, K);
        VP8_DST(3, 0) = VP8_DST(1, 1) = vp8_avg3(J, K, M);
        VP8_DST(3, 1) = VP8_DST(1, 2) = vp8_avg3(K, M, M);
        VP8_DST(3, 2) = VP8_DST(2, 2) = VP8_DST(0, 3) = VP8_DST(1, 3) = VP8_DST(2, 3) = VP8_DST(3, 3) = M;
        break;
    }
#undef VP8_DST
    VP8_UNROLL
    for (int i = 0; i < 16; ++i) out[i] = o[i];
}
// A luma macroblock under construction with its edge, as the 4x4 search of the coder keeps it (in LDS on the device): row 0 is
// the corner, the sixteen pixels above and the four above-right; rows 1..16 are the pixel to the left and the macroblock's own
// sixteen.  The borders of the frame are filled in by vp8_tile_load_edge with the values vp8_predict_sub reads there.
constexpr uint32_t kVp8TilePitch = 24;
constexpr uint32_t kVp8TileBytes = 17u * kVp8TilePitch;
// edge byte i of 37: 0 the corner, 1..16 above, 17..20 above-right, 21..36 the left column
IFHIP_HD void vp8_tile_load_edge(uint8_t* tile, const uint8_t* p, uint32_t pitch, uint32_t mbw, uint32_t mbx, uint32_t mby, uint32_t i) {
    const uint32_t x0 = mbx * 16u, y0 = mby * 16u;
    if (i == 0u) tile[0] = static_cast<uint8_t>(vp8_corner(p, pitch, x0, y0));
    else if (i <= 16u) tile[i] = static_cast<uint8_t>(vp8_top(p, pitch, x0 + i - 1u, y0));
    else if (i <= 20u) {
        int v = 127;
        if (mby) { const size_t row = static_cast<size_t>(y0 - 1u) * pitch; v = mbx + 1u < mbw ? p[row + x0 + i - 1u] : p[row + x0 + 15u]; }
        tile[i] = static_cast<uint8_t>(v);
    } else tile[(i - 20u) * kVp8TilePitch] = static_cast<uint8_t>(vp8_left(p, pitch, x0, y0 + i - 21u));
}
// the edge of sub-block (bx, by) from such a tile: what vp8_predict_sub gathers from the plane (the above-right of the last
// sub-block column comes from row 0 for all four rows)
IFHIP_HD void vp8_tile_sub_edge(const uint8_t* tile, uint32_t bx, uint32_t by, int* T, int* L, int* X) {
    const uint8_t* above = tile + 4u * by * kVp8TilePitch + 4u * bx;      // the corner of the sub-block
    *X = above[0];
    VP8_UNROLL
    for (uint32_t i = 0; i < 4u; ++i) { T[i] = above[1u + i]; L[i] = above[(1u + i) * kVp8TilePitch]; }
    VP8_UNROLL
    for (uint32_t i = 0; i < 4u; ++i) T[4u + i] = bx < 3u ? above[5u + i] : tile[17u + i];
}
// One 4x4 sub-block (bx, by) of macroblock (mbx, mby): prediction from the plane plus the block's residuals, stored to the plane.
// The above-right of the sub-blocks in the macroblock's last column is, for all four rows, the bottom row of the macroblock
// above and to the right (the above macroblock's last pixel four times at the frame's right edge).
IFHIP_HD void vp8_predict_sub(uint8_t* p, uint32_t pitch, uint32_t mbw, uint32_t mbx, uint32_t mby, uint32_t bx, uint32_t by, uint32_t mode, const int16_t* res) {
    const uint32_t x0 = mbx * 16u + bx * 4u, y0 = mby * 16u + by * 4u;
    int T[8], L[4], o[16];
    const int X = vp8_corner(p, pitch, x0, y0);
    VP8_UNROLL
    for (uint32_t i = 0; i < 4u; ++i) { T[i] = vp8_top(p, pitch, x0 + i, y0); L[i] = vp8_left(p, pitch, x0, y0 + i); }
    VP8_UNROLL
    for (uint32_t i = 0; i < 4u; ++i) {
        int v = 127;
        if (mby) {
            if (bx < 3u) v = p[static_cast<size_t>(y0 - 1u) * pitch + x0 + 4u + i];
            else {
                const size_t row = static_cast<size_t>(mby * 16u - 1u) * pitch;
                v = mbx + 1u < mbw ? p[row + x0 + 4u + i] : p[row + mbx * 16u + 15u];
            }
        } else if (by && bx < 3u) {
            v = p[static_cast<size_t>(y0 - 1u) * pitch + x0 + 4u + i];
        }
        T[4u + i] = v;
    }
    vp8_pred_sub16(mode, T, L, X, o);
    VP8_UNROLL
    for (uint32_t i = 0; i < 16u; ++i)
        p[static_cast<size_t>(y0 + (i >> 2)) * pitch + x0 + (i & 3u)] = static_cast<uint8_t>(vp8_clip8(o[i] + res[i]));
}

// the two chroma planes of macroblock (mbx, mby): its second half, which the coder also runs alone behind its 4x4 search
IFHIP_HD void vp8_predict_mb_chroma(const Vp8Planes& P, const Vp8Mb& mb, const int16_t* res, uint32_t mbx, uint32_t mby, uint32_t lane, uint32_t nlanes) {
    const uint32_t x0 = mbx * 8u, y0 = mby * 8u;
    const int dcu = mb.uvmode == 0u ? vp8_dc_large(P.u, P.uvpitch, x0, y0, 8u) : 0;
    const int dcv = mb.uvmode == 0u ? vp8_dc_large(P.v, P.uvpitch, x0, y0, 8u) : 0;
    for (uint32_t i = lane; i < 128u; i += nlanes) {
        const uint32_t c = i >> 6, px = i & 7u, py = (i >> 3) & 7u;
        uint8_t* plane = c ? P.v : P.u;
        const int r = res[16u * (16u + 4u * c + (py >> 2) * 2u + (px >> 2)) + (py & 3u) * 4u + (px & 3u)];
        plane[static_cast<size_t>(y0 + py) * P.uvpitch + x0 + px] = static_cast<uint8_t>(vp8_clip8(vp8_pred_large(plane, P.uvpitch, x0, y0, mb.uvmode, px, py, c ? dcv : dcu) + r));
    }
}
// Macroblock (mbx, mby) by `nlanes` lanes: prediction plus residual into the three planes.  The pixels of a whole-macroblock
// mode and of the chroma blocks are independent and spread over the lanes; the sixteen 4x4 sub-blocks of a 4x4-mode
// macroblock depend on each other and are lane 0's, in raster order.  Reads the finished macroblocks to the left, above,
// above-left and above-right.
IFHIP_HD void vp8_predict_mb(const Vp8Planes& P, const Vp8Mb& mb, const int16_t* res, uint32_t mbx, uint32_t mby, uint32_t lane, uint32_t nlanes) {
    if (mb.ymode == kVp8ModeB) {
        if (lane == 0u)
            for (uint32_t b = 0; b < 16u; ++b) vp8_predict_sub(P.y, P.ypitch, P.mbw, mbx, mby, b & 3u, b >> 2, mb.imodes[b], res + 16u * b);
    } else {
        const uint32_t x0 = mbx * 16u, y0 = mby * 16u;
        const int dc = mb.ymode == 0u ? vp8_dc_large(P.y, P.ypitch, x0, y0, 16u) : 0;
        for (uint32_t i = lane; i < 256u; i += nlanes) {
            const uint32_t px = i & 15u, py = i >> 4;
            const int r = res[16u * ((py >> 2) * 4u + (px >> 2)) + (py & 3u) * 4u + (px & 3u)];
            P.y[static_cast<size_t>(y0 + py) * P.ypitch + x0 + px] = static_cast<uint8_t>(vp8_clip8(vp8_pred_large(P.y, P.ypitch, x0, y0, mb.ymode, px, py, dc) + r));
        }
    }
    vp8_predict_mb_chroma(P, mb, res, mbx, mby, lane, nlanes);
}

// ---- the loop filter (libwebp's dsp: DoFilter2 / 4 / 6 behind NeedsFilter and Hev) ------------------------------------------------------------
IFHIP_HD int vp8_sclip1(int v) { return vp8_clamp(v, -128, 127); }
IFHIP_HD int vp8_sclip2(int v) { return vp8_clamp(v, -16, 15); }
IFHIP_HD void vp8_filter2(uint8_t* p, ptrdiff_t step) {
    const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
    const int a = 3 * (q0 - p0) + vp8_sclip1(p1 - q1);
    const int a1 = vp8_sclip2((a + 4) >> 3), a2 = vp8_sclip2((a + 3) >> 3);
    p[-step] = static_cast<uint8_t>(vp8_clip8(p0 + a2));
    p[0] = static_cast<uint8_t>(vp8_clip8(q0 - a1));
}
// kind 0: the simple filter; 1: a macroblock edge of the normal filter; 2: an inner edge of the normal filter.
// p: the first pixel behind the edge, step: the distance across it.  thresh is libwebp's `thresh` (2 * thresh + 1 is applied here).
IFHIP_HD void vp8_filter_edge(uint8_t* p, ptrdiff_t step, uint32_t kind, int thresh, int ithresh, int hev_thresh) {
    const int t2 = 2 * thresh + 1;
    const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
    if (4 * vp8_abs(p0 - q0) + vp8_abs(p1 - q1) > t2) return;
    if (kind == 0u) { vp8_filter2(p, step); return; }
    const int p3 = p[-4 * step], p2 = p[-3 * step], q2 = p[2 * step], q3 = p[3 * step];
    if (vp8_abs(p3 - p2) > ithresh || vp8_abs(p2 - p1) > ithresh || vp8_abs(p1 - p0) > ithresh || vp8_abs(q3 - q2) > ithresh || vp8_abs(q2 - q1) > ithresh ||
        vp8_abs(q1 - q0) > ithresh) return;
    if (vp8_abs(p1 - p0) > hev_thresh || vp8_abs(q1 - q0) > hev_thresh) { vp8_filter2(p, step); return; }
    if (kind == 1u) {
        const int a = vp8_sclip1(3 * (q0 - p0) + vp8_sclip1(p1 - q1));
        const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
        p[-3 * step] = static_cast<uint8_t>(vp8_clip8(p2 + a3));
        p[-2 * step] = static_cast<uint8_t>(vp8_clip8(p1 + a2));
        p[-step] = static_cast<uint8_t>(vp8_clip8(p0 + a1));
        p[0] = static_cast<uint8_t>(vp8_clip8(q0 - a1));
        p[step] = static_cast<uint8_t>(vp8_clip8(q1 - a2));
        p[2 * step] = static_cast<uint8_t>(vp8_clip8(q2 - a3));
    } else {
        const int a = 3 * (q0 - p0);
        const int a1 = vp8_sclip2((a + 4) >> 3), a2 = vp8_sclip2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
        p[-2 * step] = static_cast<uint8_t>(vp8_clip8(p1 + a3));
        p[-step] = static_cast<uint8_t>(vp8_clip8(p0 + a2));
        p[0] = static_cast<uint8_t>(vp8_clip8(q0 - a1));
        p[step] = static_cast<uint8_t>(vp8_clip8(q1 - a3));
    }
}
// One line across macroblock (mbx, mby): `vertical` false -- lane's row, the left macroblock edge and then the inner vertical
// edges; true -- lane's column, the top macroblock edge and then the inner horizontal edges.  Lanes 0..15 luma, 16..23 U,
// 24..31 V.  Raster macroblock order is: every lane's rows, then every lane's columns.
IFHIP_HD void vp8_filter_mb_line(const Vp8Planes& P, const Vp8Mb& mb, uint32_t filter, uint32_t mbx, uint32_t mby, uint32_t lane, bool vertical) {
    if (!mb.limit || lane >= 32u) return;
    const bool luma = lane < 16u;
    if (!luma && filter == kVp8FilterSimple) return;
    const uint32_t size = luma ? 16u : 8u, i = luma ? lane : (lane - 16u) & 7u;
    uint8_t* plane = luma ? P.y : lane < 24u ? P.u : P.v;
    const ptrdiff_t pitch = luma ? P.ypitch : P.uvpitch;
    uint8_t* p = plane + static_cast<size_t>(mby * size + (vertical ? 0u : i)) * pitch + mbx * size + (vertical ? i : 0u);
    const ptrdiff_t step = vertical ? pitch : 1;
    const bool simple = filter == kVp8FilterSimple;
    if (vertical ? mby != 0u : mbx != 0u) vp8_filter_edge(p, step, simple ? 0u : 1u, mb.limit + 4, mb.ilevel, mb.hev);
    if (mb.inner)
        for (uint32_t k = 4u; k < size; k += 4u) vp8_filter_edge(p + static_cast<ptrdiff_t>(k) * step, step, simple ? 0u : 2u, mb.limit, mb.ilevel, mb.hev);
}

// ---- the fancy upsampler and YUV -> BGR (libwebp's UpsampleBgraLinePair and VP8YuvToBgra) ----------------------------------------------------------
IFHIP_HD int vp8_mult_hi(int v, int c) { return (v * c) >> 8; }
IFHIP_HD int vp8_clip6(int v) { return (v & ~16383) == 0 ? v >> 6 : v < 0 ? 0 : 255; }
// chroma at output pixel (x, y) of a w x h image from a plane of (w + 1) / 2 x (h + 1) / 2 samples at `pitch`
IFHIP_HD int vp8_fancy_chroma(const uint8_t* c, uint32_t pitch, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
    const uint32_t last_row = (h + 1u) / 2u - 1u, last_pair = (w - 1u) >> 1;
    uint32_t near_row = 0, far_row = 0;
    if (y) {
        const uint32_t k = (y + 1u) >> 1;                                   // rows 2k - 1 and 2k lie between chroma rows k - 1 and k
        near_row = (y & 1u) ? k - 1u : k;
        far_row = (y & 1u) ? k : k - 1u;
        if (k > last_row) near_row = far_row = last_row;
    }
    const uint8_t* N = c + static_cast<size_t>(near_row) * pitch;
    const uint8_t* F = c + static_cast<size_t>(far_row) * pitch;
    if (x == 0u) return (3 * N[0] + F[0] + 2) >> 2;
    const uint32_t j = (x + 1u) >> 1;
    if (j > last_pair) return (3 * N[last_pair] + F[last_pair] + 2) >> 2;
    const int a = N[j - 1u], b = N[j], cc = F[j - 1u], d = F[j];
    const int sum = a + b + cc + d + 8;
    return (x & 1u) ? (((sum + 2 * (b + cc)) >> 3) + a) >> 1 : (((sum + 2 * (a + d)) >> 3) + b) >> 1;
}
IFHIP_HD uint32_t vp8_yuv_to_bgra(int y, int u, int v, uint32_t alpha) {
    const int yy = vp8_mult_hi(y, 19077);
    const uint32_t r = static_cast<uint32_t>(vp8_clip6(yy + vp8_mult_hi(v, 26149) - 14234));
    const uint32_t g = static_cast<uint32_t>(vp8_clip6(yy - vp8_mult_hi(u, 6419) - vp8_mult_hi(v, 13320) + 8708));
    const uint32_t b = static_cast<uint32_t>(vp8_clip6(yy + vp8_mult_hi(u, 33050) - 17685));
    return b | g << 8 | r << 16 | alpha << 24;
}
// the BGRA dword of pixel (x, y); alpha: the alpha plane (w bytes a row) or null for 255
IFHIP_HD uint32_t vp8_bgra_pixel(const Vp8Planes& P, const uint8_t* alpha, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
    const int u = vp8_fancy_chroma(P.u, P.uvpitch, w, h, x, y), v = vp8_fancy_chroma(P.v, P.uvpitch, w, h, x, y);
    return vp8_yuv_to_bgra(P.y[static_cast<size_t>(y) * P.ypitch + x], u, v, alpha ? alpha[static_cast<size_t>(y) * w + x] : 255u);
}

// ---- the alpha plane's predictors (libwebp's unfilters): what is added to the coded byte, mod 256 ---------------------------------------------
// filter 0 none, 1 horizontal, 2 vertical, 3 gradient.  Row 0 predicts from the left (its first pixel from 0), column 0 from above.
IFHIP_HD uint32_t vp8_alpha_predict(uint32_t filter, uint32_t x, uint32_t y, uint32_t left, uint32_t top, uint32_t topleft) {
    if (filter == 0u) return 0u;
    if (y == 0u) return x ? left : 0u;
    if (x == 0u) return top;
    if (filter == 1u) return left;
    if (filter == 2u) return top;
    return static_cast<uint32_t>(vp8_clip8(static_cast<int>(left) + static_cast<int>(top) - static_cast<int>(topleft)));
}

}  // namespace ifhip
