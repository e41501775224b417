// vp8_encode_core.hpp -- the one statement of the device lossy WebP coder: one VP8 key frame (RFC 6386, profile 0, no
// segments; whole-macroblock modes, and the sixteen 4x4 luma modes of a macroblock where kVp8eIntra4 asks for them) and its RIFF
// framing with an optional VP8L-coded ALPH plane.  The kernels of csrc/vp8_encode.hip and csrc/vp8_encode_intra4.hip and the CPU
// emulations of the tests (tests/vp8_encode_emulate.cpp, tests/vp8_encode_intra4_emulate.cpp) are built from the same functions.
// It stands on vp8_decode_core.hpp: prediction, dequantisation, the inverse WHT and DCT and the store into the planes are the
// decoder's own functions, fed with the decoder's own macroblock record, so that what the coder reconstructs is what a
// decoder will see.  The contract is not libwebp's bytes: device file == emulation file, and libwebp decodes that file to
// the pixels the emulation expects.
//
// Known differences from libwebp's encoder, by choice: chroma is a plain box average of the 2x2 RGB sums (no gamma-aware
// averaging, no sharp YUV); 16x16 luma modes only unless kVp8eIntra4 is set; one segment; one pass; the RGB under transparent
// pixels is coded as it is.
//
// Every function with lanes in its signature is written for `nlanes` cooperating lanes (a wave on the device, one on the CPU)
// with sync() between the phases that hand values from lane to lane.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "vp8_decode_core.hpp"

namespace ifhip {

constexpr uint32_t kVp8eMaxDim = 16383;          // 14 bits of width and height in the frame header
constexpr uint32_t kVp8eFileOverflow = 1;        // include/imageflow_hip_webp_lossy_enc.h IFHIP_VP8_ENC_FILE_OVERFLOW
constexpr uint32_t kVp8eMaxLevel = 2047;
constexpr uint32_t kVp8eProbs = 4u * 8u * 3u * 11u;
constexpr uint32_t kVp8eFirstPartMax = (1u << 19) - 1u;      // the frame tag holds the first partition's size in 19 bits
constexpr uint32_t kVp8eIntra4 = 1;              // include/imageflow_hip_webp_lossy_enc.h IFHIP_VP8_ENC_INTRA4: a macroblock may take sixteen 4x4 luma modes
constexpr uint32_t kVp8eIntra4Penalty = 8;       // bits a B_PRED macroblock is charged: the best mean gain of the family {0, 2, 4, 8, 16}
constexpr uint32_t kVp8eFilterNum = 8;           // vp8e_filter_level = index / 2: the best mean PSNR of the family {0, 2, 4, 6, 8} / 16

// the format's constants where device code can reach them (csrc/vp8_tables.inc on the host, a device copy at the stage)
struct Vp8eTables {
    uint8_t dc[128];
    uint16_t ac[128];
    uint8_t proba0[kVp8eProbs], update[kVp8eProbs];
    uint8_t zigzag[16], bands[17];
    uint8_t cat[4][12];
    // the sixteen 4x4 modes of a B_PRED macroblock: the contextual probabilities [above][left][tree node], each mode's way down
    // kVp8BModeTree as (node << 1 | bit) entries behind their count, and what the way costs under every context (vp8e_cost units)
    uint8_t bmode_proba[10][10][9];
    uint8_t bmode_path[10][10];
    uint16_t bmode_cost[10][10][10];
    uint32_t bmode_dearest;             // the largest entry of bmode_cost
};
IFHIP_HD uint32_t vp8e_cost(uint32_t p);
// (host only)
inline const Vp8eTables& vp8e_host_tables() {
    static const Vp8eTables T = [] {
#include "vp8_tables.inc"
        Vp8eTables t{};
        for (int i = 0; i < 128; ++i) { t.dc[i] = kVp8DcTable[i]; t.ac[i] = kVp8AcTable[i]; }
        for (uint32_t i = 0; i < kVp8eProbs; ++i) { t.proba0[i] = (&kVp8CoeffProba0[0][0][0][0])[i]; t.update[i] = (&kVp8CoeffUpdateProba[0][0][0][0])[i]; }
        for (int i = 0; i < 16; ++i) t.zigzag[i] = kVp8Zigzag[i];
        for (int i = 0; i < 17; ++i) t.bands[i] = kVp8Bands[i];
        for (int i = 0; i < 4; ++i) t.cat[0][i] = kVp8Cat3[i];
        for (int i = 0; i < 5; ++i) t.cat[1][i] = kVp8Cat4[i];
        for (int i = 0; i < 6; ++i) t.cat[2][i] = kVp8Cat5[i];
        for (int i = 0; i < 12; ++i) t.cat[3][i] = kVp8Cat6[i];
        for (int a = 0; a < 10; ++a) for (int l = 0; l < 10; ++l) for (int n = 0; n < 9; ++n) t.bmode_proba[a][l][n] = kVp8BModesProba[a][l][n];
        // the tree as the decoder walks it (csrc/vp8_read.cpp): node n has the children tree[2n] and tree[2n + 1]; above 0 a node, else leaf -child
        struct Walk { static void go(Vp8eTables& tt, const int8_t* tree, int node, uint8_t* path, int depth) {
            for (int bit = 0; bit < 2; ++bit) {
                const int child = tree[2 * node + bit];
                path[depth] = static_cast<uint8_t>(node << 1 | bit);
                if (child > 0) go(tt, tree, child, path, depth + 1);
                else { tt.bmode_path[-child][0] = static_cast<uint8_t>(depth + 1); for (int i = 0; i <= depth; ++i) tt.bmode_path[-child][1 + i] = path[i]; }
            }
        } };
        uint8_t path[9];
        Walk::go(t, kVp8BModeTree, 0, path, 0);
        for (int a = 0; a < 10; ++a) for (int l = 0; l < 10; ++l) for (int m = 0; m < 10; ++m) {
            uint32_t c = 0;
            for (uint32_t i = 0; i < t.bmode_path[m][0]; ++i) { const uint32_t e = t.bmode_path[m][1u + i], pr = t.bmode_proba[a][l][e >> 1]; c += vp8e_cost((e & 1u) ? 256u - pr : pr); }
            t.bmode_cost[a][l][m] = static_cast<uint16_t>(c);
            if (c > t.bmode_dearest) t.bmode_dearest = c;
        }
        return t;
    }();
    return T;
}
// libwebp's published QualityToCompression curve, then the quantiser index 0..127 (host: the kernels take the index)
inline uint32_t vp8e_quality_to_index(float quality) {
    const double q = quality < 0.f ? 0.0 : quality > 100.f ? 100.0 : static_cast<double>(quality);
    const double c = q / 100.0, lin = c < 0.75 ? c * (2.0 / 3.0) : 2.0 * c - 1.0;
    const double v = std::cbrt(lin);
    const long idx = std::lround(127.0 * (1.0 - v));
    return static_cast<uint32_t>(idx < 0 ? 0 : idx > 127 ? 127 : idx);
}

// ---- the frame's parameters: all pure integer functions of the quantiser index ------------------------------------------------
struct Vp8eParams {
    Vp8Quant q;
    uint32_t index, filter_level, lambda, n_parts, log2_parts;
    uint8_t limit, ilevel, hev;
    uint8_t i4_penalty;                 // whole bits a B_PRED macroblock is charged beyond its exact price (kVp8eIntra4Penalty)
};
IFHIP_HD uint32_t vp8e_filter_level(uint32_t index, uint32_t num) { const uint32_t l = (index * num) >> 4; return l > 63u ? 63u : l; }
IFHIP_HD uint32_t vp8e_partitions_log2(uint32_t mbh) { return mbh >= 8u ? 3u : mbh >= 4u ? 2u : mbh >= 2u ? 1u : 0u; }
IFHIP_HD Vp8eParams vp8e_params(const Vp8eTables& T, uint32_t index, uint32_t mbh, uint32_t filter_num) {
    Vp8eParams p{};
    p.index = index;
    p.q.y1[0] = T.dc[index]; p.q.y1[1] = T.ac[index];
    p.q.y2[0] = static_cast<uint16_t>(T.dc[index] * 2u);
    p.q.y2[1] = static_cast<uint16_t>((T.ac[index] * 101581u) >> 16);
    if (p.q.y2[1] < 8u) p.q.y2[1] = 8u;
    p.q.uv[0] = T.dc[index > 117u ? 117u : index]; p.q.uv[1] = T.ac[index];
    p.filter_level = vp8e_filter_level(index, filter_num);
    const uint32_t l = p.filter_level;                       // sharpness 0: libwebp's PrecomputeFilterStrengths
    if (l) { p.limit = static_cast<uint8_t>(2u * l + l); p.ilevel = static_cast<uint8_t>(l); p.hev = static_cast<uint8_t>(l >= 40u ? 2u : l >= 15u ? 1u : 0u); }
    const uint32_t ac = p.q.y1[1];
    p.lambda = (ac * ac * 3u) >> 5;                          // what a bit is worth in squared error
    if (p.lambda < 1u) p.lambda = 1u;
    p.i4_penalty = static_cast<uint8_t>(kVp8eIntra4Penalty);
    p.log2_parts = vp8e_partitions_log2(mbh);
    p.n_parts = 1u << p.log2_parts;
    return p;
}

// ---- colour: BGRA -> Y and 2x2-averaged U, V, BT.601 studio range in 16-bit fixed point (the inverse of vp8_yuv_to_bgra) ----
IFHIP_HD int vp8e_rgb_to_y(int r, int g, int b) { return (16839 * r + 33059 * g + 6420 * b + (1 << 15) + (16 << 16)) >> 16; }
IFHIP_HD int vp8e_clip_uv(int uv) { return vp8_clip8((uv + (2 << 16) + (128 << 18)) >> 18); }      // over the sums of four pixels
IFHIP_HD int vp8e_rgb_to_u(int r, int g, int b) { return vp8e_clip_uv(-9719 * r - 19081 * g + 28800 * b); }
IFHIP_HD int vp8e_rgb_to_v(int r, int g, int b) { return vp8e_clip_uv(28800 * r - 24116 * g - 4684 * b); }
struct Vp8eSource {
    const uint8_t* frame; uint32_t stride, w, h, alpha_meaningful;
    uint8_t *y, *u, *v;                 // source planes of whole macroblocks
    uint32_t* grey;                     // [h][w] B = G = R = alpha, A = 255 (null: no alpha plane is kept)
    uint32_t mbw, mbh;
};
// The 2x2 pixels at chroma position (cx, cy) of the padded planes: columns and rows beyond the picture replicate the last.
// Returns whether one of the picture's own pixels has alpha below 255.
IFHIP_HD uint32_t vp8e_convert_quad(const Vp8eSource& S, uint32_t cx, uint32_t cy) {
    int sr = 0, sg = 0, sb = 0;
    uint32_t translucent = 0;
    VP8_UNROLL
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t px = 2u * cx + (k & 1u), py = 2u * cy + (k >> 1);
        const uint32_t x = px < S.w ? px : S.w - 1u, y = py < S.h ? py : S.h - 1u;
        const uint8_t* p = S.frame + static_cast<size_t>(y) * S.stride + 4u * static_cast<size_t>(x);
        const int b = p[0], g = p[1], r = p[2];
        sr += r; sg += g; sb += b;
        S.y[static_cast<size_t>(py) * (S.mbw * 16u) + px] = static_cast<uint8_t>(vp8e_rgb_to_y(r, g, b));
        if (px < S.w && py < S.h) {
            const uint32_t a = S.alpha_meaningful ? p[3] : 255u;
            if (a != 255u) translucent = 1u;
            if (S.grey) S.grey[static_cast<size_t>(py) * S.w + px] = 0xFF000000u | a << 16 | a << 8 | a;
        }
    }
    S.u[static_cast<size_t>(cy) * (S.mbw * 8u) + cx] = static_cast<uint8_t>(vp8e_rgb_to_u(sr, sg, sb));
    S.v[static_cast<size_t>(cy) * (S.mbw * 8u) + cx] = static_cast<uint8_t>(vp8e_rgb_to_v(sr, sg, sb));
    return translucent;
}

// ---- the forward transforms (the inverses' counterparts with libwebp's scaling: a level is coefficient / step) -----------------
IFHIP_HD void vp8e_fdct(const int* d, int* out) {            // d: 16 differences in raster order
    int tmp[16];
    VP8_UNROLL
    for (int i = 0; i < 4; ++i) {
        const int a0 = d[4 * i] + d[4 * i + 3], a1 = d[4 * i + 1] + d[4 * i + 2], a2 = d[4 * i + 1] - d[4 * i + 2], a3 = d[4 * i] - d[4 * i + 3];
        tmp[4 * i] = (a0 + a1) * 8;
        tmp[4 * i + 1] = (a2 * 2217 + a3 * 5352 + 1812) >> 9;
        tmp[4 * i + 2] = (a0 - a1) * 8;
        tmp[4 * i + 3] = (a3 * 2217 - a2 * 5352 + 937) >> 9;
    }
    VP8_UNROLL
    for (int i = 0; i < 4; ++i) {
        const int a0 = tmp[i] + tmp[12 + i], a1 = tmp[4 + i] + tmp[8 + i], a2 = tmp[4 + i] - tmp[8 + i], a3 = tmp[i] - tmp[12 + i];
        out[i] = (a0 + a1 + 7) >> 4;
        out[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0 ? 1 : 0);
        out[8 + i] = (a0 - a1 + 7) >> 4;
        out[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16;
    }
}
IFHIP_HD void vp8e_fwht(const int* dc, int* out) {           // the sixteen luma DCs in block order
    int tmp[16];
    VP8_UNROLL
    for (int i = 0; i < 4; ++i) {
        const int a0 = dc[4 * i] + dc[4 * i + 2], a1 = dc[4 * i + 1] + dc[4 * i + 3], a2 = dc[4 * i + 1] - dc[4 * i + 3], a3 = dc[4 * i] - dc[4 * i + 2];
        tmp[4 * i] = a0 + a1; tmp[4 * i + 1] = a3 + a2; tmp[4 * i + 2] = a3 - a2; tmp[4 * i + 3] = a0 - a1;
    }
    VP8_UNROLL
    for (int i = 0; i < 4; ++i) {
        const int a0 = tmp[i] + tmp[8 + i], a1 = tmp[4 + i] + tmp[12 + i], a2 = tmp[4 + i] - tmp[12 + i], a3 = tmp[i] - tmp[8 + i];
        out[i] = (a0 + a1) >> 1; out[4 + i] = (a3 + a2) >> 1; out[8 + i] = (a3 - a2) >> 1; out[12 + i] = (a0 - a1) >> 1;
    }
}
// quantisation with a dead zone: bias / 256 of a step is added before the division (128 would round to nearest)
enum : uint32_t { kVp8eBiasY1Ac = 110, kVp8eBiasY2Dc = 96, kVp8eBiasY2Ac = 108, kVp8eBiasUvDc = 110, kVp8eBiasUvAc = 115,
                  kVp8eBiasI4Dc = 96 };          // the DC of a 4x4-mode luma block: a y1 DC level inside the block
IFHIP_HD int vp8e_quantise(int coef, uint32_t step, uint32_t bias) {
    const uint32_t a = static_cast<uint32_t>(vp8_abs(coef));
    uint32_t level = (a + ((step * bias) >> 8)) / step;
    if (level > kVp8eMaxLevel) level = kVp8eMaxLevel;
    return coef < 0 ? -static_cast<int>(level) : static_cast<int>(level);
}
// the estimate of a level's bits for the mode decision
IFHIP_HD uint32_t vp8e_level_bits(int level) {
    uint32_t v = static_cast<uint32_t>(vp8_abs(level)), n = 0;
    if (v == 0u) return 1u;
    while (v > 1u) { v >>= 1; ++n; }
    return 4u + 2u * n;
}
IFHIP_HD uint32_t vp8e_ymode_bits(uint32_t mode) { return mode == 0u || mode == 2u ? 3u : 4u; }      // DC TM V H
IFHIP_HD uint32_t vp8e_uvmode_bits(uint32_t mode) { return mode == 0u ? 1u : mode == 2u ? 2u : mode == 1u ? 3u : 4u; }

// the raster position of zigzag index i (kVp8Zigzag as nibbles: a constant under an unrolled loop, so that a block held in
// registers stays there)
IFHIP_HD constexpr uint32_t vp8e_zigzag(uint32_t i) { return static_cast<uint32_t>(0xFEB7ADC963258410ull >> (4u * i)) & 15u; }
// the number of zigzag positions up to the last non-zero level of a block (0: none), as the decoder's token reader counts them
IFHIP_HD uint32_t vp8e_last(const int16_t* blk) {
    uint32_t n = 0;
    VP8_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) if (blk[vp8e_zigzag(i)]) n = i + 1u;
    return n;
}

// ---- the macroblock's record, exactly as csrc/vp8_read.cpp derives it from the tokens it reads --------------------------------
IFHIP_HD Vp8Mb vp8e_mb_record(const Vp8eParams& p, const int16_t* lv, uint32_t ymode, uint32_t uvmode) {
    Vp8Mb mb{};
    mb.ymode = static_cast<uint8_t>(ymode); mb.uvmode = static_cast<uint8_t>(uvmode);
    bool coded = false;
    if (vp8e_last(lv + 16u * 24u)) {
        mb.nz |= 1u << 24;
        for (uint32_t b = 0; b < 16u && !coded; ++b) coded = vp8_wht_one(lv + 16u * 24u, p.q.y2[0], p.q.y2[1], b) != 0;
    }
    for (uint32_t b = 0; b < 16u; ++b) {
        const uint32_t nz = vp8e_last(lv + 16u * b);
        if (nz > 1u) { mb.nz |= 1u << b; coded = true; }
        if (nz <= 1u) mb.dc_only |= 1u << b; else if (nz <= 3u) mb.ac3 |= 1u << b;
    }
    for (uint32_t ch = 0; ch < 4u; ch += 2u) {
        bool plane_full = false;
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t b = 16u + 2u * ch + k, nz = vp8e_last(lv + 16u * b);
            if (nz) mb.nz |= 1u << b;
            if (nz > 1u) plane_full = true;
            if (nz > 1u || (nz == 1u && static_cast<int16_t>(lv[16u * b] * p.q.uv[0]) != 0)) coded = true;
        }
        if (!plane_full) mb.dc_only |= 0xFu << (16u + 2u * ch);
    }
    mb.limit = p.limit; mb.ilevel = p.ilevel; mb.hev = p.hev;
    mb.inner = coded ? 1 : 0;
    mb.pad = (mb.nz >> 24) & 1u ? 3u : 0u;                  // the Y2 contexts it hands on (vp8e_ctx_left, vp8e_ctx_above): its own Y2 block's
    return mb;
}
// The record of a B_PRED macroblock: sixteen 4x4 modes, no Y2 block, luma blocks that start at their DC, inner edges always
// filtered.  y2_left, y2_above: the Y2 contexts it found, which it hands on as they are (below).
IFHIP_HD Vp8Mb vp8e_mb_record4(const Vp8eParams& p, const int16_t* lv, const uint8_t* imodes, uint32_t uvmode, uint32_t y2_left, uint32_t y2_above) {
    Vp8Mb mb{};
    mb.ymode = static_cast<uint8_t>(kVp8ModeB); mb.uvmode = static_cast<uint8_t>(uvmode);
    for (uint32_t b = 0; b < 16u; ++b) {
        const uint32_t nz = vp8e_last(lv + 16u * b);
        mb.imodes[b] = imodes[b];
        if (nz) mb.nz |= 1u << b;
        if (nz <= 1u) mb.dc_only |= 1u << b; else if (nz <= 3u) mb.ac3 |= 1u << b;
    }
    for (uint32_t ch = 0; ch < 4u; ch += 2u) {
        bool plane_full = false;
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t b = 16u + 2u * ch + k, nz = vp8e_last(lv + 16u * b);
            if (nz) mb.nz |= 1u << b;
            if (nz > 1u) plane_full = true;
        }
        if (!plane_full) mb.dc_only |= 0xFu << (16u + 2u * ch);
    }
    mb.limit = p.limit; mb.ilevel = p.ilevel; mb.hev = p.hev;
    mb.inner = 1;
    mb.pad = static_cast<uint8_t>((y2_left & 1u) | (y2_above & 1u) << 1);
    return mb;
}
// The Y2 context trap: a B_PRED macroblock has no Y2 block and leaves the left and the above Y2 context as it found them, so
// the context of a 16x16 macroblock's Y2 block is that of the NEAREST macroblock with a Y2 block along its row and up its
// column -- two chains, which differ.  Each record carries what it hands on in its pad byte (the decoder does not read it):
// bit 0 to the right, bit 1 downwards.  Row starts and the top row are 0.  The word a macroblock's tokens take for a
// neighbour is its nz with bit 24 replaced by the chain's bit.
IFHIP_HD uint32_t vp8e_ctx_left(const Vp8Mb& left) { return (left.nz & 0xFFFFFFu) | static_cast<uint32_t>(left.pad & 1u) << 24; }
IFHIP_HD uint32_t vp8e_ctx_above(const Vp8Mb& above) { return (above.nz & 0xFFFFFFu) | static_cast<uint32_t>((above.pad >> 1) & 1u) << 24; }
// The sub-mode a neighbouring macroblock shows to the contexts of kVp8BModesProba at its sub-block b: its own where it is B_PRED,
// the sub-mode of its 16x16 mode's number otherwise (DC TM V H -> DC TM VE HE, as csrc/vp8_read.cpp spreads it), B_DC outside the frame.
IFHIP_HD uint32_t vp8e_bmode_of(const Vp8Mb* mb, uint32_t b) { return !mb ? 0u : mb->ymode == kVp8ModeB ? mb->imodes[b] : mb->ymode; }
IFHIP_HD bool vp8e_mb_skipped(const Vp8Mb& mb) { return (mb.nz & 0x1FFFFFFu) == 0u; }

// ---- one macroblock: mode decision, forward path, reconstruction --------------------------------------------------------------
struct Vp8eMbWork {                     // a wave's working set (LDS on the device)
    int16_t lv[4][17 * 16];             // per luma mode: blocks 0..15, then the Y2 block
    int16_t cv[4][8 * 16];              // per chroma mode: U0..U3, V0..V3
    int dcs[4][16];
    uint32_t sse[4][16], bits[4][16], csse[4][8], cbits[4][8];
    uint32_t full[4][2];                // per chroma mode and plane: a block with a second level
    uint32_t ymode, uvmode;
    int16_t res[kVp8MbLevels];
    Vp8Mb mb;
};
struct Vp8eFrame {
    Vp8Planes src, rec;                 // the source and the reconstruction, whole macroblocks
    Vp8Mb* mbs;
    int16_t* levels;                    // [mbw * mbh][400], raster positions inside a block
    Vp8eParams p;
};
// the 16 differences source - prediction of 4x4 block (bx, by) of a plane's macroblock at (x0, y0), `size` 16 or 8
IFHIP_HD void vp8e_block_diff(const uint8_t* src, const uint8_t* rec, uint32_t pitch, uint32_t x0, uint32_t y0, uint32_t size, uint32_t mode, uint32_t bx, uint32_t by,
                              int* d, int* pred) {
    const int dc = mode == 0u ? vp8_dc_large(rec, pitch, x0, y0, size) : 0;
    VP8_UNROLL
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t px = 4u * bx + (i & 3u), py = 4u * by + (i >> 2);
        pred[i] = vp8_pred_large(rec, pitch, x0, y0, mode, px, py, dc);
        d[i] = static_cast<int>(src[static_cast<size_t>(y0 + py) * pitch + x0 + px]) - pred[i];
    }
}
// The trial of the whole-macroblock modes: W.ymode, W.uvmode and the levels of every mode in W.  luma_cost (nullable): where
// lane 0 leaves the chosen luma mode's squared error + lambda * bits.
template <typename Sync>
IFHIP_HD void vp8e_try_mb(const Vp8eFrame& F, Vp8eMbWork& W, uint32_t mbx, uint32_t mby, uint32_t lane, uint32_t nlanes, Sync sync, uint64_t* luma_cost) {
    const Vp8Quant& q = F.p.q;
    // luma, phase 1: every (mode, block) -- prediction, differences, forward DCT; the AC levels, the DC set aside for the WHT
    for (uint32_t t = lane; t < 64u; t += nlanes) {
        const uint32_t mode = t >> 4, b = t & 15u;
        int d[16], pred[16], c[16];
        vp8e_block_diff(F.src.y, F.rec.y, F.src.ypitch, mbx * 16u, mby * 16u, 16u, mode, b & 3u, b >> 2, d, pred);
        vp8e_fdct(d, c);
        W.dcs[mode][b] = c[0];
        W.lv[mode][16u * b] = 0;
        uint32_t bits = 0;
        VP8_UNROLL
        for (uint32_t i = 1; i < 16u; ++i) { const int l = vp8e_quantise(c[i], q.y1[1], kVp8eBiasY1Ac); W.lv[mode][16u * b + i] = static_cast<int16_t>(l); bits += vp8e_level_bits(l); }
        W.bits[mode][b] = bits;
    }
    sync();
    // phase 2: per mode, the WHT of the sixteen DCs and its levels
    for (uint32_t mode = lane; mode < 4u; mode += nlanes) {
        int c[16];
        vp8e_fwht(W.dcs[mode], c);
        for (uint32_t i = 0; i < 16u; ++i) W.lv[mode][256u + i] = static_cast<int16_t>(vp8e_quantise(c[i], i ? q.y2[1] : q.y2[0], i ? kVp8eBiasY2Ac : kVp8eBiasY2Dc));
    }
    sync();
    // phase 3: every (mode, block) reconstructed with the decoder's transforms; its squared error
    for (uint32_t t = lane; t < 64u; t += nlanes) {
        const uint32_t mode = t >> 4, b = t & 15u;
        int d[16], pred[16];
        vp8e_block_diff(F.src.y, F.rec.y, F.src.ypitch, mbx * 16u, mby * 16u, 16u, mode, b & 3u, b >> 2, d, pred);
        int16_t blk[16];
        VP8_UNROLL
        for (uint32_t i = 0; i < 16u; ++i) blk[i] = W.lv[mode][16u * b + i];
        const uint32_t nz = vp8e_last(blk);
        const bool y2 = vp8e_last(W.lv[mode] + 256u) != 0u;
        if (nz > 1u || y2) vp8_residual_block(blk, y2 ? vp8_wht_one(W.lv[mode] + 256u, q.y2[0], q.y2[1], b) : 0, q.y1[1], nz <= 1u, !(nz == 2u || nz == 3u));
        uint32_t sse = 0;
        VP8_UNROLL
        for (uint32_t i = 0; i < 16u; ++i) { const int e = pred[i] + d[i] - vp8_clip8(pred[i] + blk[i]); sse += static_cast<uint32_t>(e * e); }
        W.sse[mode][b] = sse;
    }
    // chroma, phase 1: every (mode, block)
    for (uint32_t t = lane; t < 32u; t += nlanes) {
        const uint32_t mode = t >> 3, b = t & 7u, k = b & 3u;
        const uint8_t* src = b < 4u ? F.src.u : F.src.v;
        const uint8_t* rec = b < 4u ? F.rec.u : F.rec.v;
        int d[16], pred[16], c[16];
        vp8e_block_diff(src, rec, F.src.uvpitch, mbx * 8u, mby * 8u, 8u, mode, k & 1u, k >> 1, d, pred);
        vp8e_fdct(d, c);
        uint32_t bits = 0;
        VP8_UNROLL
        for (uint32_t i = 0; i < 16u; ++i) {
            const int l = vp8e_quantise(c[i], i ? q.uv[1] : q.uv[0], i ? kVp8eBiasUvAc : kVp8eBiasUvDc);
            W.cv[mode][16u * b + i] = static_cast<int16_t>(l); bits += vp8e_level_bits(l);
        }
        W.cbits[mode][b] = bits;
    }
    sync();
    for (uint32_t t = lane; t < 8u; t += nlanes) {           // per (mode, plane): a block with a second level takes the plane to the full transform
        const uint32_t mode = t >> 1, plane = t & 1u;
        uint32_t full = 0;
        for (uint32_t k = 0; k < 4u; ++k) if (vp8e_last(W.cv[mode] + 16u * (4u * plane + k)) > 1u) full = 1u;
        W.full[mode][plane] = full;
    }
    sync();
    for (uint32_t t = lane; t < 32u; t += nlanes) {
        const uint32_t mode = t >> 3, b = t & 7u, k = b & 3u;
        const uint8_t* src = b < 4u ? F.src.u : F.src.v;
        const uint8_t* rec = b < 4u ? F.rec.u : F.rec.v;
        int d[16], pred[16];
        vp8e_block_diff(src, rec, F.src.uvpitch, mbx * 8u, mby * 8u, 8u, mode, k & 1u, k >> 1, d, pred);
        int16_t blk[16];
        VP8_UNROLL
        for (uint32_t i = 0; i < 16u; ++i) blk[i] = W.cv[mode][16u * b + i];
        if (vp8e_last(blk)) vp8_residual_block(blk, vp8_dequant(blk[0], q.uv[0]), q.uv[1], !W.full[mode][b >> 2], true);
        uint32_t sse = 0;
        VP8_UNROLL
        for (uint32_t i = 0; i < 16u; ++i) { const int e = pred[i] + d[i] - vp8_clip8(pred[i] + blk[i]); sse += static_cast<uint32_t>(e * e); }
        W.csse[mode][b] = sse;
    }
    sync();
    // the decision: squared error + lambda * bits, a tie to the lower mode number
    if (lane == 0u) {
        uint64_t best = ~0ull, cbest = ~0ull;
        for (uint32_t mode = 0; mode < 4u; ++mode) {
            uint64_t sse = 0, bits = vp8e_ymode_bits(mode);
            for (uint32_t b = 0; b < 16u; ++b) { sse += W.sse[mode][b]; bits += W.bits[mode][b]; }
            for (uint32_t i = 0; i < 16u; ++i) bits += vp8e_level_bits(W.lv[mode][256u + i]);
            const uint64_t cost = sse + F.p.lambda * bits;
            if (cost < best) { best = cost; W.ymode = mode; }
            uint64_t csse = 0, cbits = vp8e_uvmode_bits(mode);
            for (uint32_t b = 0; b < 8u; ++b) { csse += W.csse[mode][b]; cbits += W.cbits[mode][b]; }
            const uint64_t ccost = csse + F.p.lambda * cbits;
            if (ccost < cbest) { cbest = ccost; W.uvmode = mode; }
        }
        if (luma_cost) *luma_cost = best;
    }
    sync();
}
// the chosen whole-macroblock modes into the frame
template <typename Sync>
IFHIP_HD void vp8e_store_mb(const Vp8eFrame& F, Vp8eMbWork& W, uint32_t mbx, uint32_t mby, uint32_t lane, uint32_t nlanes, Sync sync) {
    const Vp8Quant& q = F.p.q;
    const size_t m = static_cast<size_t>(mby) * F.src.mbw + mbx;
    // the levels of the chosen modes, in the decoder's layout; the record; the decoder's residuals and its store into the planes
    int16_t* out = F.levels + m * kVp8MbLevels;
    for (uint32_t i = lane; i < kVp8MbLevels; i += nlanes) {
        const int16_t v = i < 256u ? W.lv[W.ymode][i] : i < 384u ? W.cv[W.uvmode][i - 256u] : W.lv[W.ymode][256u + (i - 384u)];
        out[i] = v; W.res[i] = v;
    }
    sync();
    if (lane == 0u) { W.mb = vp8e_mb_record(F.p, W.res, W.ymode, W.uvmode); F.mbs[m] = W.mb; }
    sync();
    for (uint32_t b = lane; b < 24u; b += nlanes) vp8_residual_mb_block(W.res, W.mb, q, b);
    sync();
    vp8_predict_mb(F.rec, W.mb, W.res, mbx, mby, lane, nlanes);
    sync();
}
template <typename Sync>
IFHIP_HD void vp8e_code_mb(const Vp8eTables&, const Vp8eFrame& F, Vp8eMbWork& W, uint32_t mbx, uint32_t mby, uint32_t lane, uint32_t nlanes, Sync sync) {
    vp8e_try_mb(F, W, mbx, mby, lane, nlanes, sync, nullptr);
    vp8e_store_mb(F, W, mbx, mby, lane, nlanes, sync);
}

// ---- the sixteen 4x4 luma modes (kVp8eIntra4) ---------------------------------------------------------------------------------------
// Sub-block (bx, by) needs its left, above and above-right neighbours reconstructed: the sub-blocks run on the anti-diagonal
// schedule bx + 2 by, ten steps of at most two sub-blocks, the (sub-block, mode) pairs of a step a lane each.  The candidate
// reconstruction lives in a tile with its edge (vp8_decode_core.hpp), the candidates' levels beside it: nothing of a B_PRED
// trial touches the planes before it has won.
struct Vp8eI4Work {
    uint8_t tile[kVp8TileBytes];
    int16_t cand_lv[20][16];            // per (sub-block of the step, mode): levels, reconstruction, cost
    uint8_t cand_rec[20][16];
    uint64_t cand_cost[20];
    int16_t lv[16][16];                 // the chosen modes' levels
    uint64_t block_cost[16];
    uint8_t imodes[16];
    uint8_t above_modes[4], left_modes[4];      // the sub-mode contexts from the macroblocks above and to the left
    uint64_t cost16, cost4;             // in 1 / 256 of the decision's unit: (squared error + lambda * bits) * 256
    uint32_t y2_left, y2_above, i4;
};
struct Vp8eMb4Work { Vp8eMbWork w; Vp8eI4Work i4; };
IFHIP_HD uint32_t vp8e_i4_first_row(uint32_t step) { return step > 3u ? (step - 2u) >> 1 : 0u; }        // the by of a step's first sub-block: bx = step - 2 by <= 3
IFHIP_HD uint32_t vp8e_i4_count(uint32_t step) { const uint32_t last = step >> 1 < 3u ? step >> 1 : 3u; return last - vp8e_i4_first_row(step) + 1u; }
template <typename Sync>
IFHIP_HD void vp8e_try_intra4(const Vp8eTables& T, const Vp8eFrame& F, Vp8eI4Work& W, uint32_t mbx, uint32_t mby, uint32_t lane, uint32_t nlanes, Sync sync) {
    const Vp8Quant& q = F.p.q;
    const uint32_t mbw = F.src.mbw;
    const size_t m = static_cast<size_t>(mby) * mbw + mbx;
    for (uint32_t i = lane; i < 37u; i += nlanes) vp8_tile_load_edge(W.tile, F.rec.y, F.rec.ypitch, mbw, mbx, mby, i);
    for (uint32_t i = lane; i < 8u; i += nlanes) {
        if (i < 4u) W.above_modes[i] = static_cast<uint8_t>(vp8e_bmode_of(mby ? &F.mbs[m - mbw] : nullptr, 12u + i));
        else W.left_modes[i - 4u] = static_cast<uint8_t>(vp8e_bmode_of(mbx ? &F.mbs[m - 1u] : nullptr, 4u * (i - 4u) + 3u));
    }
    sync();
    for (uint32_t step = 0; step < 10u; ++step) {
        const uint32_t by0 = vp8e_i4_first_row(step), n = vp8e_i4_count(step);
        for (uint32_t t = lane; t < 10u * n; t += nlanes) {
            const uint32_t mode = t % 10u, by = by0 + t / 10u, bx = step - 2u * by, b = 4u * by + bx;
            int Tp[8], L[4], X, pred[16], d[16], c[16];
            vp8_tile_sub_edge(W.tile, bx, by, Tp, L, &X);
            vp8_pred_sub16(mode, Tp, L, X, pred);
            const uint8_t* src = F.src.y + static_cast<size_t>(mby * 16u + 4u * by) * F.src.ypitch + mbx * 16u + 4u * bx;
            VP8_UNROLL
            for (uint32_t i = 0; i < 16u; ++i) d[i] = static_cast<int>(src[static_cast<size_t>(i >> 2) * F.src.ypitch + (i & 3u)]) - pred[i];
            vp8e_fdct(d, c);
            int16_t blk[16];
            uint32_t bits = 0;
            VP8_UNROLL
            for (uint32_t i = 0; i < 16u; ++i) {
                const int l = vp8e_quantise(c[i], i ? q.y1[1] : q.y1[0], i ? kVp8eBiasY1Ac : kVp8eBiasI4Dc);
                blk[i] = static_cast<int16_t>(l); W.cand_lv[t][i] = static_cast<int16_t>(l); bits += vp8e_level_bits(l);
            }
            const uint32_t nz = vp8e_last(blk);
            if (nz) vp8_residual_block(blk, vp8_dequant(blk[0], q.y1[0]), q.y1[1], nz <= 1u, !(nz == 2u || nz == 3u));
            uint32_t sse = 0;
            VP8_UNROLL
            for (uint32_t i = 0; i < 16u; ++i) {
                const int r = vp8_clip8(pred[i] + blk[i]), e = pred[i] + d[i] - r;
                W.cand_rec[t][i] = static_cast<uint8_t>(r); sse += static_cast<uint32_t>(e * e);
            }
            const uint32_t above = by ? W.imodes[b - 4u] : W.above_modes[bx], left = bx ? W.imodes[b - 1u] : W.left_modes[by];
            W.cand_cost[t] = (static_cast<uint64_t>(sse) + static_cast<uint64_t>(F.p.lambda) * bits) * 256u + static_cast<uint64_t>(F.p.lambda) * T.bmode_cost[above][left][mode];
        }
        sync();
        for (uint32_t j = lane; j < n; j += nlanes) {             // the cheapest mode of each sub-block, a tie to the lower number
            const uint32_t by = by0 + j, bx = step - 2u * by, b = 4u * by + bx;
            uint32_t best = 0;
            for (uint32_t mode = 1; mode < 10u; ++mode) if (W.cand_cost[10u * j + mode] < W.cand_cost[10u * j + best]) best = mode;
            const uint32_t t = 10u * j + best;
            W.imodes[b] = static_cast<uint8_t>(best); W.block_cost[b] = W.cand_cost[t];
            uint8_t* dst = W.tile + (1u + 4u * by) * kVp8TilePitch + 1u + 4u * bx;
            for (uint32_t i = 0; i < 16u; ++i) { W.lv[b][i] = W.cand_lv[t][i]; dst[(i >> 2) * kVp8TilePitch + (i & 3u)] = W.cand_rec[t][i]; }
        }
        sync();
    }
}
// One macroblock under kVp8eIntra4: the whole-macroblock trial as ever, the 4x4 trial, and B_PRED where that is cheaper -- each
// side with its bit of the is_i4 flag under its probability 145; a tie goes to 16x16.  The winner is stored once.  Needs the
// macroblocks to the left, above, above-left and above-right finished: skew 2.
template <typename Sync>
IFHIP_HD void vp8e_code_mb4(const Vp8eTables& T, const Vp8eFrame& F, Vp8eMb4Work& W4, uint32_t mbx, uint32_t mby, uint32_t lane, uint32_t nlanes, Sync sync) {
    Vp8eMbWork& W = W4.w;
    Vp8eI4Work& I = W4.i4;
    const Vp8Quant& q = F.p.q;
    const size_t m = static_cast<size_t>(mby) * F.src.mbw + mbx;
    vp8e_try_mb(F, W, mbx, mby, lane, nlanes, sync, &I.cost16);
    vp8e_try_intra4(T, F, I, mbx, mby, lane, nlanes, sync);
    if (lane == 0u) {
        uint64_t c4 = static_cast<uint64_t>(F.p.lambda) * (vp8e_cost(145u) + 256u * F.p.i4_penalty);
        for (uint32_t b = 0; b < 16u; ++b) c4 += I.block_cost[b];
        I.cost4 = c4;
        I.cost16 = I.cost16 * 256u + static_cast<uint64_t>(F.p.lambda) * vp8e_cost(256u - 145u);
        I.i4 = I.cost4 < I.cost16 ? 1u : 0u;
        I.y2_left = mbx ? F.mbs[m - 1u].pad & 1u : 0u;
        I.y2_above = mby ? (F.mbs[m - F.src.mbw].pad >> 1) & 1u : 0u;
    }
    sync();
    if (!I.i4) { vp8e_store_mb(F, W, mbx, mby, lane, nlanes, sync); return; }      // (uniform over the lanes)
    int16_t* out = F.levels + m * kVp8MbLevels;
    for (uint32_t i = lane; i < kVp8MbLevels; i += nlanes) {
        const int16_t v = i < 256u ? I.lv[i >> 4][i & 15u] : i < 384u ? W.cv[W.uvmode][i - 256u] : 0;
        out[i] = v; W.res[i] = v;
    }
    sync();
    if (lane == 0u) { W.mb = vp8e_mb_record4(F.p, W.res, I.imodes, W.uvmode, I.y2_left, I.y2_above); F.mbs[m] = W.mb; }
    sync();
    for (uint32_t b = 16u + lane; b < 24u; b += nlanes) vp8_residual_mb_block(W.res, W.mb, q, b);
    sync();
    for (uint32_t i = lane; i < 256u; i += nlanes)             // luma: the tile holds what the decoder's vp8_predict_sub will make of these levels
        F.rec.y[static_cast<size_t>(mby * 16u + (i >> 4)) * F.rec.ypitch + mbx * 16u + (i & 15u)] = I.tile[(1u + (i >> 4)) * kVp8TilePitch + 1u + (i & 15u)];
    vp8_predict_mb_chroma(F.rec, W.mb, W.res, mbx, mby, lane, nlanes);
    sync();
}

// ---- tokens: one walk for the statistics and for the bool coder ---------------------------------------------------------------------
// Sink: coef(bit, type, band, ctx, node) for a bit under a coefficient probability, fixed(bit, prob) for the others.
IFHIP_HD uint32_t vp8e_prob_index(uint32_t type, uint32_t band, uint32_t ctx, uint32_t node) { return ((type * 8u + band) * 3u + ctx) * 11u + node; }
template <typename Sink>
IFHIP_HD void vp8e_put_block(const Vp8eTables& T, const int16_t* blk, uint32_t type, uint32_t ctx, uint32_t first, Sink& s) {
    const uint32_t last = vp8e_last(blk);                 // (for first == 1 position 0 is zero)
    uint32_t n = first, band = T.bands[n];
    while (n < 16u) {
        if (n >= last) { s.coef(0u, type, band, ctx, 0u); return; }
        s.coef(1u, type, band, ctx, 0u);
        while (!blk[vp8e_zigzag(n)]) { s.coef(0u, type, band, ctx, 1u); ++n; band = T.bands[n]; ctx = 0u; }
        s.coef(1u, type, band, ctx, 1u);
        const int level = blk[vp8e_zigzag(n)];
        const uint32_t v = static_cast<uint32_t>(vp8_abs(level));
        if (v == 1u) s.coef(0u, type, band, ctx, 2u);
        else {
            s.coef(1u, type, band, ctx, 2u);
            if (v <= 4u) {
                s.coef(0u, type, band, ctx, 3u);
                if (v == 2u) s.coef(0u, type, band, ctx, 4u); else { s.coef(1u, type, band, ctx, 4u); s.coef(v - 3u, type, band, ctx, 5u); }
            } else if (v <= 10u) {
                s.coef(1u, type, band, ctx, 3u); s.coef(0u, type, band, ctx, 6u);
                if (v <= 6u) { s.coef(0u, type, band, ctx, 7u); s.fixed(v - 5u, 159u); }
                else { s.coef(1u, type, band, ctx, 7u); s.fixed((v - 7u) >> 1, 165u); s.fixed((v - 7u) & 1u, 145u); }
            } else {
                const uint32_t cat = v <= 18u ? 0u : v <= 34u ? 1u : v <= 66u ? 2u : 3u, nbits = cat == 3u ? 11u : 3u + cat;
                s.coef(1u, type, band, ctx, 3u); s.coef(1u, type, band, ctx, 6u); s.coef(cat >> 1, type, band, ctx, 8u); s.coef(cat & 1u, type, band, ctx, 9u + (cat >> 1));
                const uint32_t extra = v - 3u - (8u << cat);
                for (uint32_t i = 0; i < nbits; ++i) s.fixed((extra >> (nbits - 1u - i)) & 1u, T.cat[cat][i]);
            }
        }
        s.fixed(level < 0 ? 1u : 0u, 128u);
        ++n; band = T.bands[n]; ctx = v == 1u ? 1u : 2u;
    }
}
// The tokens of a macroblock that is not skipped.  above, left: vp8e_ctx_above / vp8e_ctx_left of those macroblocks' records (0
// outside the frame; their nz words where no macroblock of the frame is B_PRED): a block's context is the sum of the non-zero
// flags of the blocks above it and to its left, which depend on their levels alone; bit 24 is the Y2 chain's (above).
template <typename Sink>
IFHIP_HD void vp8e_mb_tokens(const Vp8eTables& T, const int16_t* lv, const Vp8Mb& mb, uint32_t above, uint32_t left, Sink& s) {
    const bool i4 = mb.ymode == kVp8ModeB;                 // no Y2 block; luma blocks of type 3 from their first coefficient
    if (!i4) vp8e_put_block(T, lv + 16u * 24u, 1u, ((above >> 24) & 1u) + ((left >> 24) & 1u), 0u, s);
    for (uint32_t b = 0; b < 16u; ++b) {
        const uint32_t t = b < 4u ? (above >> (12u + b)) & 1u : (mb.nz >> (b - 4u)) & 1u;
        const uint32_t l = (b & 3u) == 0u ? (left >> (b + 3u)) & 1u : (mb.nz >> (b - 1u)) & 1u;
        vp8e_put_block(T, lv + 16u * b, i4 ? 3u : 0u, t + l, i4 ? 0u : 1u, s);
    }
    for (uint32_t b = 16u; b < 24u; ++b) {
        const uint32_t k = (b - 16u) & 3u;
        const uint32_t t = k < 2u ? (above >> (b + 2u)) & 1u : (mb.nz >> (b - 2u)) & 1u;
        const uint32_t l = (k & 1u) == 0u ? (left >> (b + 1u)) & 1u : (mb.nz >> (b - 1u)) & 1u;
        vp8e_put_block(T, lv + 16u * b, 2u, t + l, 0u, s);
    }
}

// ---- probabilities -----------------------------------------------------------------------------------------------------------------
// 256 * log2(256 / p) for p in 1..256, by integer squaring (eight fraction bits)
IFHIP_HD uint32_t vp8e_cost(uint32_t p) {
    uint32_t n = 0;
    while ((p >> n) > 1u) ++n;
    uint64_t m = static_cast<uint64_t>(p) << (31u - n);         // [2^31, 2^32)
    uint32_t frac = 0;
    for (uint32_t i = 0; i < 8u; ++i) {
        m = (m * m) >> 31;
        frac <<= 1;
        if (m >> 32) { frac |= 1u; m >>= 1; }
    }
    return 8u * 256u - (n * 256u + frac);
}
IFHIP_HD uint64_t vp8e_branch_cost(uint32_t n0, uint32_t n1, uint32_t p) { return static_cast<uint64_t>(n0) * vp8e_cost(p) + static_cast<uint64_t>(n1) * vp8e_cost(256u - p); }
// the probability of a zero from the counts of zeros and ones, 1..255
IFHIP_HD uint32_t vp8e_prob_from_counts(uint32_t n0, uint32_t n1) {
    const uint64_t total = static_cast<uint64_t>(n0) + n1;
    if (!total) return 255u;
    const uint32_t p = 255u - static_cast<uint32_t>(static_cast<uint64_t>(n1) * 255u / total);
    return p < 1u ? 1u : p;
}
// A coefficient probability is updated where that saves bits: the update flag costs what its own probability says, the new
// value 8 bits.  Returns the probability in force; *updated says whether it is written.
IFHIP_HD uint32_t vp8e_decide_prob(uint32_t n0, uint32_t n1, uint32_t old_p, uint32_t update_p, uint32_t* updated) {
    const uint32_t new_p = vp8e_prob_from_counts(n0, n1);
    const uint64_t keep = vp8e_branch_cost(n0, n1, old_p) + vp8e_cost(update_p);
    const uint64_t change = vp8e_branch_cost(n0, n1, new_p) + vp8e_cost(256u - update_p) + 8u * 256u;
    *updated = new_p != old_p && change < keep ? 1u : 0u;
    return *updated ? new_p : old_p;
}
IFHIP_HD uint32_t vp8e_skip_prob(uint32_t n_skipped, uint32_t n_mbs) { return vp8e_prob_from_counts(n_mbs - n_skipped, n_skipped); }

// ---- the bool coder (RFC 6386 7.3) in the run-deferred form ------------------------------------------------------------------------
// The last byte that a carry may still reach is held back together with the count of 0xFF bytes behind it; the next byte or
// carry resolves them.  No byte that was stored is ever revisited.  Stores beyond `cap` are dropped and counted.
struct Vp8eBool {
    uint8_t* out; uint32_t cap, pos;
    uint32_t range, bottom; int bit_count;
    int held; uint32_t run;
    IFHIP_HD void init(uint8_t* o, uint32_t capacity) { out = o; cap = capacity; pos = 0; range = 255u; bottom = 0u; bit_count = 24; held = -1; run = 0u; }
    IFHIP_HD void store(uint32_t b) { if (pos < cap) out[pos] = static_cast<uint8_t>(b); ++pos; }
    IFHIP_HD void resolve(uint32_t carry) {
        if (held >= 0) store(static_cast<uint32_t>(held) + carry);
        for (; run; --run) store(carry ? 0u : 255u);
        held = -1;
    }
    IFHIP_HD void carry() {
        if (run) { const uint32_t zeros = run - 1u; run = 0u; if (held >= 0) store(static_cast<uint32_t>(held) + 1u); for (uint32_t i = 0; i < zeros; ++i) store(0u); held = 0; }
        else if (held >= 0) ++held;
    }
    IFHIP_HD void append(uint32_t b) {
        if (b == 255u) { ++run; return; }
        resolve(0u);
        held = static_cast<int>(b);
    }
    IFHIP_HD void put(uint32_t bit, uint32_t prob) {
        const uint32_t split = 1u + (((range - 1u) * prob) >> 8);
        if (bit) { bottom += split; range -= split; } else range = split;
        while (range < 128u) {
            range <<= 1;
            if (bottom & 0x80000000u) carry();
            bottom <<= 1;
            if (--bit_count == 0) { append(bottom >> 24); bottom &= 0xFFFFFFu; bit_count = 8; }
        }
    }
    IFHIP_HD void value(uint32_t v, uint32_t bits) { for (uint32_t i = bits; i-- > 0u;) put((v >> i) & 1u, 128u); }
    IFHIP_HD uint32_t finish() {                             // -> the stream's bytes (beyond cap: it did not fit)
        const int c = bit_count;
        uint32_t v = bottom;
        if (v & (1u << (32 - c))) carry();
        v <<= c & 7;
        for (int i = c >> 3; i > 0; --i) v <<= 8;
        for (int i = 0; i < 4; ++i) { append(v >> 24); v <<= 8; }
        resolve(0u);
        return pos;
    }
};
struct Vp8eCountSink {                  // the statistics: counts[index][bit]
    uint32_t* counts;
    IFHIP_HD void coef(uint32_t bit, uint32_t type, uint32_t band, uint32_t ctx, uint32_t node) { ++counts[2u * vp8e_prob_index(type, band, ctx, node) + bit]; }
    IFHIP_HD void fixed(uint32_t, uint32_t) {}
};
struct Vp8eCodeSink {
    Vp8eBool* e; const uint8_t* probs;
    IFHIP_HD void coef(uint32_t bit, uint32_t type, uint32_t band, uint32_t ctx, uint32_t node) { e->put(bit, probs[vp8e_prob_index(type, band, ctx, node)]); }
    IFHIP_HD void fixed(uint32_t bit, uint32_t prob) { e->put(bit, prob); }
};

// the first partition: the frame header, the probability updates, then skip flag and modes of every macroblock
// (mbw: the macroblocks of a row, for the sub-mode contexts of B_PRED macroblocks; a frame without them does not look at it)
IFHIP_HD uint32_t vp8e_first_partition(const Vp8eTables& T, const Vp8eParams& p, const uint8_t* probs, const uint8_t* updated, uint32_t skip_p, const Vp8Mb* mbs, size_t n_mbs,
                                       uint8_t* out, uint32_t cap, uint32_t mbw = 0u) {
    Vp8eBool e;
    e.init(out, cap);
    e.put(0u, 128u); e.put(0u, 128u);                         // colour space, clamping type
    e.put(0u, 128u);                                          // no segments
    e.put(0u, 128u); e.value(p.filter_level, 6u); e.value(0u, 3u);     // the normal filter, its level, sharpness 0
    e.put(0u, 128u);                                          // no filter deltas
    e.value(p.log2_parts, 2u);
    e.value(p.index, 7u);
    for (uint32_t i = 0; i < 5u; ++i) e.put(0u, 128u);        // the five quantiser deltas
    e.put(0u, 128u);                                          // refresh entropy probabilities
    for (uint32_t i = 0; i < kVp8eProbs; ++i) {
        e.put(updated[i], T.update[i]);
        if (updated[i]) e.value(probs[i], 8u);
    }
    e.put(1u, 128u); e.value(skip_p, 8u);
    for (size_t m = 0; m < n_mbs; ++m) {
        const Vp8Mb& mb = mbs[m];
        e.put(vp8e_mb_skipped(mb) ? 1u : 0u, skip_p);
        if (mb.ymode == kVp8ModeB) {
            e.put(0u, 145u);
            const Vp8Mb* above = m >= mbw ? &mbs[m - mbw] : nullptr;
            const Vp8Mb* left = m % mbw ? &mbs[m - 1u] : nullptr;
            for (uint32_t b = 0; b < 16u; ++b) {
                const uint32_t a = b >= 4u ? mb.imodes[b - 4u] : vp8e_bmode_of(above, 12u + b), l = (b & 3u) ? mb.imodes[b - 1u] : vp8e_bmode_of(left, b + 3u);
                const uint8_t* path = T.bmode_path[mb.imodes[b]];
                for (uint32_t i = 0; i < path[0]; ++i) e.put(path[1u + i] & 1u, T.bmode_proba[a][l][path[1u + i] >> 1]);
            }
        } else {
            e.put(1u, 145u);
            if (mb.ymode == 1u || mb.ymode == 3u) { e.put(1u, 156u); e.put(mb.ymode == 1u ? 1u : 0u, 128u); }
            else { e.put(0u, 156u); e.put(mb.ymode == 2u ? 1u : 0u, 163u); }
        }
        if (mb.uvmode == 0u) e.put(0u, 142u);
        else if (mb.uvmode == 2u) { e.put(1u, 142u); e.put(0u, 114u); }
        else { e.put(1u, 142u); e.put(1u, 114u); e.put(mb.uvmode == 1u ? 1u : 0u, 183u); }
    }
    return e.finish();
}
// token partition `part` of n_parts: the macroblock rows part, part + n_parts, ...
IFHIP_HD uint32_t vp8e_token_partition(const Vp8eTables& T, const uint8_t* probs, const Vp8Mb* mbs, const int16_t* levels, uint32_t mbw, uint32_t mbh, uint32_t part, uint32_t n_parts,
                                       uint8_t* out, uint32_t cap) {
    Vp8eBool e;
    e.init(out, cap);
    Vp8eCodeSink s{&e, probs};
    for (uint32_t y = part; y < mbh; y += n_parts)
        for (uint32_t x = 0; x < mbw; ++x) {
            const size_t m = static_cast<size_t>(y) * mbw + x;
            if (vp8e_mb_skipped(mbs[m])) continue;
            vp8e_mb_tokens(T, levels + m * kVp8MbLevels, mbs[m], y ? vp8e_ctx_above(mbs[m - mbw]) : 0u, x ? vp8e_ctx_left(mbs[m - 1u]) : 0u, s);
        }
    return e.finish();
}

// ---- sizes -------------------------------------------------------------------------------------------------------------------------
// What a stream can take at most.  A bit under a coefficient probability costs at most 3 bits on average over its node: the
// node either keeps its default or is updated to its own frequency (8 bits of rounding slack within 1 / 256), whichever is
// cheaper.  A level has at most 7 such bits, the 11 extra bits of the last category cost 31 bits under their fixed
// probabilities when all are set, the sign 1: 53 bits a coefficient, 400 coefficients and 25 ends of block a macroblock.
// The streams are stored with a bound check all the same: a stream that outgrew this raises the overflow word.
constexpr uint32_t kVp8eMbTokenBytes = (400u * 53u + 25u * 3u + 7u) / 8u + 4u;
constexpr uint32_t kVp8eMbModeBytes = 2u;                    // skip flag (3 bits by the same argument) + 7.4 bits of modes
constexpr uint32_t kVp8eHeaderBytes = (kVp8eProbs * 17u + 64u) / 8u + 8u;
// Under kVp8eIntra4 a macroblock's modes are at most: the skip flag (3 bits), the is_i4 bit under 145, sixteen times the dearest
// leaf of kVp8BModesProba over all contexts (computed from the table: Vp8eTables::bmode_dearest, 15.3 bits) and the dearest
// chroma mode: 32 bytes.  The frame tag's 19 bits (kVp8eFirstPartMax) cap the first partition's bound from 16 313 macroblocks
// on; a real first partition of B_PRED macroblocks (4.4 bytes each on photo-like content) outgrows them at about 120 000.
// (host only)
inline uint32_t vp8e_mb_mode_bytes(uint32_t flags) {
    if (!(flags & kVp8eIntra4)) return kVp8eMbModeBytes;
    const uint32_t uv = vp8e_cost(256u - 142u) + vp8e_cost(256u - 114u) + vp8e_cost(256u - 183u);       // (the dearer of node 183's two sides)
    const uint32_t bits256 = 3u * 256u + vp8e_cost(145u) + 16u * vp8e_host_tables().bmode_dearest + uv;
    const uint32_t bytes = (bits256 + 2047u) / 2048u;
    return bytes > kVp8eMbModeBytes ? bytes : kVp8eMbModeBytes;
}
inline uint64_t vp8e_first_cap(uint64_t n_mbs, uint32_t flags = 0u) { return kVp8eHeaderBytes + n_mbs * vp8e_mb_mode_bytes(flags); }
IFHIP_HD uint64_t vp8e_part_cap(uint32_t mbw, uint32_t mbh, uint32_t n_parts) { return 8u + static_cast<uint64_t>(mbw) * ((mbh + n_parts - 1u) / n_parts) * kVp8eMbTokenBytes; }
// alph_bound: the inner lossless coder's bound on a file of the grey frame (0: no alpha plane)
inline uint64_t vp8e_max_file_bytes(uint32_t w, uint32_t h, uint64_t alph_bound, uint32_t flags = 0u) {
    const uint32_t mbw = (w + 15u) / 16u, mbh = (h + 15u) / 16u, n_parts = 1u << vp8e_partitions_log2(mbh);
    uint64_t first = vp8e_first_cap(static_cast<uint64_t>(mbw) * mbh, flags);
    if (first > kVp8eFirstPartMax) first = kVp8eFirstPartMax;
    uint64_t n = 12u + 8u + 10u + first + 3u * (n_parts - 1u) + n_parts * vp8e_part_cap(mbw, mbh, n_parts) + 1u;
    if (alph_bound) n += 18u + 8u + alph_bound + 1u;
    return n;
}

// ---- the file: a list of pieces, and the byte at any offset ------------------------------------------------------------------------------
struct Vp8eLayout {
    uint32_t w, h, alpha;               // alpha: the file carries VP8X + ALPH
    uint32_t alph_len;                  // the ALPH chunk's body: 1 header byte + the headless VP8L stream
    const uint8_t* alph_stream;         // the inner file's payload behind its five header bytes
    uint32_t first_len, n_parts;
    const uint8_t* first;
    const uint8_t* part[8];
    uint32_t part_len[8];
    uint32_t vp8_len, file_len;         // set by vp8e_layout_sizes
    uint32_t vp8_at, alph_at;           // where the `VP8 ` and `ALPH` chunk headers start
};
IFHIP_HD void vp8e_layout_sizes(Vp8eLayout& L) {
    uint64_t n = 10u + static_cast<uint64_t>(L.first_len) + 3u * (L.n_parts - 1u);
    for (uint32_t i = 0; i < L.n_parts; ++i) n += L.part_len[i];
    L.vp8_len = static_cast<uint32_t>(n);
    uint32_t at = 12u;
    L.alph_at = 0u;
    if (L.alpha) { at += 18u; L.alph_at = at; at += 8u + L.alph_len + (L.alph_len & 1u); }
    L.vp8_at = at;
    L.file_len = at + 8u + L.vp8_len + (L.vp8_len & 1u);
}
IFHIP_HD uint32_t vp8e_le_byte(uint32_t v, uint32_t k) { return (v >> (8u * k)) & 255u; }
IFHIP_HD uint32_t vp8e_tag_byte(const char* tag, uint32_t size, uint32_t k) { return k < 4u ? static_cast<uint8_t>(tag[k]) : vp8e_le_byte(size, k - 4u); }
IFHIP_HD uint32_t vp8e_file_byte(const Vp8eLayout& L, uint32_t i) {
    if (i >= L.file_len) return 0u;                          // the zeros behind the file (and its pad bytes, below)
    if (i < 12u) return i < 8u ? vp8e_tag_byte("RIFF", L.file_len - 8u, i) : static_cast<uint8_t>("WEBP"[i - 8u]);
    if (L.alpha) {
        if (i < 30u) {
            const uint32_t k = i - 12u;
            if (k < 8u) return vp8e_tag_byte("VP8X", 10u, k);
            if (k == 8u) return 0x10u;                       // the alpha flag
            if (k < 12u) return 0u;
            return k < 15u ? vp8e_le_byte(L.w - 1u, k - 12u) : vp8e_le_byte(L.h - 1u, k - 15u);
        }
        if (i < L.vp8_at) {
            const uint32_t k = i - L.alph_at;
            if (k < 8u) return vp8e_tag_byte("ALPH", L.alph_len, k);
            if (k == 8u) return 0x01u;                       // VP8L-coded, no filter, no pre-processing
            return k - 8u < L.alph_len ? L.alph_stream[k - 9u] : 0u;
        }
    }
    uint32_t k = i - L.vp8_at;
    if (k < 8u) return vp8e_tag_byte("VP8 ", L.vp8_len, k);
    k -= 8u;
    if (k < 3u) return vp8e_le_byte((1u << 4) | (L.first_len << 5), k);      // key frame, profile 0, shown
    if (k < 6u) return k == 3u ? 0x9Du : k == 4u ? 0x01u : 0x2Au;
    if (k < 10u) return k < 8u ? vp8e_le_byte(L.w, k - 6u) : vp8e_le_byte(L.h, k - 8u);
    k -= 10u;
    if (k < L.first_len) return L.first[k];
    k -= L.first_len;
    if (k < 3u * (L.n_parts - 1u)) return vp8e_le_byte(L.part_len[k / 3u], k % 3u);
    k -= 3u * (L.n_parts - 1u);
    for (uint32_t p = 0; p < L.n_parts; ++p) {
        if (k < L.part_len[p]) return L.part[p][k];
        k -= L.part_len[p];
    }
    return 0u;                                               // the pad byte
}

}  // namespace ifhip
