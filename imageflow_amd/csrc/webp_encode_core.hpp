// webp_encode_core.hpp -- the arithmetic of the device lossless-WebP coder (csrc/webp_encode.hip), written so that it
// compiles for the gfx950 kernels AND for a plain host compiler: tests/webp_emulate.cpp runs the same predictor choice,
// the same parse, the same code construction and the same bit placement on the CPU, and libwebp must decode what comes
// out to the source pixels -- test infrastructure; the product has one path, the kernels.
//
// What is coded: EncoderPreset::WebPLossless (codecs/webp.rs:281-345, codecs/auto.rs:282-319: WebPEncodeLosslessBGRA /
// WebPEncodeLosslessBGR): a VP8L stream in a RIFF container.  A lossless coder is free in its choices; these are this
// coder's own: subtract green, a predictor per 16 x 16 tile, LZ77 over the residual pixels at the two distances image
// data favours (one pixel back, one row up), a group of five prefix codes per band of 64 rows, no colour cache.  Every
// rule of the format with a bit in it lives here.  The code construction (lengths of at most 15 bits, canonical codes,
// the run-length coded header) is prefix_code_core.hpp's, shared with the deflate back end: VP8L took both from deflate.
#pragma once
#include <cstdint>

#include "prefix_code_core.hpp"

namespace ifhip {

constexpr uint32_t kWebpMaxDim = 16384;                 // 14 bits of width - 1 and height - 1
constexpr uint32_t kWebpTileBits = 4, kWebpTile = 1u << kWebpTileBits;     // predictor tiles
constexpr uint32_t kWebpBandBits = 6, kWebpBand = 1u << kWebpBandBits;     // entropy tiles; a band is one row of them: at most 256 groups
constexpr uint32_t kWebpSeg = 4096;                     // pixels a workgroup parses and emits; segments do not cross bands
constexpr uint32_t kWebpMinMatch = 3, kWebpMaxMatch = 4096;
constexpr uint32_t kWebpG = 0, kWebpR = 280, kWebpB = 536, kWebpA = 792, kWebpD = 1048, kWebpSyms = 1088;   // the five alphabets of a group
constexpr uint32_t kWebpGroupWords = 512;               // a group's five code headers: at most 3983 + 3 * 3647 + 623 = 15547 bits
constexpr uint32_t kWebpSubWords = 256;                 // a sub-image's: one alphabet of many symbols, four of one
constexpr uint32_t kWebpRiff = 20;                      // "RIFF" size "WEBP" "VP8L" size
constexpr uint32_t kWebpFileOverflow = 1;
constexpr uint32_t kWebpSegMaxBits = kWebpSeg * 60u;    // four codes of 15 bits per literal pixel

IFHIP_HD uint32_t webp_alphabet_offset(uint32_t a) { return a == 0u ? kWebpG : a == 1u ? kWebpR : a == 2u ? kWebpB : a == 3u ? kWebpA : kWebpD; }
IFHIP_HD uint32_t webp_alphabet_size(uint32_t a) { return a == 0u ? 280u : a == 4u ? 40u : 256u; }

// ---- geometry ---------------------------------------------------------------------------------------------------------------
struct WebpShape {
    uint32_t w, h, tiles_x, tiles_y, ent_x, n_bands, segs_per_band, n_segs;
};
IFHIP_HD WebpShape webp_shape(uint32_t w, uint32_t h) {
    WebpShape s;
    s.w = w; s.h = h;
    s.tiles_x = (w + kWebpTile - 1u) >> kWebpTileBits; s.tiles_y = (h + kWebpTile - 1u) >> kWebpTileBits;
    s.ent_x = (w + kWebpBand - 1u) >> kWebpBandBits; s.n_bands = (h + kWebpBand - 1u) >> kWebpBandBits;
    s.segs_per_band = (w * kWebpBand + kWebpSeg - 1u) / kWebpSeg;
    s.n_segs = s.segs_per_band * s.n_bands;
    return s;
}
// segment `seg` covers the pixels [*start, *start + n) of the image in scan order (n may be 0 in the last band)
IFHIP_HD uint32_t webp_segment(const WebpShape& s, uint32_t seg, uint32_t* start) {
    const uint32_t band = seg / s.segs_per_band, j = seg % s.segs_per_band;
    const uint32_t rows = s.h - band * kWebpBand < kWebpBand ? s.h - band * kWebpBand : kWebpBand;
    const uint32_t band_px = rows * s.w, off = j * kWebpSeg;
    *start = band * kWebpBand * s.w + off;
    return off >= band_px ? 0u : band_px - off < kWebpSeg ? band_px - off : kWebpSeg;
}

// ---- transforms -------------------------------------------------------------------------------------------------------------
// BGRA bytes read as a little-endian dword are VP8L's ARGB
IFHIP_HD uint32_t webp_sub_green(uint32_t p) {
    const uint32_t g = (p >> 8) & 255u;
    return (p & 0xFF00FF00u) | (((p & 0x00FF00FFu) + 0x01000100u - g * 0x00010001u) & 0x00FF00FFu);
}
IFHIP_HD uint32_t webp_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
IFHIP_HD int webp_iabs(int v) { return v < 0 ? -v : v; }
IFHIP_HD uint32_t webp_clamp8(int v) { return v < 0 ? 0u : v > 255 ? 255u : static_cast<uint32_t>(v); }
IFHIP_HD uint32_t webp_predict(uint32_t mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (mode) {
    case 0: return 0xFF000000u;
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return webp_avg2(webp_avg2(L, TR), T);
    case 6: return webp_avg2(L, TL);
    case 7: return webp_avg2(L, T);
    case 8: return webp_avg2(TL, T);
    case 9: return webp_avg2(T, TR);
    case 10: return webp_avg2(webp_avg2(L, TL), webp_avg2(T, TR));
    case 11: {                                          // Select: over all four channels; L when its distance is strictly smaller
        int dl = 0, dt = 0;
        for (uint32_t s = 0; s < 32u; s += 8u) {
            const int l = (L >> s) & 255, t = (T >> s) & 255, tl = (TL >> s) & 255;
            dl += webp_iabs(t - tl);                    // |L + T - TL - L|
            dt += webp_iabs(l - tl);
        }
        return dl < dt ? L : T;
    }
    case 12: {
        uint32_t r = 0;
        for (uint32_t s = 0; s < 32u; s += 8u)
            r |= webp_clamp8(static_cast<int>((L >> s) & 255u) + static_cast<int>((T >> s) & 255u) - static_cast<int>((TL >> s) & 255u)) << s;
        return r;
    }
    default: {                                          // 13: the division truncates toward zero
        const uint32_t av = webp_avg2(L, T);
        uint32_t r = 0;
        for (uint32_t s = 0; s < 32u; s += 8u) {
            const int a = (av >> s) & 255, b = (TL >> s) & 255;
            r |= webp_clamp8(a + (a - b) / 2) << s;
        }
        return r;
    }
    }
}
IFHIP_HD uint32_t webp_sub_pixels(uint32_t a, uint32_t b) {             // per channel, modulo 256
    const uint32_t ag = 0x00FF00FFu + (a & 0xFF00FF00u) - (b & 0xFF00FF00u), rb = 0xFF00FF00u + (a & 0x00FF00FFu) - (b & 0x00FF00FFu);
    return (ag & 0xFF00FF00u) | (rb & 0x00FF00FFu);
}
IFHIP_HD uint32_t webp_byte_cost(uint32_t v) { return v < 128u ? v : 256u - v; }             // |the residual byte as a signed one|
IFHIP_HD uint32_t webp_residual_cost(uint32_t r) {
    return webp_byte_cost(r & 255u) + webp_byte_cost((r >> 8) & 255u) + webp_byte_cost((r >> 16) & 255u) + webp_byte_cost(r >> 24);
}
// The pixel at (x, y) of a frame, as the predictor sees it: alpha 255 where it is not meaningful, green subtracted.
IFHIP_HD uint32_t webp_source(const uint8_t* frame, uint32_t stride, uint32_t x, uint32_t y, uint32_t alpha_or) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(y) * stride + 4u * x);
    return webp_sub_green(v | alpha_or);
}
// What mode `mode` predicts for (x, y), with the format's boundary rules: 0xFF000000 for the first pixel, L in the rest
// of row 0, T in column 0; the rightmost pixel's TR is the first pixel of its own row.
struct WebpNeighbours { uint32_t L, T, TL, TR; };
IFHIP_HD WebpNeighbours webp_neighbours(const uint8_t* frame, uint32_t stride, uint32_t w, uint32_t x, uint32_t y, uint32_t alpha_or) {
    WebpNeighbours n = {0, 0, 0, 0};
    if (x) n.L = webp_source(frame, stride, x - 1u, y, alpha_or);
    if (y) {
        n.T = webp_source(frame, stride, x, y - 1u, alpha_or);
        if (x) n.TL = webp_source(frame, stride, x - 1u, y - 1u, alpha_or);
        n.TR = x + 1u < w ? webp_source(frame, stride, x + 1u, y - 1u, alpha_or) : webp_source(frame, stride, 0, y, alpha_or);
    }
    return n;
}
IFHIP_HD uint32_t webp_predict_at(uint32_t mode, uint32_t x, uint32_t y, const WebpNeighbours& n) {
    if (y == 0u) return x == 0u ? 0xFF000000u : n.L;
    if (x == 0u) return n.T;
    return webp_predict(mode, n.L, n.T, n.TL, n.TR);
}
IFHIP_HD uint32_t webp_choose_mode(const uint32_t sums[14]) {           // the smallest sum; a tie goes to the lowest number
    uint32_t best = 0, least = sums[0];
    for (uint32_t m = 1; m < 14u; ++m) if (sums[m] < least) { least = sums[m]; best = m; }
    return best;
}

// ---- colour indexing --------------------------------------------------------------------------------------------------------
// A frame of at most 256 distinct colours may open with the colour-indexing transform instead (IFHIP_WEBP_ENC_COLOR_INDEXING):
// the palette is the frame's distinct ARGB dwords (alpha 255 where it is not meaningful) in ascending order, so that it does
// not depend on who found a colour first; the main image holds the indices in green, 8, 4 or 2 of them bundled into one
// pixel where the palette is small.  Nothing follows the transform: no subtract green, no predictor -- the LZ77 parse
// and the codes below work on the packed pixels as they work on residuals, with the packed width as the row distance.
constexpr uint32_t kWebpMaxPalette = 256;
IFHIP_HD uint32_t webp_index_width_bits(uint32_t n_colours) { return n_colours <= 2u ? 3u : n_colours <= 4u ? 2u : n_colours <= 16u ? 1u : 0u; }
IFHIP_HD uint32_t webp_packed_width(uint32_t w, uint32_t width_bits) { return (w + (1u << width_bits) - 1u) >> width_bits; }
// the pixel at (x, y) as the palette holds it
IFHIP_HD uint32_t webp_argb(const uint8_t* frame, uint32_t stride, uint32_t x, uint32_t y, uint32_t alpha_or) {
    return *reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(y) * stride + 4u * x) | alpha_or;
}
// where `c` lies in the ascending palette of n entries (it does): a binary search of at most 8 steps
IFHIP_HD uint32_t webp_palette_index(const uint32_t* pal, uint32_t n, uint32_t c) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pal[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}
// Packed pixel xp of row y: source pixel x of the bundle sits at bit (x mod 2^bits) * (8 >> bits) of green; alpha is 255,
// red and blue are 0, and the padding behind the row's last pixel is index 0.
IFHIP_HD uint32_t webp_bundle(const uint8_t* frame, uint32_t stride, uint32_t w, uint32_t xp, uint32_t y, uint32_t alpha_or, const uint32_t* pal, uint32_t n,
                              uint32_t width_bits) {
    const uint32_t per = 1u << width_bits, depth = 8u >> width_bits;
    uint32_t green = 0;
    for (uint32_t k = 0; k < per; ++k) {
        const uint32_t x = xp * per + k;
        if (x < w) green |= webp_palette_index(pal, n, webp_argb(frame, stride, x, y, alpha_or)) << (k * depth);
    }
    return 0xFF000000u | (green << 8);
}
// entry i of the colour table as the stream codes it: the difference from the entry before, per channel
IFHIP_HD uint32_t webp_palette_delta(const uint32_t* pal, uint32_t i) { return i ? webp_sub_pixels(pal[i], pal[i - 1u]) : pal[0]; }

// ---- LZ77 symbols -----------------------------------------------------------------------------------------------------------
// a length or a distance code v >= 1 as prefix symbol and extra bits
IFHIP_HD void webp_prefix(uint32_t v, uint32_t* sym, uint32_t* ebits, uint32_t* eval) {
    const uint32_t p = v - 1u;
    if (p < 4u) { *sym = p; *ebits = 0; *eval = 0; return; }
    const uint32_t hb = floor_log2(p), e = hb - 1u;
    *sym = 2u * hb + ((p >> e) & 1u); *ebits = e; *eval = p & ((1u << e) - 1u);
}
IFHIP_HD uint32_t webp_prefix_extra_bits(uint32_t sym) { return sym < 4u ? 0u : (sym - 2u) >> 1; }
// A token is 0 (the pixel is inside a match), length | select << 16: select 0 a literal (length 1), 1 a match one row up
// (distance code 1: dx 0, dy 1 -- prefix symbol 0), 2 a match one pixel back (distance code 2: dx 1, dy 0 -- symbol 1).
constexpr uint32_t kWebpSelRow = 1, kWebpSelLeft = 2;
// The match of a position from the runs of equal pixels that start there at the two distances: the longer one, the
// pixel back on a tie; shorter than kWebpMinMatch is a literal.
IFHIP_HD uint32_t webp_choose_match(uint32_t run_left, uint32_t run_row, uint32_t cap) {
    const uint32_t l1 = run_left < cap ? run_left : cap, lw = run_row < cap ? run_row : cap;
    const uint32_t best = l1 >= lw ? l1 : lw;
    if (best < kWebpMinMatch) return 1u;
    return best | ((l1 >= lw ? kWebpSelLeft : kWebpSelRow) << 16);
}
struct WebpTokenSymbols { uint32_t n, s0, s1, s2, s3; };             // the symbols (indices of a group's 1088) a token uses: 4 or 2
IFHIP_HD WebpTokenSymbols webp_count_token(uint32_t tok, uint32_t argb) {
    WebpTokenSymbols t = {4u, kWebpG + ((argb >> 8) & 255u), kWebpR + ((argb >> 16) & 255u), kWebpB + (argb & 255u), kWebpA + (argb >> 24)};
    if ((tok >> 16) != 0u) {
        uint32_t s, eb, ev;
        webp_prefix(tok & 0xFFFFu, &s, &eb, &ev);
        t.n = 2u; t.s0 = kWebpG + 256u + s; t.s1 = kWebpD + ((tok >> 16) == kWebpSelRow ? 0u : 1u);
    }
    return t;
}
// the bits of one token under its group's tables (bit-reversed code | length << 16): green, red, blue, alpha, or the
// length symbol, its extra bits and the distance symbol (which has none here); at most 60
IFHIP_HD uint32_t webp_token_bits(const uint32_t* tab, uint32_t tok, uint32_t argb, uint64_t* value) {
    uint64_t v = 0;
    uint32_t n = 0;
    if ((tok >> 16) == 0u) {
        const uint32_t t[4] = {tab[kWebpG + ((argb >> 8) & 255u)], tab[kWebpR + ((argb >> 16) & 255u)], tab[kWebpB + (argb & 255u)], tab[kWebpA + (argb >> 24)]};
        for (uint32_t k = 0; k < 4u; ++k) { v |= static_cast<uint64_t>(t[k] & 0xFFFFu) << n; n += t[k] >> 16; }
    } else {
        uint32_t s, eb, ev;
        webp_prefix(tok & 0xFFFFu, &s, &eb, &ev);
        uint32_t t = tab[kWebpG + 256u + s];
        v = t & 0xFFFFu; n = t >> 16;
        v |= static_cast<uint64_t>(ev) << n; n += eb;
        t = tab[kWebpD + ((tok >> 16) == kWebpSelRow ? 0u : 1u)];
        v |= static_cast<uint64_t>(t & 0xFFFFu) << n; n += t >> 16;
    }
    *value = v;
    return n;
}

// ---- prefix codes -----------------------------------------------------------------------------------------------------------
struct WebpCodeWork {
    CodeWork P;                     // the prefix-code workspace
    uint8_t len[kCodeMaxSyms];      // the lengths of the code under construction
    uint8_t keep[kCodeMaxSyms];     // the Huffman lengths while the fixed code is sized
};
IFHIP_HD uint32_t webp_cl_order(uint32_t i) {           // 17 18 0 1 2 3 4 5 16 6 7 ... 15
    return i == 0u ? 17u : i == 1u ? 18u : i < 8u ? i - 2u : i == 8u ? 16u : i - 3u;
}
// The flat code a channel falls back to when its Huffman code with its header is larger: 256 symbols of 8 bits (green:
// only in a group without matches; a group with matches falls back as a whole, see webp_flat_group_bits).
IFHIP_HD uint32_t webp_fixed_length(uint32_t s) { return s < 256u ? 8u : 0u; }
// The header of the normal code whose lengths are in W.len[0, n), over ALL n lengths (code_plan_header).  Returns its bits:
// the normal-code bit, the 4-bit count and the "all symbols follow" bit are VP8L's own.
IFHIP_HD uint32_t webp_plan_header(WebpCodeWork& W, uint32_t n) {
    return 1u + 4u + 1u + code_plan_header(W.P, n, [&](uint32_t i) -> uint32_t { return W.len[i]; }, webp_cl_order);
}
IFHIP_HD void webp_write_header(WebpCodeWork& W, uint32_t* hdr, uint32_t* pos) {
    put_bits(hdr, pos, 0u, 1);                                  // a normal code
    put_bits(hdr, pos, W.P.hclen - 4u, 4);
    code_write_cl_lengths(W.P, hdr, pos, webp_cl_order);
    put_bits(hdr, pos, 0u, 1);                                  // all symbols follow
    code_write_rle(W.P, hdr, pos);
}
IFHIP_HD void webp_put_simple_symbol(uint32_t* hdr, uint32_t* pos, uint32_t s) {
    if (s < 2u) { put_bits(hdr, pos, 0u, 1); put_bits(hdr, pos, s, 1); } else { put_bits(hdr, pos, 1u, 1); put_bits(hdr, pos, s, 8); }
}
// One alphabet's code from its counts, by one lane (W.P.sorted filled by code_rank_sort_lane over cnt): the table (bit-
// reversed code | length << 16 per symbol) and the header's bits appended to the zeroed dword stream hdr at *pos.  VP8L
// rejects incomplete codes: no or one used symbol below 256 is the simple one-symbol code (no bits per use), two such the
// simple two-symbol code; everything else is a normal code, Huffman lengths or, where that is smaller with its header (or
// when `force_flat`), the flat code of webp_fixed_length (not for the distance alphabet, nor for green when length symbols
// are in use).  *fixed: the flat code was taken.  Returns the bits of the counted symbols under the code, without extra bits.
IFHIP_HD uint64_t webp_build_code(WebpCodeWork& W, const uint32_t* cnt, uint32_t alphabet, uint32_t* tab, uint32_t* hdr, uint32_t* pos, uint32_t* fixed,
                                  bool force_flat = false) {
    const uint32_t n = webp_alphabet_size(alphabet);
    uint32_t m = 0, s0 = 0, s1 = 0;
    bool with_lengths = false;
    for (uint32_t s = 0; s < n; ++s) {
        tab[s] = 0;
        if (!cnt[s]) continue;
        if (m == 0u) s0 = s; else if (m == 1u) s1 = s;
        ++m;
        if (s >= 256u) with_lengths = true;
    }
    *fixed = 0;
    if (force_flat && alphabet < 4u) {
        for (uint32_t s = 0; s < n; ++s) W.len[s] = static_cast<uint8_t>(webp_fixed_length(s));
        (void)webp_plan_header(W, n);
        webp_write_header(W, hdr, pos);
        code_assign_codes(W.P, W.len, n, tab);
        *fixed = 1;
        uint64_t bits = 0;
        for (uint32_t s = 0; s < n; ++s) bits += static_cast<uint64_t>(cnt[s]) * W.len[s];
        return bits;
    }
    if (m < 2u && s0 < 256u) {
        put_bits(hdr, pos, 1u, 1); put_bits(hdr, pos, 0u, 1);
        webp_put_simple_symbol(hdr, pos, s0);
        return 0;
    }
    if (m == 2u && s1 < 256u) {
        put_bits(hdr, pos, 1u, 1); put_bits(hdr, pos, 1u, 1);
        webp_put_simple_symbol(hdr, pos, s0);
        put_bits(hdr, pos, s1, 8);
        tab[s0] = 0u | (1u << 16); tab[s1] = 1u | (1u << 16);
        return static_cast<uint64_t>(cnt[s0]) + cnt[s1];
    }
    code_build_lengths(W.P, cnt, n, 15, W.len, s0, true);
    uint64_t huff = webp_plan_header(W, n);
    for (uint32_t s = 0; s < n; ++s) huff += static_cast<uint64_t>(cnt[s]) * W.len[s];
    if (alphabet < 4u && !with_lengths) {
        for (uint32_t s = 0; s < n; ++s) { W.keep[s] = W.len[s]; W.len[s] = static_cast<uint8_t>(webp_fixed_length(s)); }
        uint64_t fix = webp_plan_header(W, n);
        for (uint32_t s = 0; s < n; ++s) fix += static_cast<uint64_t>(cnt[s]) * W.len[s];
        if (fix < huff) *fixed = 1;
        else {
            for (uint32_t s = 0; s < n; ++s) W.len[s] = W.keep[s];
            (void)webp_plan_header(W, n);
        }
    }
    webp_write_header(W, hdr, pos);
    code_assign_codes(W.P, W.len, n, tab);
    uint64_t bits = 0;
    for (uint32_t s = 0; s < n; ++s) bits += static_cast<uint64_t>(cnt[s]) * W.len[s];
    return bits;
}
// The headers of a group that is coded as literals under four flat codes (and the one-symbol distance code, 4 bits):
// what a band falls back to when its own codes, headers and matches included, come out larger than 32 bits a pixel.
IFHIP_HD uint32_t webp_flat_group_bits(WebpCodeWork& W) {
    uint32_t bits = 4u;
    for (uint32_t a = 0; a < 4u; ++a) {
        const uint32_t n = webp_alphabet_size(a);
        for (uint32_t s = 0; s < n; ++s) W.len[s] = static_cast<uint8_t>(webp_fixed_length(s));
        bits += webp_plan_header(W, n);
    }
    return bits;
}
// the bits `cnt` (a group's 1088 counts) takes under `tab`, extra bits of the length symbols included
IFHIP_HD uint32_t webp_symbol_cost(const uint32_t* tab, uint32_t s) { return (tab[s] >> 16) + (s >= kWebpG + 256u && s < kWebpR ? webp_prefix_extra_bits(s - 256u) : 0u); }

// ---- the stream's fixed parts -----------------------------------------------------------------------------------------------
// signature, size, alpha_is_used, version 0; subtract green; the predictor transform and its tile bits: 49 bits in front
// of the mode sub-image
IFHIP_HD void webp_put_front(uint32_t* hdr, uint32_t* pos, uint32_t w, uint32_t h, uint32_t alpha) {
    put_bits(hdr, pos, 0x2Fu, 8); put_bits(hdr, pos, w - 1u, 14); put_bits(hdr, pos, h - 1u, 14); put_bits(hdr, pos, alpha, 1); put_bits(hdr, pos, 0u, 3);
    put_bits(hdr, pos, 1u, 1); put_bits(hdr, pos, 2u, 2);
    put_bits(hdr, pos, 1u, 1); put_bits(hdr, pos, 0u, 2); put_bits(hdr, pos, kWebpTileBits - 2u, 3);
    put_bits(hdr, pos, 0u, 1);                                   // the mode sub-image: no colour cache
}
// the indexed stream's front: signature, size (the frame's own width), alpha_is_used, version 0; the colour-indexing
// transform and its table's size: 51 bits in front of the colour table, a size x 1 sub-image without a colour cache
IFHIP_HD void webp_put_front_indexed(uint32_t* hdr, uint32_t* pos, uint32_t w, uint32_t h, uint32_t alpha, uint32_t n_colours) {
    put_bits(hdr, pos, 0x2Fu, 8); put_bits(hdr, pos, w - 1u, 14); put_bits(hdr, pos, h - 1u, 14); put_bits(hdr, pos, alpha, 1); put_bits(hdr, pos, 0u, 3);
    put_bits(hdr, pos, 1u, 1); put_bits(hdr, pos, 3u, 2); put_bits(hdr, pos, n_colours - 1u, 8);
    put_bits(hdr, pos, 0u, 1);
}
// no further transform; the main image: no colour cache, meta prefix codes with their tile bits; the entropy sub-image: no cache
IFHIP_HD void webp_put_middle(uint32_t* hdr, uint32_t* pos) {
    put_bits(hdr, pos, 0u, 1); put_bits(hdr, pos, 0u, 1); put_bits(hdr, pos, 1u, 1); put_bits(hdr, pos, kWebpBandBits - 2u, 3);
    put_bits(hdr, pos, 0u, 1);
}
IFHIP_HD void webp_le32(uint8_t* p, uint32_t v) { p[0] = static_cast<uint8_t>(v); p[1] = static_cast<uint8_t>(v >> 8); p[2] = static_cast<uint8_t>(v >> 16); p[3] = static_cast<uint8_t>(v >> 24); }
// the 20 bytes in front of a payload of payload_bytes; returns the file's size (the payload is padded to an even size)
IFHIP_HD uint32_t webp_write_riff(uint8_t* o, uint32_t payload_bytes) {
    const uint32_t padded = payload_bytes + (payload_bytes & 1u);
    o[0] = 'R'; o[1] = 'I'; o[2] = 'F'; o[3] = 'F'; webp_le32(o + 4, 12u + padded);
    o[8] = 'W'; o[9] = 'E'; o[10] = 'B'; o[11] = 'P'; o[12] = 'V'; o[13] = 'P'; o[14] = '8'; o[15] = 'L'; webp_le32(o + 16, payload_bytes);
    return kWebpRiff + padded;
}

// ---- the largest file of a geometry -----------------------------------------------------------------------------------------
// Exact arithmetic over the choices above (host only: it sizes the fixed codes' headers with the planner itself).
//   front and middle, the sub-images' cache bits included: 50 + 7 bits.
//   a sub-image: its green code is a Huffman code over at most 14 modes (at most 4 bits a tile: no deeper than 13) or
//     over the bands' indices, all equally frequent (at most 8 bits: 256 bands); the other four are one-symbol codes
//     (4 or 11 bits).  Its header is below the largest normal header, 63 + 280 * 14 bits, plus 4 * 11.
//   a group with its pixels: a band whose five codes, their headers and its tokens come out larger than the same band as
//     literals under four flat codes is written as those literals (the codes kernel compares the two exact sizes), so it
//     takes at most webp_flat_group_bits() of headers and 8 + 8 + 8 + 8 = 32 bits a pixel: the flat-code floor.
inline uint64_t webp_max_file_bytes(uint32_t w, uint32_t h) {
    const WebpShape s = webp_shape(w, h);
    WebpCodeWork W;
    const uint64_t sub_hdr = 63u + 280u * 14u + 4u * 11u;
    const uint64_t group = webp_flat_group_bits(W);
    uint64_t bits = 50u + 7u + 2u * sub_hdr;
    bits += 4ull * s.tiles_x * s.tiles_y + 8ull * s.ent_x * s.n_bands;
    bits += group * s.n_bands;
    bits += 32ull * w * h;
    const uint64_t payload = (bits + 7u) >> 3;
    return kWebpRiff + payload + (payload & 1u);
}

}  // namespace ifhip
