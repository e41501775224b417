// webp_decode_core.hpp -- the one statement of the VP8L format for the device WebP decoder (csrc/webp_decode.hip), written
// so that it compiles for the gfx950 kernels AND for a plain host compiler: the host prepare (csrc/webp_read.cpp) and
// the CPU emulation of the tests (tests/webp_decode_emulate.cpp) run the same bit reader, the same token loop and the
// same inverse transforms (the emulation writes the predictor's skewed schedule a second time, after the kernel's: the
// kernel's own loop is covered by the GPU tests); libwebp (through Pillow) is the yardstick for every pixel.
//
// What is decoded: what WebPDecode hands the reference for a lossless file (imageflow_core/src/codecs/webp.rs:20-248):
// BGRA bytes, alpha as coded.  Every rule with a bit in it lives here -- the prefix codes with libwebp's refusals
// (VP8LBuildHuffmanTable: an over-subscribed or incomplete set unless one symbol is used, which then reads no bits; no
// symbol at all; ReadHuffmanCodeLengths: a repeat beyond the alphabet, max_symbol beyond it), the token loop (literals,
// length / distance prefixes, the 120-entry distance map, the colour cache, meta prefix groups), and the four inverse
// transforms with their edge rules.
//
// Who runs what: the HOST reads the header, the transform list with its sub-images, the entropy image and every group's
// five codes (a few percent of a file's bits), and turns the codes into compact decode records.  The DEVICE runs the main
// image's token loop from the bit where it starts, one wave per file, and the inverse transforms.  The token loop is
// wave-UNIFORM code, like png_inflate: every lane runs it identically (on the CPU: once); the wave-wide parts go through
// an executor X:
//   X.lanes(f)     f(lane) for lanes 0..63 with a barrier in front and behind (CPU: a loop)
//   X.one(f)       f() on one lane, no barrier
//   X.sync()       a barrier (CPU: nothing)
//   X.fence()      this wave's earlier stores to memory are visible to its later loads (CPU: nothing)
//   X.max64(p, v)  *p = max(*p, v) on a 64-bit LDS word, atomically among the lanes
#pragma once
#include <cstdint>

#include <vector>

#include "prefix_code_core.hpp"      // IFHIP_HD; the encoders' code construction there has no decode half to share

namespace ifhip {

enum : uint32_t {
    kWebpDecOk = 0,
    kWebpDecTruncated = 1,       // a bit was used that the stream does not have
    kWebpDecCodeLengths = 2,     // a set of code lengths libwebp refuses, a repeat or max_symbol beyond the alphabet
    kWebpDecBadCode = 3,         // bits that are no code of the set (a complete set has none: the guard of the canonical walk)
    kWebpDecDistance = 4,        // a copy whose source lies before the image's first pixel
    kWebpDecCopyEnd = 5,         // a copy that runs past the image's last pixel
    kWebpDecCacheSymbol = 6,     // a colour-cache symbol beyond the cache (without a cache the alphabet has none: a guard)
    kWebpDecTransform = 7,       // a transform twice, colour cache bits outside 1..11
    kWebpDecTooLittle = 8,       // the payload ends inside the five header bytes (the library's container walk refuses such a chunk first)
    kWebpDecContainer = 9,       // the RIFF container did not parse (batch only)
};

constexpr uint32_t kWebpLanes = 64;
constexpr uint32_t kWebpIn = 4096;               // staged input bytes held in LDS at a time
constexpr uint32_t kWebpCacheMax = 2048;         // colour cache entries at 11 bits
constexpr uint32_t kWebpGreenMax = 256 + 24 + kWebpCacheMax;
// one group's record in 16-bit words: a head of 8 (where its five codes start), and per code 15 counts (lengths 1..15),
// the number of used symbols, and the used symbols in canonical order
constexpr uint32_t kWebpCodeHead = 16, kWebpGroupHead = 8;
constexpr uint32_t kWebpGroupWords = kWebpGroupHead + 5u * kWebpCodeHead + kWebpGreenMax + 3u * 256u + 40u;
static_assert(kWebpGroupWords % 2u == 0, "a group's record is staged in dwords");

typedef uint32_t WebpQuad __attribute__((vector_size(16)));
typedef uint32_t __attribute__((may_alias)) WebpWord;           // a dword of memory that is declared as quads or as 16-bit words

struct WebpLds {
    WebpQuad in[kWebpIn / 16u + 1u];             // the input window (one quad to spare)
    uint64_t cache[kWebpCacheMax];               // colour cache: (position + 1) << 32 | ARGB -- the later insert wins by its position
    alignas(4) uint16_t tab[kWebpGroupWords];    // the staged group's record (staged in dwords)
};

// ---- the bit reader: bounded by the staged length -----------------------------------------------------------------------------------
// src: 16-byte aligned, readable in whole quads up to `len` rounded up to 16 (the host pads with zeros); nothing beyond is
// touched: quads past the end enter the LDS window as zeros, and using a bit the stream does not have is kWebpDecTruncated.
struct WebpBits {
    const uint8_t* src;
    uint32_t len, base, pos, cnt;        // base: stream offset of the LDS window; pos: the next byte to enter buf (a multiple of 4); cnt: valid bits in buf
    uint64_t buf;
};
template <typename X>
IFHIP_HD void webp_bits_window(X& x, WebpLds& S, WebpBits& b, bool force) {
    if (!force && b.pos + 32u <= b.base + kWebpIn) return;
    b.base = b.pos & ~15u;
    const uint32_t padded = (b.len + 15u) & ~15u, base = b.base;
    const WebpQuad* src = reinterpret_cast<const WebpQuad*>(b.src);
    x.lanes([&](uint32_t lane) {
        for (uint32_t q = lane; q < kWebpIn / 16u + 1u; q += kWebpLanes) {
            const uint32_t off = base + q * 16u;
            WebpQuad v = {0u, 0u, 0u, 0u};
            if (off < padded) v = src[off >> 4];
            S.in[q] = v;
        }
    });
}
IFHIP_HD void webp_bits_need32(const WebpLds& S, WebpBits& b) {           // at least 32 valid (or zero-filled) bits in buf
    if (b.cnt >= 32u) return;
    const uint32_t v = reinterpret_cast<const WebpWord*>(S.in)[(b.pos - b.base) >> 2];
    b.buf |= static_cast<uint64_t>(v) << b.cnt;
    b.cnt += 32u; b.pos += 4u;
}
IFHIP_HD uint32_t webp_bits_take(WebpBits& b, uint32_t n) {               // n < 32, after webp_bits_need32
    const uint32_t v = static_cast<uint32_t>(b.buf) & ((1u << n) - 1u);
    b.buf >>= n; b.cnt -= n;
    return v;
}
IFHIP_HD uint64_t webp_bits_position(const WebpBits& b) { return static_cast<uint64_t>(b.pos) * 8u - b.cnt; }
IFHIP_HD bool webp_bits_overrun(const WebpBits& b) { return webp_bits_position(b) > static_cast<uint64_t>(b.len) * 8u; }
template <typename X>
IFHIP_HD void webp_bits_start(X& x, WebpLds& S, WebpBits& b, const uint8_t* src, uint32_t len, uint64_t bit) {
    b.src = src; b.len = len; b.buf = 0; b.cnt = 0; b.base = 0;
    b.pos = static_cast<uint32_t>(bit >> 3) & ~3u;
    const uint32_t skip = static_cast<uint32_t>(bit - static_cast<uint64_t>(b.pos) * 8u);     // 0..31
    webp_bits_window(x, S, b, true);
    webp_bits_need32(S, b);
    webp_bits_take(b, skip);
}
// one read of n < 32 bits with the window and the refill in front (the host's header reads; the token loop refills itself)
template <typename X>
IFHIP_HD uint32_t webp_bits_read(X& x, WebpLds& S, WebpBits& b, uint32_t n) {
    webp_bits_window(x, S, b, false);
    webp_bits_need32(S, b);
    return webp_bits_take(b, n);
}

// ---- one symbol of a code record ------------------------------------------------------------------------------------------------------
// t: 15 counts, the number of used symbols, the symbols.  A code with one used symbol reads no bits, whatever its length.
IFHIP_HD int webp_read_symbol(const uint16_t* t, uint32_t bits, uint32_t* len) {
    if (t[15] == 1u) { *len = 0; return t[kWebpCodeHead]; }
    uint32_t code = 0, first = 0, index = 0;                               // the canonical walk, a bit at a time
    for (uint32_t l = 1; l < 16u; ++l) {
        code |= (bits >> (l - 1u)) & 1u;
        const uint32_t cnt = t[l - 1u];
        if (code < first + cnt) { *len = l; return t[kWebpCodeHead + index + (code - first)]; }
        index += cnt; first = (first + cnt) << 1; code <<= 1;
    }
    *len = 0;
    return -1;
}
// the value of a length or distance prefix symbol (extra bits: at most 10 for a length, 18 for a distance)
IFHIP_HD uint32_t webp_prefix_extra_bits(uint32_t sym) { return sym < 4u ? 0u : (sym - 2u) >> 1; }
IFHIP_HD uint32_t webp_prefix_value(uint32_t sym, uint32_t extra) {
    if (sym < 4u) return sym + 1u;
    return ((2u + (sym & 1u)) << ((sym - 2u) >> 1)) + extra + 1u;
}
// distance codes 1..120: dy << 4 | (8 - dx), the pixel dx to the left and dy rows up
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__
#endif
static const uint8_t kWebpDistMap[120] = {
    0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
    0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
    0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
    0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
    0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
    0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
IFHIP_HD uint32_t webp_distance(uint32_t code, uint32_t xsize) {         // code >= 1
    if (code > 120u) return code - 120u;
    const uint32_t m = kWebpDistMap[code - 1u];
    const int64_t d = static_cast<int64_t>(m >> 4) * xsize + (8 - static_cast<int>(m & 15u));
    return d >= 1 ? static_cast<uint32_t>(d) : 1u;
}
IFHIP_HD uint32_t webp_cache_slot(uint32_t argb, uint32_t cache_bits) { return (0x1E35A7BDu * argb) >> (32u - cache_bits); }

// ---- the token loop over an entropy-coded image ---------------------------------------------------------------------------------------
struct WebpImage {
    uint32_t xsize, ysize;
    uint32_t cache_bits;                 // 0: no colour cache
    uint32_t prefix_bits, ent_x;         // the entropy image's tile bits and width (entropy != nullptr)
    const uint32_t* entropy;             // the group of every tile; nullptr: one group
    const uint32_t* group_off;           // where group g's record starts in `tables`, in dwords
    const uint32_t* tables;
};
// xsize * ysize ARGB values into out[], from bit `start` of the stream; the stores are bounded by xsize * ysize, the reads
// by the staged length.  Returns the status; *end_bit: the bit behind the last token (nullptr: not wanted).
template <typename X>
IFHIP_HD uint32_t webp_pixels(X& x, WebpLds& S, const uint8_t* src, uint32_t len, uint64_t start, const WebpImage& im, uint32_t* out, uint64_t* end_bit) {
    WebpBits b;
    webp_bits_start(x, S, b, src, len, start);
    const uint32_t n = im.xsize * im.ysize, mask = im.entropy ? (1u << im.prefix_bits) - 1u : 0xFFFFFFFFu;
    const uint32_t cache_size = im.cache_bits ? 1u << im.cache_bits : 0u;
    x.lanes([&](uint32_t lane) { for (uint32_t k = lane; k < cache_size; k += kWebpLanes) S.cache[k] = 0; });
    const uint16_t* tab = S.tab;
    WebpWord* tab_words = reinterpret_cast<WebpWord*>(S.tab);
    uint32_t status = kWebpDecOk, i = 0, col = 0, row = 0, staged = 0xFFFFFFFFu;
    bool look = true;
    while (i < n) {
        if (look) {                                                        // the group of the pixel this symbol is read for
            const uint32_t g = im.entropy ? im.entropy[static_cast<size_t>(row >> im.prefix_bits) * im.ent_x + (col >> im.prefix_bits)] : 0u;
            if (g != staged) {
                const uint32_t from = im.group_off[g], words = im.group_off[g + 1u] - from;     // (the host keeps words <= kWebpGroupWords / 2)
                const uint32_t* rec = im.tables + from;
                x.lanes([&](uint32_t lane) { for (uint32_t k = lane; k < words; k += kWebpLanes) tab_words[k] = rec[k]; });
                staged = g;
            }
            look = false;
        }
        webp_bits_window(x, S, b, false);
        webp_bits_need32(S, b);
        uint32_t l;
        const int s = webp_read_symbol(tab + tab[0], static_cast<uint32_t>(b.buf), &l);
        if (s < 0) { status = kWebpDecBadCode; break; }
        webp_bits_take(b, l);
        if (s < 256) {
            uint32_t v = static_cast<uint32_t>(s) << 8;
            int c;
            webp_bits_need32(S, b);
            if ((c = webp_read_symbol(tab + tab[1], static_cast<uint32_t>(b.buf), &l)) < 0) { status = kWebpDecBadCode; break; }
            webp_bits_take(b, l); v |= static_cast<uint32_t>(c) << 16;
            webp_bits_need32(S, b);
            if ((c = webp_read_symbol(tab + tab[2], static_cast<uint32_t>(b.buf), &l)) < 0) { status = kWebpDecBadCode; break; }
            webp_bits_take(b, l); v |= static_cast<uint32_t>(c);
            webp_bits_need32(S, b);
            if ((c = webp_read_symbol(tab + tab[3], static_cast<uint32_t>(b.buf), &l)) < 0) { status = kWebpDecBadCode; break; }
            webp_bits_take(b, l); v |= static_cast<uint32_t>(c) << 24;
            if (webp_bits_overrun(b)) { status = kWebpDecTruncated; break; }
            const uint32_t at = i;
            x.one([&] {
                out[at] = v;
                if (cache_size) x.max64(&S.cache[webp_cache_slot(v, im.cache_bits)], static_cast<uint64_t>(at + 1u) << 32 | v);
            });
            i += 1u; col += 1u;
            if (col == im.xsize) { col = 0; row += 1u; look = true; }
            else if ((col & mask) == 0u) look = true;
        } else if (s < 280) {
            webp_bits_need32(S, b);
            const uint32_t ls = static_cast<uint32_t>(s) - 256u;
            const uint32_t length = webp_prefix_value(ls, webp_bits_take(b, webp_prefix_extra_bits(ls)));
            webp_bits_need32(S, b);
            const int ds = webp_read_symbol(tab + tab[4], static_cast<uint32_t>(b.buf), &l);
            if (ds < 0) { status = kWebpDecBadCode; break; }
            webp_bits_take(b, l);
            webp_bits_need32(S, b);
            const uint32_t dist = webp_distance(webp_prefix_value(static_cast<uint32_t>(ds), webp_bits_take(b, webp_prefix_extra_bits(static_cast<uint32_t>(ds)))), im.xsize);
            if (webp_bits_overrun(b)) { status = kWebpDecTruncated; break; }
            if (dist > i) { status = kWebpDecDistance; break; }
            if (length > n - i) { status = kWebpDecCopyEnd; break; }
            // out[i + j] = out[i - dist + (j mod dist)]: every source lies below i, so it is the output of an EARLIER token;
            // the fence stands between those tokens' stores and this token's loads
            x.fence();
            const uint32_t at = i;
            for (uint32_t j0 = 0; j0 < length; j0 += kWebpLanes)
                x.lanes([&](uint32_t lane) {
                    const uint32_t j = j0 + lane;
                    if (j >= length) return;
                    const uint32_t v = out[at - dist + (dist >= length ? j : j % dist)];
                    out[at + j] = v;
                    if (cache_size) x.max64(&S.cache[webp_cache_slot(v, im.cache_bits)], static_cast<uint64_t>(at + j + 1u) << 32 | v);
                });
            i += length; col += length;
            if (col >= im.xsize) { row += col / im.xsize; col %= im.xsize; }
            look = im.entropy != nullptr;
        } else {
            const uint32_t k = static_cast<uint32_t>(s) - 280u;
            if (k >= cache_size) { status = kWebpDecCacheSymbol; break; }
            if (webp_bits_overrun(b)) { status = kWebpDecTruncated; break; }
            x.sync();
            const uint32_t v = static_cast<uint32_t>(S.cache[k]);          // (its own slot holds it already: nothing to insert)
            const uint32_t at = i;
            x.one([&] { out[at] = v; });
            i += 1u; col += 1u;
            if (col == im.xsize) { col = 0; row += 1u; look = true; }
            else if ((col & mask) == 0u) look = true;
        }
    }
    if (end_bit) *end_bit = webp_bits_position(b);
    return status;
}

// ---- the inverse transforms -------------------------------------------------------------------------------------------------------------
IFHIP_HD uint32_t webp_add(uint32_t a, uint32_t b) { return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu); }
IFHIP_HD uint32_t webp_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
IFHIP_HD int webp_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
IFHIP_HD int webp_abs(int v) { return v < 0 ? -v : v; }
// modes 0..13 of the specification; 14 and 15 predict opaque black, as libwebp's table does (a mode is the low 4 bits of the tile's green)
IFHIP_HD uint32_t webp_predict(uint32_t mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (mode) {
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
    case 11: {
        int d = 0;                                                         // sum |L - TL| - sum |T - TL| per channel: above zero takes L
        for (uint32_t s = 0; s < 32u; s += 8u) {
            const int l = (L >> s) & 255, t = (T >> s) & 255, tl = (TL >> s) & 255;
            d += webp_abs(l - tl) - webp_abs(t - tl);
        }
        return d > 0 ? L : T;
    }
    case 12: {
        uint32_t v = 0;
        for (uint32_t s = 0; s < 32u; s += 8u) v |= static_cast<uint32_t>(webp_clamp255(static_cast<int>((L >> s) & 255u) + static_cast<int>((T >> s) & 255u) - static_cast<int>((TL >> s) & 255u))) << s;
        return v;
    }
    case 13: {
        const uint32_t a = webp_avg2(L, T);
        uint32_t v = 0;
        for (uint32_t s = 0; s < 32u; s += 8u) {
            const int av = (a >> s) & 255, tl = (TL >> s) & 255;
            v |= static_cast<uint32_t>(webp_clamp255(av + (av - tl) / 2)) << s;       // (the division truncates toward zero)
        }
        return v;
    }
    default: return 0xFF000000u;
    }
}
// the prediction of pixel (x, y) with the edge rules: the first pixel adds opaque black, the first row L, the first column T
IFHIP_HD uint32_t webp_predict_at(uint32_t mode, uint32_t x, uint32_t y, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    if (y == 0u) return x == 0u ? 0xFF000000u : L;
    if (x == 0u) return T;
    return webp_predict(mode, L, T, TL, TR);
}
IFHIP_HD uint32_t webp_tile_mode(uint32_t tile_argb) { return (tile_argb >> 8) & 15u; }
IFHIP_HD int webp_color_delta(uint32_t multiplier, uint32_t color) { return (static_cast<int>(static_cast<int8_t>(multiplier)) * static_cast<int>(static_cast<int8_t>(color))) >> 5; }
IFHIP_HD uint32_t webp_cross_color(uint32_t v, uint32_t e) {              // e: red_to_blue << 16 | green_to_blue << 8 | green_to_red
    const uint32_t green = (v >> 8) & 255u;
    const uint32_t red = ((v >> 16) + static_cast<uint32_t>(webp_color_delta(e, green))) & 255u;
    const uint32_t blue = (v + static_cast<uint32_t>(webp_color_delta(e >> 8, green)) + static_cast<uint32_t>(webp_color_delta(e >> 16, red))) & 255u;
    return (v & 0xFF00FF00u) | red << 16 | blue;
}
IFHIP_HD uint32_t webp_add_green(uint32_t v) { const uint32_t g = (v >> 8) & 255u; return (v & 0xFF00FF00u) | (((v & 0x00FF00FFu) + (g << 16 | g)) & 0x00FF00FFu); }
IFHIP_HD uint32_t webp_index_bits(uint32_t palette_size) { return palette_size <= 2u ? 3u : palette_size <= 4u ? 2u : palette_size <= 16u ? 1u : 0u; }
IFHIP_HD uint32_t webp_subsample(uint32_t size, uint32_t bits) { return (size + (1u << bits) - 1u) >> bits; }
// pixel x of a row of bundled indices -> its palette entry; an index beyond the palette is transparent black
IFHIP_HD uint32_t webp_index_pixel(const uint32_t* packed_row, uint32_t x, uint32_t bits, const uint32_t* palette, uint32_t palette_size) {
    const uint32_t step = 8u >> bits, g = (packed_row[x >> bits] >> 8) & 255u;
    const uint32_t idx = bits ? (g >> ((x & ((1u << bits) - 1u)) * step)) & ((1u << step) - 1u) : g;
    return idx < palette_size ? palette[idx] : 0u;
}

// ---- the host's part: header, transforms, entropy image, the groups' codes (plain host code) -------------------------------------------
struct WebpHostExec {
    template <typename F> void lanes(F f) { for (uint32_t lane = 0; lane < kWebpLanes; ++lane) f(lane); }
    template <typename F> void one(F f) { f(); }
    void sync() {}
    void fence() {}
    void max64(uint64_t* p, uint64_t v) { if (v > *p) *p = v; }
};
struct WebpTransform {
    uint32_t kind = 0, bits = 0;         // 0 predictor, 1 cross-colour, 2 subtract green, 3 colour indexing
    uint32_t xsize = 0;                  // the width of the image this transform gives back
    std::vector<uint32_t> data;          // the tiles' ARGB (0, 1), the palette with its deltas summed (3)
};
struct WebpPrepared {
    uint32_t w = 0, h = 0, alpha = 0;
    uint32_t n_transforms = 0;
    WebpTransform t[4];                  // in file order; the decoder applies them last to first
    uint32_t xsize = 0;                  // the coded main image's width (reduced by colour indexing)
    uint32_t cache_bits = 0, prefix_bits = 0, ent_x = 0;
    std::vector<uint32_t> entropy;       // empty: one group
    std::vector<uint32_t> group_off;     // groups + 1
    std::vector<uint32_t> tables;
    uint64_t start_bit = 0;              // where the main image's tokens start
    std::vector<WebpQuad> payload;       // the library's copy of the stream: 16-byte aligned, zero-padded (csrc/webp_read.cpp)
};

class WebpHeadReader {
  public:
    // payload: 16-byte aligned, zero-padded to a multiple of 16
    WebpHeadReader(const uint8_t* payload, uint32_t len) : S_(new WebpLds) { webp_bits_start(x_, *S_, b_, payload, len, 0); }
    ~WebpHeadReader() { delete S_; }
    WebpHeadReader(const WebpHeadReader&) = delete;

    uint32_t prepare(WebpPrepared* P) {
        if (b_.len < 5u) return kWebpDecTooLittle;
        if (bits(8) != 0x2Fu) return kWebpDecContainer;
        P->w = bits(14) + 1u; P->h = bits(14) + 1u; P->alpha = bits(1);
        if (bits(3) != 0u) return kWebpDecContainer;
        return prepare_body(P);
    }
    // a stream without signature and size field (the VP8L-coded plane of an ALPH chunk): the image's size is the caller's
    uint32_t prepare_headless(uint32_t w, uint32_t h, WebpPrepared* P) {
        P->w = w; P->h = h; P->alpha = 0;
        return prepare_body(P);
    }
    uint32_t prepare_body(WebpPrepared* P) {
        uint32_t xsize = P->w, seen = 0;
        P->n_transforms = 0;
        while (bits(1)) {
            const uint32_t kind = bits(2);
            if (seen & (1u << kind)) return kWebpDecTransform;
            seen |= 1u << kind;
            WebpTransform& T = P->t[P->n_transforms++];
            T.kind = kind; T.bits = 0; T.xsize = xsize; T.data.clear();
            if (kind < 2u) {
                T.bits = bits(3) + 2u;
                if (uint32_t st = sub_image(webp_subsample(xsize, T.bits), webp_subsample(P->h, T.bits), &T.data)) return st;
            } else if (kind == 3u) {
                const uint32_t size = bits(8) + 1u;
                if (uint32_t st = sub_image(size, 1u, &T.data)) return st;
                for (uint32_t i = 1; i < size; ++i) T.data[i] = webp_add(T.data[i], T.data[i - 1u]);
                T.bits = webp_index_bits(size);
                xsize = webp_subsample(xsize, T.bits);
            }
            if (webp_bits_overrun(b_)) return kWebpDecTruncated;
        }
        P->xsize = xsize;
        if (uint32_t st = cache_bits(&P->cache_bits)) return st;
        P->entropy.clear(); P->prefix_bits = 0; P->ent_x = 0;
        uint32_t groups = 1;
        if (bits(1)) {
            P->prefix_bits = bits(3) + 2u;
            P->ent_x = webp_subsample(xsize, P->prefix_bits);
            if (uint32_t st = sub_image(P->ent_x, webp_subsample(P->h, P->prefix_bits), &P->entropy)) return st;
            for (uint32_t& v : P->entropy) { v = (v >> 8) & 0xFFFFu; if (v + 1u > groups) groups = v + 1u; }
        }
        if (uint32_t st = read_groups(groups, P->cache_bits, &P->group_off, &P->tables)) return st;
        if (webp_bits_overrun(b_)) return kWebpDecTruncated;
        P->start_bit = webp_bits_position(b_);
        return kWebpDecOk;
    }
    // the main image as the device decodes it (the emulation of the tests)
    uint32_t main_image(const WebpPrepared& P, std::vector<uint32_t>* out, uint64_t* end_bit) {
        out->assign(static_cast<size_t>(P.xsize) * P.h, 0u);
        const WebpImage im = {P.xsize, P.h, P.cache_bits, P.prefix_bits, P.ent_x, P.entropy.empty() ? nullptr : P.entropy.data(), P.group_off.data(), P.tables.data()};
        return webp_pixels(x_, *S_, b_.src, b_.len, P.start_bit, im, out->data(), end_bit);
    }

  private:
    uint32_t bits(uint32_t n) { return webp_bits_read(x_, *S_, b_, n); }
    uint32_t cache_bits(uint32_t* out) {
        *out = 0;
        if (bits(1)) { *out = bits(4); if (*out < 1u || *out > 11u) return kWebpDecTransform; }
        return kWebpDecOk;
    }
    // a code's lengths -> its record behind `rec`; libwebp's refusals (VP8LBuildHuffmanTable)
    static uint32_t append_code(const std::vector<uint8_t>& len, std::vector<uint16_t>* rec) {
        uint32_t count[16] = {0}, used = 0;
        for (uint8_t l : len) { count[l] += 1u; used += l ? 1u : 0u; }
        if (used == 0u) return kWebpDecCodeLengths;
        if (used > 1u) {
            uint32_t kraft = 0;
            for (uint32_t l = 1; l < 16u; ++l) kraft += count[l] << (15u - l);
            if (kraft != 1u << 15) return kWebpDecCodeLengths;
        }
        for (uint32_t l = 1; l < 16u; ++l) rec->push_back(static_cast<uint16_t>(count[l]));
        rec->push_back(static_cast<uint16_t>(used));
        for (uint32_t l = 1; l < 16u; ++l)
            for (size_t s = 0; s < len.size(); ++s) if (len[s] == l) rec->push_back(static_cast<uint16_t>(s));
        return kWebpDecOk;
    }
    uint32_t read_code(uint32_t alphabet, std::vector<uint16_t>* rec) {
        static const uint8_t order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
        std::vector<uint8_t> len(alphabet, 0);
        if (bits(1)) {                                                     // a simple code: one or two symbols
            // (a symbol at or beyond the alphabet -- the distance alphabet has 40 -- is left uncounted, as libwebp builds its
            // table from the alphabet's lengths only: alone it is "no symbol", beside a legal one it leaves a one-symbol code)
            const uint32_t two = bits(1);
            const uint32_t first = bits(bits(1) ? 8u : 1u);
            if (first < alphabet) len[first] = 1;
            if (two) { const uint32_t second = bits(8); if (second < alphabet) len[second] = 1; }
        } else {
            std::vector<uint8_t> cl(19, 0);
            const uint32_t n = 4u + bits(4);
            for (uint32_t i = 0; i < n; ++i) cl[order[i]] = static_cast<uint8_t>(bits(3));
            std::vector<uint16_t> cl_rec;
            if (webp_bits_overrun(b_)) return kWebpDecTruncated;
            if (uint32_t st = append_code(cl, &cl_rec)) return st;
            uint32_t max_symbol = alphabet;
            if (bits(1)) {
                const uint32_t nbits = 2u + 2u * bits(3);
                max_symbol = 2u + bits(nbits);
                if (webp_bits_overrun(b_)) return kWebpDecTruncated;
                if (max_symbol > alphabet) return kWebpDecCodeLengths;
            }
            uint32_t prev = 8, s = 0;
            while (s < alphabet && max_symbol) {
                max_symbol -= 1u;
                webp_bits_window(x_, *S_, b_, false);
                webp_bits_need32(*S_, b_);
                uint32_t l;
                const int c = webp_read_symbol(cl_rec.data(), static_cast<uint32_t>(b_.buf), &l);
                if (c < 0) return kWebpDecBadCode;
                webp_bits_take(b_, l);
                if (c < 16) {
                    len[s++] = static_cast<uint8_t>(c);
                    if (c) prev = static_cast<uint32_t>(c);
                } else {
                    const uint32_t rep = c == 16 ? 3u + bits(2) : c == 17 ? 3u + bits(3) : 11u + bits(7);
                    if (webp_bits_overrun(b_)) return kWebpDecTruncated;
                    if (s + rep > alphabet) return kWebpDecCodeLengths;
                    for (uint32_t k = 0; k < rep; ++k) len[s++] = static_cast<uint8_t>(c == 16 ? prev : 0u);
                }
                if (webp_bits_overrun(b_)) return kWebpDecTruncated;
            }
        }
        if (webp_bits_overrun(b_)) return kWebpDecTruncated;
        return append_code(len, rec);
    }
    uint32_t read_groups(uint32_t groups, uint32_t cache_bits, std::vector<uint32_t>* off, std::vector<uint32_t>* tables) {
        const uint32_t alphabet[5] = {256u + 24u + (cache_bits ? 1u << cache_bits : 0u), 256u, 256u, 256u, 40u};
        off->clear(); tables->clear();
        std::vector<uint16_t> rec;
        for (uint32_t g = 0; g < groups; ++g) {
            rec.assign(kWebpGroupHead, 0);
            for (uint32_t k = 0; k < 5u; ++k) {
                rec[k] = static_cast<uint16_t>(rec.size());
                if (uint32_t st = read_code(alphabet[k], &rec)) return st;
            }
            if (rec.size() & 1u) rec.push_back(0);
            off->push_back(static_cast<uint32_t>(tables->size()));
            for (size_t k = 0; k < rec.size(); k += 2u) tables->push_back(static_cast<uint32_t>(rec[k]) | static_cast<uint32_t>(rec[k + 1u]) << 16);
        }
        off->push_back(static_cast<uint32_t>(tables->size()));
        return kWebpDecOk;
    }
    // a sub-image (no meta codes): its own cache bits, one group, its tokens -- the same loop as the main image's
    uint32_t sub_image(uint32_t xsize, uint32_t ysize, std::vector<uint32_t>* out) {
        uint32_t cb = 0;
        if (uint32_t st = cache_bits(&cb)) return st;
        std::vector<uint32_t> off, tables;
        if (uint32_t st = read_groups(1u, cb, &off, &tables)) return st;
        out->assign(static_cast<size_t>(xsize) * ysize, 0u);
        const WebpImage im = {xsize, ysize, cb, 0u, 0u, nullptr, off.data(), tables.data()};
        uint64_t end = 0;
        const uint32_t st = webp_pixels(x_, *S_, b_.src, b_.len, webp_bits_position(b_), im, out->data(), &end);
        if (st) return st;
        webp_bits_start(x_, *S_, b_, b_.src, b_.len, end);
        return kWebpDecOk;
    }

    WebpHostExec x_;
    WebpLds* S_;
    WebpBits b_;
};

}  // namespace ifhip
