// png_quantize_core.hpp -- the arithmetic of the device palette quantiser (csrc/png_quantize.hip), written so that it
// compiles for the gfx950 kernels AND for a plain host compiler: tests/png_quantize_emulate.cpp runs the same histogram
// keys, the same palette growth, the same Lloyd sums, the same nearest-entry search and the same error diffusion on the
// CPU -- test infrastructure; the product has one path, the kernels.
//
// What is coded: EncoderPreset::Pngquant (imageflow_types/src/lib.rs:756-761, codecs/pngquant.rs:35-139): at most 256
// RGBA colours, Floyd-Steinberg dithering at full strength, an 8-bit palette PNG as lode.rs:162-195 writes it (filter 0
// on every row, IHDR / PLTE / tRNS / IDAT / IEND and nothing else).  The quantiser is this project's own -- libimagequant
// is not reproduced entry for entry -- and every value in it is an integer, so that no result depends on the
// order in which lanes or atomics arrive.
#pragma once
#include <cmath>
#include <cstdint>

#include "png_encode_core.hpp"

namespace ifhip {

constexpr uint32_t kPqMaxColors = 256;
constexpr uint32_t kPqTableBits = 16, kPqSlots = 1u << kPqTableBits;   // slots of one histogram table
constexpr uint32_t kPqMaxEntries = 1u << 15;                           // more distinct colours than this (fewer at high speed): posterise and re-run
constexpr uint32_t kPqMaxProbe = 2048;                                 // a probe sequence longer than this counts as overflow
constexpr uint32_t kPqLevels = 6;                                      // 0..5 low bits dropped; 5 leaves 8^4 = 4096 colours, which fit
constexpr uint32_t kPqMaxPixels = 1u << 28;                            // keeps sum(weight * distance) inside 64 bits
constexpr uint32_t kPqPaletteTap = kPqMaxColors * 4u + 4u;             // bytes per image of the palette tap: 256 RGBA, then the count
constexpr uint32_t kPqQualityTooLow = 2;                               // the status word, beside kPngFileOverflow
constexpr uint32_t kPqHeadMax = 8u + 25u + (12u + 768u) + (12u + 256u);   // signature, IHDR, a full PLTE and tRNS
constexpr uint32_t kPqFramingMax = kPqHeadMax + 12u + 12u;             // + IDAT's 12 bytes and IEND
constexpr uint64_t kPqUnbounded = (1ull << 36) - 1u;                   // a bound no image reaches (a distance is below 2^35)
constexpr uint64_t kPqDistanceUnit = 6ull * 65025ull * 65025ull;       // the distance of black to white: an MSE of 1 on channels 0..1

// ---- colours -----------------------------------------------------------------------------------------------------------------------
// A key is the frame's BGRA dword after normalize_unused_alpha (alpha 255 where it is not meaningful) with every pixel of
// alpha 0 folded into 00 00 00 00.  A table slot stores key ^ 0x00FFFFFF, so that 0 -- what a memset leaves -- is the one
// value no key has (alpha 0 with a colour) and marks an empty slot.
constexpr uint32_t kPqSlotXor = 0x00FFFFFFu;
IFHIP_HD uint32_t pq_normalize(uint32_t bgra, bool alpha_meaningful) {
    if (!alpha_meaningful) return bgra | 0xFF000000u;
    return (bgra >> 24) ? bgra : 0u;
}
// The key rule of a coder (QuantArgs::key_rule).  kPqKeyPng: pq_normalize.  kPqKeyGif: what GifEncoder::write_frame prepares
// (codecs/gif/mod.rs:385-592): a pixel of meaningful alpha below 0x10 is 00 00 00 00, every other pixel is opaque.
constexpr uint32_t kPqKeyPng = 0, kPqKeyGif = 1;
IFHIP_HD uint32_t pq_key(uint32_t bgra, bool alpha_meaningful, uint32_t rule) {
    if (rule == kPqKeyGif) return alpha_meaningful && (bgra >> 24) < 0x10u ? 0u : bgra | 0xFF000000u;
    return pq_normalize(bgra, alpha_meaningful);
}
IFHIP_HD uint32_t pq_posterize_channel(uint32_t c, uint32_t bits) {    // low bits dropped, the high ones repeated into them (255 stays 255)
    const uint32_t hi = c & ~((1u << bits) - 1u) & 255u;
    uint32_t v = hi;
    for (uint32_t s = 8u - bits; s < 8u; s += 8u - bits) v |= hi >> s;
    return v;
}
IFHIP_HD uint32_t pq_posterize(uint32_t key, uint32_t bits) {
    if (bits == 0u) return key;
    const uint32_t a = pq_posterize_channel(key >> 24, bits);
    if (a == 0u) return 0u;
    return pq_posterize_channel(key & 255u, bits) | (pq_posterize_channel((key >> 8) & 255u, bits) << 8) |
           (pq_posterize_channel((key >> 16) & 255u, bits) << 16) | (a << 24);
}
IFHIP_HD uint32_t pq_hash(uint32_t key) { return (key * 0x9E3779B1u) >> (32u - kPqTableBits); }

// The colour the distance works on: B, G, R multiplied by alpha (0..65025) and 255 * alpha.
struct PqColor { int32_t c[4]; };
IFHIP_HD PqColor pq_premultiply(uint32_t key) {
    const int32_t a = static_cast<int32_t>(key >> 24);
    PqColor p;
    p.c[0] = static_cast<int32_t>(key & 255u) * a; p.c[1] = static_cast<int32_t>((key >> 8) & 255u) * a;
    p.c[2] = static_cast<int32_t>((key >> 16) & 255u) * a; p.c[3] = 255 * a;
    return p;
}
// The squared error of the two colours composited over black plus that over white, summed over the three channels.  Over
// black a pixel shows c*a, over white c*a + 255*(255 - a): the colour of a transparent pixel carries no weight, and two
// keys that differ have a distance above 0.  At most kPqDistanceUnit.
IFHIP_HD uint64_t pq_distance(const PqColor& x, const PqColor& y) {
    const int32_t da = x.c[3] - y.c[3];
    uint64_t d = 0;
    for (int k = 0; k < 3; ++k) {
        const int32_t b = x.c[k] - y.c[k], w = b - da;
        const uint32_t ub = static_cast<uint32_t>(b < 0 ? -b : b), uw = static_cast<uint32_t>(w < 0 ? -w : w);   // <= 65025: the squares fit 32 bits unsigned
        d += static_cast<uint64_t>(ub * ub) + (uw * uw);
    }
    return d;
}
// the nearest of `count` palette colours; the lowest index on a tie
IFHIP_HD uint32_t pq_nearest(const PqColor* pal, uint32_t count, const PqColor& x, uint64_t* dist_out) {
    uint32_t best = 0;
    uint64_t least = ~0ull;
    for (uint32_t i = 0; i < count; ++i) {
        const uint64_t d = pq_distance(pal[i], x);
        if (d < least) { least = d; best = i; }
    }
    *dist_out = least;
    return best;
}

// ---- the histogram --------------------------------------------------------------------------------------------------------------------
// One pixel into an open-addressed table (slots: key ^ kPqSlotXor, counts) by compare-and-swap; *entries counts the
// claimed slots.  false: the table has more than max_entries colours or a probe ran too long -- the pass is void.
// cas(p, expected, value) returns what *p held; add(p, v) returns what *p held.
template <typename Cas, typename Add>
IFHIP_HD bool pq_insert(uint32_t* slots, uint32_t* counts, uint32_t* entries, uint32_t max_entries, uint32_t key, Cas cas, Add add) {
    const uint32_t stored = key ^ kPqSlotXor;
    uint32_t s = pq_hash(key);
    for (uint32_t probe = 0; probe < kPqMaxProbe; ++probe, s = (s + 1u) & (kPqSlots - 1u)) {
        uint32_t held = slots[s];
        if (held == 0u) {
            held = cas(slots + s, 0u, stored);
            if (held == 0u) {
                if (add(entries, 1u) >= max_entries) return false;
                held = stored;
            }
        }
        if (held == stored) { add(counts + s, 1u); return true; }
    }
    return false;
}

// speed 1..10 -> Lloyd iterations over the histogram, and the number of distinct colours above which the histogram is
// posterised (a frame of at most 256 colours is never posterised, at any speed)
IFHIP_HD uint32_t pq_speed_iterations(uint32_t speed) { return speed >= 9u ? 0u : speed >= 4u ? 9u - speed : speed == 3u ? 6u : speed == 2u ? 8u : 10u; }
IFHIP_HD uint32_t pq_speed_max_entries(uint32_t speed) { return kPqMaxEntries >> (speed <= 4u ? 0u : speed <= 6u ? 1u : speed <= 8u ? 2u : 3u); }

// ---- palette growth and Lloyd refinement ----------------------------------------------------------------------------------------------
// Growth: the first entry is the heaviest histogram colour; every further one is the histogram colour with the largest
// weight * distance to its nearest entry so far (the lowest key on a tie).  Growth ends at the first size whose summed
// error is within the target bound, or at max_colors.  A lane's share of one growth pass over entries [lane, n) by nlanes:
struct PqGrow { uint64_t err, score; uint32_t key; };
IFHIP_HD void pq_grow_better(PqGrow* g, uint64_t score, uint32_t key) {
    if (score > g->score || (score == g->score && key < g->key)) { g->score = score; g->key = key; }
}
IFHIP_HD void pq_grow_lane(const uint32_t* ekey, const uint32_t* ew, uint64_t* edmin, uint32_t n, uint32_t lane, uint32_t nlanes, uint32_t newest_key,
                           bool first, PqGrow* g) {
    const PqColor nc = pq_premultiply(newest_key);
    for (uint32_t i = lane; i < n; i += nlanes) {
        uint64_t d = pq_distance(pq_premultiply(ekey[i]), nc);
        if (!first && edmin[i] < d) d = edmin[i];
        edmin[i] = d;
        const uint64_t sc = d * ew[i];
        g->err += sc;
        pq_grow_better(g, sc, ekey[i]);
    }
}
// One Lloyd centroid from its integer sums {sum w*a*B, sum w*a*G, sum w*a*R, sum w*a, sum w}: alpha is the weighted mean,
// the colour the mean weighted by alpha too (a single colour comes back exactly).  An empty cluster keeps its entry.
IFHIP_HD uint32_t pq_centroid(const uint64_t s[5], uint32_t old_key) {
    if (s[4] == 0u) return old_key;
    const uint32_t a = static_cast<uint32_t>((s[3] + s[4] / 2u) / s[4]);
    if (a == 0u || s[3] == 0u) return 0u;
    const uint32_t b = static_cast<uint32_t>((s[0] + s[3] / 2u) / s[3]), g = static_cast<uint32_t>((s[1] + s[3] / 2u) / s[3]),
                   r = static_cast<uint32_t>((s[2] + s[3] / 2u) / s[3]);
    return b | (g << 8) | (r << 16) | (a << 24);
}
// The file's order: entries with alpha below 255 first (tRNS then holds exactly those), each group in growth order.  One lane.
IFHIP_HD uint32_t pq_order_palette(const uint32_t* keys, uint32_t count, uint32_t* out) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < count; ++i) if ((keys[i] >> 24) != 255u) out[n++] = keys[i];
    const uint32_t n_trans = n;
    for (uint32_t i = 0; i < count; ++i) if ((keys[i] >> 24) == 255u) out[n++] = keys[i];
    return n_trans;
}

// ---- the remap: Floyd-Steinberg, left to right on every row ----------------------------------------------------------------------------
// Errors are sixteenths of a channel step, B G R A.  `in`: what reaches this pixel from the left and from the row above.
// The target is the source plus the error, clamped to the channel's range and rounded to a byte for the search; the error
// handed on is target - chosen entry.  A target of alpha 0 is the transparent key, and where source or entry is fully
// transparent no colour error is handed on (there is no colour to be wrong about).
IFHIP_HD uint32_t pq_remap_pixel(const PqColor* pal, const uint32_t* pal_keys, uint32_t count, uint32_t key, const int32_t in[4], bool dither, int32_t err[4]) {
    int32_t t[4];
    uint32_t target = 0;
    for (int k = 0; k < 4; ++k) {
        int32_t v = static_cast<int32_t>((key >> (8 * k)) & 255u) * 16 + (dither ? in[k] : 0);
        v = v < 0 ? 0 : v > 4080 ? 4080 : v;
        t[k] = v;
        target |= static_cast<uint32_t>((v + 8) >> 4) << (8 * k);
    }
    if ((target >> 24) == 0u) target = 0u;
    uint64_t d;
    const uint32_t idx = pq_nearest(pal, count, pq_premultiply(target), &d);
    const uint32_t chosen = pal_keys[idx];
    const bool no_colour = (key >> 24) == 0u || (chosen >> 24) == 0u || (target >> 24) == 0u;
    for (int k = 0; k < 4; ++k) err[k] = dither && !(no_colour && k < 3) ? t[k] - static_cast<int32_t>((chosen >> (8 * k)) & 255u) * 16 : 0;
    return idx;
}
// 7/16 to the right, 3/16 below left, 1/16 below right, the rest (5/16 and what the shifts dropped) below
IFHIP_HD void pq_split_error(int32_t e, int32_t* right, int32_t* below_left, int32_t* below, int32_t* below_right) {
    *right = (e * 7) >> 4; *below_left = (e * 3) >> 4; *below_right = e >> 4;
    *below = e - *right - *below_left - *below_right;
}

// ---- quality -------------------------------------------------------------------------------------------------------------------------
// quality 0..100 -> the largest mean distance per pixel that still counts as reaching it, in pq_distance's unit.  100 asks
// for no error at all, 0 for nothing.  In between: the mapping libimagequant is remembered to use, on this quantiser's own
// scale (no gamma) -- the scale is NOT pinned to libimagequant.  Host only.
// (pq_quality_bound, at the end of this file)

// ---- the file's head --------------------------------------------------------------------------------------------------------------------
// signature, IHDR (8 bit, colour type 3, no interlace), PLTE, and tRNS when n_trans > 0 (lode.rs:162-195: lodepng writes
// no gAMA / sRGB / cHRM).  keys: the palette in file order.  Returns the bytes written.  One lane.
IFHIP_HD uint32_t pq_head_bytes(uint32_t count, uint32_t n_trans) { return 8u + 25u + 12u + 3u * count + (n_trans ? 12u + n_trans : 0u); }
IFHIP_HD uint32_t pq_write_head(uint8_t* o, uint32_t w, uint32_t h, const uint32_t* keys, uint32_t count, uint32_t n_trans) {
    o[0] = 0x89; o[1] = 'P'; o[2] = 'N'; o[3] = 'G'; o[4] = 13; o[5] = 10; o[6] = 26; o[7] = 10;
    uint8_t* c = o + 8;
    png_be32(c + 8, w); png_be32(c + 12, h);
    c[16] = 8; c[17] = 3; c[18] = 0; c[19] = 0; c[20] = 0;
    c += png_close_chunk(c, 0x49484452u, 13);                       // IHDR
    for (uint32_t i = 0; i < count; ++i) {
        c[8u + 3u * i] = static_cast<uint8_t>(keys[i] >> 16); c[9u + 3u * i] = static_cast<uint8_t>(keys[i] >> 8); c[10u + 3u * i] = static_cast<uint8_t>(keys[i]);
    }
    c += png_close_chunk(c, 0x504C5445u, 3u * count);               // PLTE
    if (n_trans) {
        for (uint32_t i = 0; i < n_trans; ++i) c[8u + i] = static_cast<uint8_t>(keys[i] >> 24);
        c += png_close_chunk(c, 0x74524E53u, n_trans);              // tRNS
    }
    return static_cast<uint32_t>(c - o);
}

}  // namespace ifhip

namespace ifhip {
inline uint64_t pq_quality_bound(uint32_t quality) {
    if (quality >= 100u) return 0u;
    if (quality == 0u) return kPqUnbounded;
    const double q = static_cast<double>(quality);
    const double extra = 0.016 / (0.001 + q) - 0.001;
    const double mse = (extra > 0.0 ? extra : 0.0) + 2.5 / std::pow(210.0 + q, 1.2) * (100.1 - q) / 100.0;
    const double bound = mse * static_cast<double>(kPqDistanceUnit);
    return bound >= static_cast<double>(kPqUnbounded) ? kPqUnbounded : static_cast<uint64_t>(bound);
}
}  // namespace ifhip
