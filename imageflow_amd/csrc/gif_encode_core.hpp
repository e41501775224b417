// gif_encode_core.hpp -- the one statement of the device GIF coder (csrc/gif_encode.hip), written so that it compiles for
// the gfx950 kernels AND for a plain host compiler: the CPU emulation of the tests (tests/gif_encode_emulate.cpp) runs the
// same segment coder, the same gather of the segments' bits, the same sub-block positions and the same head.
//
// What is coded: EncoderPreset::Gif (imageflow_core/src/codecs/gif/mod.rs:385-592): one frame, the logical screen of its
// size without a global colour table, a local colour table of at most 256 entries, no dithering.  The palette is the
// integer quantiser's of png_quantize_core.hpp under the key rule kPqKeyGif -- NOT the gif crate's NeuQuant.
//
// The LZW stream is cut by clear codes at fixed pixel positions: between two clear codes a stream depends on nothing in
// front of it (the fact the decoder's segments rest on, gif_decode_core.hpp), so a segment of kGifEncSegmentPixels indices
// is coded by one wave on its own.  Segment s writes, from bit 0 of its private slot: the stream's leading clear code
// (s = 0 only), its codes -- greedy longest match, a clear code and a fresh table whenever the table is full -- and the
// clear code in front of the next segment, or the end code.  A code's width is the one gif_width_at reads it with.
//
// The wave goes through an executor:
//   W.fetch(p, base, n)   lane L takes p[base + L] (0 beyond n)           (CPU: 64 bytes into an array)
//   W.byte(j)             what lane j took, the same in every lane
//   W.uniform(v)          v of the first lane: marks a value that is the same in every lane
//   W.clear(table)        kGifEncHashSlots zero words, every lane sees them afterwards
//   W.one(f)              f() on one lane
#pragma once
#include <cstdint>

#include "gif_decode_core.hpp"       // gif_width_at
#include "png_quantize_core.hpp"

namespace ifhip {

#ifndef IFHIP_GIF_ENC_SEGMENT_PIXELS
#define IFHIP_GIF_ENC_SEGMENT_PIXELS 16384
#endif
constexpr uint32_t kGifEncSegmentPixels = IFHIP_GIF_ENC_SEGMENT_PIXELS;   // (bytes against latency)
constexpr uint32_t kGifEncHashBits = 13, kGifEncHashSlots = 1u << kGifEncHashBits;   // at most 4090 entries: half full
constexpr uint32_t kGifEncMinRunCodes = 4094u - 256u;    // codes between two clear codes of a full table, at the least (m = 8)
constexpr uint32_t kGifEncFileOverflow = 1;              // the status word
constexpr uint32_t kGifEncHeadMax = 6u + 7u + 19u + 8u + 10u + 768u + 1u;   // signature .. minimum code size, with NETSCAPE2.0 and 256 entries
constexpr uint32_t kGifEncThreads = 256;

// ---- sizes: arithmetic alone ---------------------------------------------------------------------------------------------------------
IFHIP_HD uint32_t gifenc_segments(uint32_t n_pix) { return (n_pix + kGifEncSegmentPixels - 1u) / kGifEncSegmentPixels; }
// the codes `pixels` indices of one segment can become: each a code, a clear per full table, the leading clear, the terminator
IFHIP_HD uint64_t gifenc_max_codes(uint64_t pixels) { return pixels + pixels / kGifEncMinRunCodes + 2u; }
// dwords of a segment's slot: every code 12 bits wide, and one dword more, so that the gather may read two at any bit
IFHIP_HD uint32_t gifenc_slot_words() { return static_cast<uint32_t>((gifenc_max_codes(kGifEncSegmentPixels) * 12u + 31u) / 32u) + 1u; }
// bytes of a frame's LZW data at the most (below 2^29 for 2^28 pixels: bit positions fit 32 bits)
IFHIP_HD uint64_t gifenc_max_data_bytes(uint64_t n_pix) {
    const uint64_t segs = (n_pix + kGifEncSegmentPixels - 1u) / kGifEncSegmentPixels;
    return ((n_pix + n_pix / kGifEncMinRunCodes + 2u * segs) * 12u + 7u) / 8u;
}
IFHIP_HD uint64_t gifenc_max_file_bytes(uint64_t n_pix) {
    const uint64_t d = gifenc_max_data_bytes(n_pix);
    return kGifEncHeadMax + d + (d + 254u) / 255u + 2u;          // the sub-blocks' length bytes, the terminator and ';'
}

// ---- the palette's place in the file ------------------------------------------------------------------------------------------------
// the table holds 2^bits entries, 2 at the least; the minimum code size is max(2, bits)
IFHIP_HD uint32_t gifenc_palette_bits(uint32_t count) {
    uint32_t b = 1;
    while ((1u << b) < count) ++b;
    return b;
}
IFHIP_HD uint32_t gifenc_min_code(uint32_t count) { const uint32_t b = gifenc_palette_bits(count); return b < 2u ? 2u : b; }

// ---- one segment by one wave -----------------------------------------------------------------------------------------------------------
// table: kGifEncHashSlots words, an entry is (prefix << 8 | byte) << 12 | code and 0 is empty (no code is 0).  Returns the
// segment's length in bits; the slot's dwords up to that length are written.
IFHIP_HD uint32_t gifenc_hash(uint32_t key) { return (key * 0x9E3779B1u) >> (32u - kGifEncHashBits); }

template <typename W>
IFHIP_HD uint32_t gifenc_segment(W& x, uint32_t* table, const uint8_t* idx, uint32_t n, uint32_t m, bool first, bool last, uint32_t* slot) {
    const uint32_t clear = 1u << m, run_codes = 4094u - clear;   // the code that would make entry 4095 is followed by a clear
    uint64_t acc = 0;
    uint32_t nacc = 0, nw = 0;
    uint32_t k = 0, width = m + 1u;                              // codes since the last clear, and gif_width_at(m, k)
    auto put = [&](uint32_t code) {
        acc |= static_cast<uint64_t>(code) << nacc;
        nacc += width;
        if (nacc >= 32u) {
            const uint32_t word = static_cast<uint32_t>(acc);
            x.one([&] { slot[nw] = word; });
            ++nw; acc >>= 32; nacc -= 32u;
        }
    };
    auto counted = [&] { ++k; while (width < 12u && k >= (1u << width) - clear - 1u) ++width; };
    if (first) put(clear);
    x.clear(table);
    uint32_t prefix = 0, next = clear + 2u;
    for (uint32_t i = 0; i < n; ++i) {
        if ((i & 63u) == 0u) x.fetch(idx, i, n);
        const uint32_t b = x.byte(i & 63u);
        if (i == 0u) { prefix = b; continue; }
        const uint32_t key = prefix << 8 | b;
        uint32_t h = gifenc_hash(key), e = x.uniform(table[h]);
        while (e != 0u && (e >> 12) != key) { h = (h + 1u) & (kGifEncHashSlots - 1u); e = x.uniform(table[h]); }
        if (e != 0u) { prefix = e & 0xFFFu; continue; }
        put(prefix);
        counted();
        if (k == run_codes) {
            put(clear);
            x.clear(table);
            k = 0; width = m + 1u; next = clear + 2u;
        } else {
            table[h] = key << 12 | next;                         // (every lane: the same word)
            ++next;
        }
        prefix = b;
    }
    put(prefix);
    counted();
    put(last ? clear + 1u : clear);
    const uint32_t bits = nw * 32u + nacc;
    if (nacc) { const uint32_t word = static_cast<uint32_t>(acc); x.one([&] { slot[nw] = word; }); }
    return bits;
}

// ---- the gather: dword j of the frame's stream, by the lane that owns it ------------------------------------------------------------------
// off[0 .. n_seg]: the segments' exclusive bit offsets and the total.  slots: n_seg slots of slot_words dwords.
IFHIP_HD uint32_t gifenc_gather_word(const uint32_t* off, uint32_t n_seg, const uint32_t* slots, uint32_t slot_words, uint32_t j) {
    const uint64_t bit = static_cast<uint64_t>(j) * 32u;
    uint32_t lo = 0, hi = n_seg;                                 // the last segment that starts at or before `bit`
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (off[mid] <= bit) lo = mid; else hi = mid; }
    uint32_t out = 0, filled = 0;
    for (uint32_t s = lo; s < n_seg && filled < 32u; ++s) {
        const uint64_t at = bit + filled;
        if (at >= off[s + 1u]) continue;
        const uint32_t local = static_cast<uint32_t>(at - off[s]), avail = off[s + 1u] - static_cast<uint32_t>(at);
        const uint32_t take = avail < 32u - filled ? avail : 32u - filled;
        const uint32_t* p = slots + static_cast<size_t>(s) * slot_words + (local >> 5);
        const uint64_t two = static_cast<uint64_t>(p[0]) | static_cast<uint64_t>(p[1]) << 32;
        const uint32_t v = static_cast<uint32_t>(two >> (local & 31u)) & (take == 32u ? 0xFFFFFFFFu : (1u << take) - 1u);
        out |= v << filled;
        filled += take;
    }
    return out;
}

// ---- the file ----------------------------------------------------------------------------------------------------------------------------
// repeat < 0: no NETSCAPE2.0 block.  The head ends with the minimum code size; data byte i of D lies at
// head + gifenc_data_position(i), a sub-block's length byte in front of every 255; then the terminator and ';'.
IFHIP_HD uint32_t gifenc_head_bytes(uint32_t count, int32_t repeat) { return 6u + 7u + (repeat >= 0 ? 19u : 0u) + 8u + 10u + 3u * (1u << gifenc_palette_bits(count)) + 1u; }
IFHIP_HD uint64_t gifenc_data_position(uint64_t i) { return i + i / 255u + 1u; }
IFHIP_HD uint64_t gifenc_file_bytes(uint32_t head, uint64_t data_bytes) { return head + data_bytes + (data_bytes + 254u) / 255u + 2u; }
// The file's own part of the head: signature, logical screen, NETSCAPE2.0.  One lane.  Returns the bytes written.
IFHIP_HD uint32_t gifenc_screen_bytes(int32_t repeat) { return 6u + 7u + (repeat >= 0 ? 19u : 0u); }
IFHIP_HD uint32_t gifenc_write_screen(uint8_t* o, uint32_t w, uint32_t h, int32_t repeat) {
    uint8_t* c = o;
    const uint8_t sig[6] = {'G', 'I', 'F', '8', '9', 'a'};
    for (int i = 0; i < 6; ++i) *c++ = sig[i];
    *c++ = static_cast<uint8_t>(w); *c++ = static_cast<uint8_t>(w >> 8); *c++ = static_cast<uint8_t>(h); *c++ = static_cast<uint8_t>(h >> 8);
    *c++ = 0x70; *c++ = 0; *c++ = 0;                              // no global table (8 bits of colour resolution), background 0, no aspect
    if (repeat >= 0) {
        const uint8_t app[14] = {0x21, 0xFF, 11, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0'};
        for (int i = 0; i < 14; ++i) *c++ = app[i];
        *c++ = 3; *c++ = 1; *c++ = static_cast<uint8_t>(repeat); *c++ = static_cast<uint8_t>(repeat >> 8); *c++ = 0;
    }
    return static_cast<uint32_t>(c - o);
}
// A frame's part: graphic control extension, image descriptor, local table, minimum code size.  keys: the palette in file
// order (the transparent entry, if any, is entry 0).  One lane.  Returns the bytes written.
IFHIP_HD uint32_t gifenc_frame_head_bytes(uint32_t count) { return 8u + 10u + 3u * (1u << gifenc_palette_bits(count)) + 1u; }
constexpr uint32_t kGifEncFrameHeadMax = 8u + 10u + 768u + 1u;
IFHIP_HD uint32_t gifenc_write_frame_head(uint8_t* o, uint32_t w, uint32_t h, const uint32_t* keys, uint32_t count, uint32_t n_trans, uint32_t delay, uint32_t user_input,
                                          uint32_t dispose) {
    uint8_t* c = o;
    *c++ = 0x21; *c++ = 0xF9; *c++ = 4;
    *c++ = static_cast<uint8_t>(dispose << 2 | (user_input ? 2u : 0u) | (n_trans ? 1u : 0u));
    *c++ = static_cast<uint8_t>(delay); *c++ = static_cast<uint8_t>(delay >> 8); *c++ = 0; *c++ = 0;
    const uint32_t bits = gifenc_palette_bits(count);
    *c++ = 0x2C; *c++ = 0; *c++ = 0; *c++ = 0; *c++ = 0;
    *c++ = static_cast<uint8_t>(w); *c++ = static_cast<uint8_t>(w >> 8); *c++ = static_cast<uint8_t>(h); *c++ = static_cast<uint8_t>(h >> 8);
    *c++ = static_cast<uint8_t>(0x80u | (bits - 1u));
    for (uint32_t i = 0; i < (1u << bits); ++i) {
        const uint32_t key = i < count ? keys[i] : 0u;           // padded with black
        *c++ = static_cast<uint8_t>(key >> 16); *c++ = static_cast<uint8_t>(key >> 8); *c++ = static_cast<uint8_t>(key);
    }
    *c++ = static_cast<uint8_t>(gifenc_min_code(count));
    return static_cast<uint32_t>(c - o);
}
// the head of a one-frame file: disposal 1 (keep), as the gif crate's Frame::default
IFHIP_HD uint32_t gifenc_write_head(uint8_t* o, uint32_t w, uint32_t h, const uint32_t* keys, uint32_t count, uint32_t n_trans, int32_t repeat, uint32_t delay,
                                    uint32_t user_input) {
    const uint32_t at = gifenc_write_screen(o, w, h, repeat);
    return at + gifenc_write_frame_head(o + at, w, h, keys, count, n_trans, delay, user_input, 1u);
}

// ---- the animation: N frames in one file -------------------------------------------------------------------------------------
// The file is the screen part, then per frame a BODY -- the frame's head, its data in sub-blocks, the terminator -- then ';'.
// Frames of meaningful alpha carry disposal 2 in a file of more than one frame: with the reference's Keep a transparent
// pixel of frame k would show frame k - 1 through it.  A one-frame file is the one-frame coder's, byte for byte.
IFHIP_HD uint32_t gifenc_animation_dispose(uint32_t n_frames, bool alpha_meaningful) { return n_frames > 1u && alpha_meaningful ? 2u : 1u; }
IFHIP_HD uint32_t gifenc_body_bytes(uint32_t count, uint32_t data_bytes) { return gifenc_frame_head_bytes(count) + data_bytes + (data_bytes + 254u) / 255u + 1u; }
IFHIP_HD uint64_t gifenc_max_body_bytes(uint64_t n_pix) { const uint64_t d = gifenc_max_data_bytes(n_pix); return kGifEncFrameHeadMax + d + (d + 254u) / 255u + 1u; }
// Byte q of a body: head: the frame's head (head_bytes of it), data: its LZW stream of data_bytes.
IFHIP_HD uint32_t gifenc_body_byte(const uint8_t* head, uint32_t head_bytes, const uint8_t* data, uint32_t data_bytes, uint32_t q) {
    if (q < head_bytes) return head[q];
    const uint32_t s = q - head_bytes, blk = s >> 8, r = s & 255u;         // a sub-block: its length byte and 255 bytes
    if (s >= data_bytes + (data_bytes + 254u) / 255u) return 0u;           // the terminator
    if (r == 0u) return data_bytes - 255u * blk < 255u ? data_bytes - 255u * blk : 255u;
    return data[255u * blk + r - 1u];
}
// What one chunk of frames adds to the file.  off[0 .. n]: the byte offsets of the chunk's bodies in the FILE and its end;
// [lo, hi) is what the chunk owns: with the screen part in front where it is the first, with ';' behind where it is the last.
struct GifAnimChunk {
    const uint32_t* off;             // [n + 1]
    const uint8_t* heads;            // the screen part (32 bytes), then a frame head every kGifEncFrameHeadPitch bytes
    const uint8_t* streams;          // a frame's LZW data every stream_pitch bytes
    const uint32_t* data_bytes;      // [n]
    const uint32_t* head_bytes;      // [n]
    uint32_t n, stream_pitch, lo, hi, first, last;
};
constexpr uint32_t kGifEncScreenPitch = 32u, kGifEncFrameHeadPitch = 800u;
IFHIP_HD uint32_t gifenc_animation_byte(const GifAnimChunk& c, uint32_t p, uint32_t* frame) {
    if (p < c.off[0]) return c.heads[p];                                    // (the first chunk: the screen part)
    if (p >= c.off[c.n]) return 0x3Bu;                                      // (the last chunk)
    uint32_t i = *frame;
    while (p >= c.off[i + 1u]) ++i;
    *frame = i;
    return gifenc_body_byte(c.heads + kGifEncScreenPitch + static_cast<size_t>(i) * kGifEncFrameHeadPitch, c.head_bytes[i],
                            c.streams + static_cast<size_t>(i) * c.stream_pitch, c.data_bytes[i], p - c.off[i]);
}
// The rule of the gather, stated over the FILE's dwords: dword j is assembled, all four bytes, by the one lane that owns
// it, so two frames that share a dword never both write it.  A chunk owns the dwords that END inside [lo, hi): j in
// [lo / 4, hi / 4).  The bytes of dword lo / 4 in front of lo belong to the chunk before: it left them in `carry_in` (the
// dword's low bytes).  The bytes behind the chunk's last whole dword go to the next chunk the same way, or -- the last
// chunk -- are stored one by one.
IFHIP_HD uint32_t gifenc_animation_first_frame(const GifAnimChunk& c, uint32_t p) {
    uint32_t lo = 0, hi = c.n;                                   // the last body that starts at or before p
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (c.off[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}
IFHIP_HD uint32_t gifenc_animation_word(const GifAnimChunk& c, uint32_t j, uint32_t carry_in) {
    uint32_t word = 0, frame = gifenc_animation_first_frame(c, 4u * j < c.lo ? c.lo : 4u * j);
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t p = 4u * j + b;
        const uint32_t v = p < c.lo ? (carry_in >> (8u * b)) & 0xFFu : p < c.hi ? gifenc_animation_byte(c, p, &frame) : 0u;
        word |= v << (8u * b);
    }
    return word;
}

#ifndef __HIPCC__
struct GifEncCpuWave {
    uint8_t held[64];
    void fetch(const uint8_t* p, uint32_t base, uint32_t n) { for (uint32_t l = 0; l < 64u; ++l) held[l] = base + l < n ? p[base + l] : 0u; }
    uint32_t byte(uint32_t j) const { return held[j]; }
    uint32_t uniform(uint32_t v) const { return v; }
    void clear(uint32_t* table) { for (uint32_t i = 0; i < kGifEncHashSlots; ++i) table[i] = 0u; }
    template <typename F> void one(F f) { f(); }
};
#endif

}  // namespace ifhip
