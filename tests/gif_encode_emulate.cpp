// gif_encode_emulate.cpp -- the passes of csrc/gif_encode.hip on the CPU from the same core header
// (csrc/gif_encode_core.hpp): the key rule per pixel, the palette and the undithered nearest-entry remap through
// tests/png_quantize_emulate.cpp (with which, and tests/png_emulate.cpp, this file is compiled: on keys that are 0 or
// opaque pq_normalize is the identity, so its passes are the device's under kPqKeyGif), every segment by gifenc_segment
// into a slot of the device's size, the scan, the gather dword by dword, the sub-blocks, head and tail.
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/gif_encode_core.hpp"

using namespace ifhip;

extern "C" int pq_emu_quantize(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful, int quality, int min_quality, int speed_in,
                               uint32_t max_colors, int dither, int zlib_level, uint8_t* file, size_t cap, size_t* len, uint32_t* status, uint8_t* palette,
                               uint8_t* indices, uint32_t* info, uint64_t* err);

extern "C" {

// palette: kPqPaletteTap bytes (RGBA in file order, the count); indices: w * h.  *status: 0 or kGifEncFileOverflow (then
// *len = 0).  info[4]: segments, LZW data bytes, minimum code size, entries of alpha below 255.
int gifenc_emu_encode(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful, int repeat, uint32_t delay, int needs_user_input,
                      uint8_t* file, size_t cap, size_t* len, uint32_t* status, uint8_t* palette, uint8_t* indices, uint32_t* info) {
    const uint32_t npix = w * h;
    std::vector<uint32_t> keys(npix);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            uint32_t px; std::memcpy(&px, bgra + static_cast<size_t>(y) * stride + 4u * x, 4);
            keys[static_cast<size_t>(y) * w + x] = pq_key(px, alpha_meaningful != 0, kPqKeyGif);
        }
    size_t qlen = 0;
    uint32_t qstatus = 0, qinfo[4];
    uint64_t qerr[2];
    if (int rc = pq_emu_quantize(reinterpret_cast<const uint8_t*>(keys.data()), w, h, 4u * w, 1, -1, -1, -1, kPqMaxColors, 0, 6, nullptr, 0, &qlen, &qstatus, palette,
                                 indices, qinfo, qerr)) return rc;
    if (qstatus) return 10;
    uint32_t count; std::memcpy(&count, palette + 4u * kPqMaxColors, 4);
    uint32_t ordered[kPqMaxColors];
    for (uint32_t i = 0; i < count; ++i)
        ordered[i] = static_cast<uint32_t>(palette[4u * i + 2u]) | static_cast<uint32_t>(palette[4u * i + 1u]) << 8 | static_cast<uint32_t>(palette[4u * i]) << 16 |
                     static_cast<uint32_t>(palette[4u * i + 3u]) << 24;
    const uint32_t n_trans = qinfo[2], m = gifenc_min_code(count);
    // lzw: a slot per segment, filled with a pattern (the device's are not cleared either)
    const uint32_t n_seg = gifenc_segments(npix), slot_words = gifenc_slot_words();
    std::vector<uint32_t> slots(static_cast<size_t>(n_seg) * slot_words, 0xA5A5A5A5u), off(n_seg + 1u), table(kGifEncHashSlots, 0xA5A5A5A5u);
    GifEncCpuWave wave;
    for (uint32_t s = n_seg; s-- > 0u;) {                          // (any order: segments share nothing)
        const uint32_t first = s * kGifEncSegmentPixels, n = npix - first < kGifEncSegmentPixels ? npix - first : kGifEncSegmentPixels;
        off[s] = gifenc_segment(wave, table.data(), indices + first, n, m, s == 0u, s + 1u == n_seg, slots.data() + static_cast<size_t>(s) * slot_words);
        if ((static_cast<uint64_t>(off[s]) + 31u) / 32u > slot_words - 1u) return 11;
    }
    uint32_t run = 0;
    for (uint32_t s = 0; s < n_seg; ++s) { const uint32_t v = off[s]; off[s] = run; run += v; }
    off[n_seg] = run;
    const uint32_t data = (run + 7u) / 8u, stream_words = static_cast<uint32_t>((gifenc_max_data_bytes(npix) + 3u) / 4u);
    if ((run + 31u) / 32u > stream_words) return 12;
    std::vector<uint32_t> stream(stream_words, 0xA5A5A5A5u);
    for (uint32_t j = (run + 31u) / 32u; j-- > 0u;) stream[j] = gifenc_gather_word(off.data(), n_seg, slots.data(), slot_words, j);
    info[0] = n_seg; info[1] = data; info[2] = m; info[3] = n_trans;
    const uint32_t head = gifenc_head_bytes(count, repeat);
    const uint64_t total = gifenc_file_bytes(head, data);
    *len = 0; *status = 0;
    if (total > cap) { *status = kGifEncFileOverflow; return 0; }
    const uint8_t* src = reinterpret_cast<const uint8_t*>(stream.data());
    for (uint32_t i = 0; i < data; ++i) {
        const uint64_t at = head + gifenc_data_position(i);
        file[at] = src[i];
        if (i % 255u == 0u) file[at - 1u] = static_cast<uint8_t>(data - i < 255u ? data - i : 255u);
    }
    if (gifenc_write_head(file, w, h, ordered, count, n_trans, repeat, delay, needs_user_input ? 1u : 0u) != head) return 13;
    file[total - 2u] = 0; file[total - 1u] = 0x3B;
    *len = static_cast<size_t>(total);
    return 0;
}

uint64_t gifenc_emu_max_file_bytes(uint32_t w, uint32_t h) { return gifenc_max_file_bytes(static_cast<uint64_t>(w) * h); }
uint32_t gifenc_emu_segment_pixels() { return kGifEncSegmentPixels; }

}  // extern "C"
