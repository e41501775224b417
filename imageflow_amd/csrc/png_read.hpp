// png_read.hpp -- what the host learns from a PNG file before the device sees it (csrc/png_read.cpp): the header facts, the
// palette with tRNS applied, the colour verdict, and where the payloads of all IDAT chunks lie (they are one stream).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ifhip {

struct PngParsed {
    uint32_t w = 0, h = 0, depth = 0, color_type = 0, interlace = 0;
    bool alpha_used = false, uses_palette = false;
    int color_kind = 0;                  // 0: no colour chunks (or gAMA alone); 1: declared sRGB; 2: a colour space that is not sRGB
    bool has_iccp = false;               // the verdict comes from an iCCP profile (else from sRGB / gAMA + cHRM)
    std::vector<uint8_t> icc;            // the iCCP profile, inflated (empty where the chunk did not inflate)
    uint32_t gama = 0, chrm[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // gAMA and cHRM as the chunks hold them (x 100000): white, red, green, blue x, y
    uint32_t palette[256];               // BGRA dwords, tRNS applied; beyond PLTE opaque black
    uint32_t has_trns = 0, key[3] = {0, 0, 0};   // the tRNS key of gray / RGB files, masked to the file's depth
    uint64_t inflated = 0;               // the expected size of the inflated stream
    // the IDAT payloads in file order: pointers into the caller's file (nothing is copied by the walk); idat_len: their sum
    std::vector<std::pair<const uint8_t*, size_t>> idat;
    size_t idat_len = 0;
};
// IFHIP_OK, or IFHIP_INVALID_ARGUMENT with an "ImageMalformed: ..." message.  gather: note where the IDAT payloads lie (else only the facts).
int parse_png(const uint8_t* d, size_t len, PngParsed* out, bool gather);

// The device part of a decode (csrc/png_decode.hip) for files walked already with gather: one walk over the chunks per file,
// whoever needs the facts first.  parsed[i] == nullptr: the file's chunks did not parse (its status word says so).
int png_decode_parsed_device(const PngParsed* const* parsed, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                             const uint32_t* strides, uint32_t* d_status, void* hip_stream);
const char* png_status_text(uint32_t status);

}  // namespace ifhip
