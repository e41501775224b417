// jpeg_progressive_read.hpp -- the host front end of the device progressive JPEG decoder (csrc/jpeg_progressive_read.cpp; no
// HIP): a file walked once into a *prepared* file -- frame facts, latched quantisation tables, the scan list with its
// dependency levels, the streams -- and n prepared files laid out as the one block a batch uploads.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "jpeg_progressive_core.hpp"

namespace ifhip {

struct ProgPrepared {
    uint32_t width = 0, height = 0, ncomp = 0;
    uint8_t hs[3] = {0, 0, 0}, vs[3] = {0, 0, 0};
    uint32_t bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};
    uint16_t qt[3][64];                              // as latched at each component's first scan
    std::vector<ProgScanRec> scans;                  // file 0, tables counted from 0
    std::vector<uint32_t> scan_level;
    std::vector<ProgStreamRec> streams;              // scans and words counted from 0, in file order
    std::vector<ProgTable> tables;
    std::vector<uint32_t> words;                     // big-endian, every stream from a word of its own
    uint32_t n_levels = 0;
};

// IFHIP_OK, or IFHIP_METHOD_NOT_IMPLEMENTED for every file the device path does not take (the host reader's verdict stands).
int prog_prepare(const uint8_t* d, size_t len, ProgPrepared* out);

// The block of a batch: [files][scans][streams, by level][tables][words + slack], each part from a 16-byte boundary.  `blob`
// is what the host writes; the device reads nothing behind it.
struct ProgLayout {
    std::vector<uint8_t> blob;
    size_t files_off = 0, scans_off = 0, streams_off = 0, tables_off = 0, words_off = 0;
    uint64_t n_words = 0;
    uint32_t n_files = 0, n_streams = 0;
    std::vector<uint32_t> level_first;               // n_levels + 1
    uint64_t max_plane_blocks = 0;
    ProgArgs args(uint8_t* block, uint32_t* status) const;
};
constexpr uint32_t kProgSlackWords = 8;
// coef[3 * i + c], plane_bytes[3 * i + c]: plane c of file i.  false: a plane is missing, misaligned or too small.
bool prog_layout_batch(const ProgPrepared* const* files, uint32_t n, void* const* coef, const size_t* plane_bytes, ProgLayout* L);

}  // namespace ifhip
