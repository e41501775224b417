// jpeg_parse.hpp -- what the entropy stage (jpeg_entropy.hip; its host half: jpeg_entropy_tables.cpp, jpeg_entropy_plan.cpp,
// jpeg_scan_report.cpp) takes from the host front end of a baseline file (jpeg_parse.cpp): the parsed headers and the scan's
// bytes, un-stuffed and cut at the restart markers.
#pragma once
#include <vector>

#include "jpeg_markers.hpp"

namespace ifhip {
constexpr uint32_t kSubBits = 1024;     // bits per sub-sequence (one lane of the entropy kernels)
constexpr uint32_t kSubWords = kSubBits / 32;
using jpeg::HuffSpec, jpeg::kMaxBlocksInMcu;         // (files with more blocks in an MCU are rejected by the parser)

struct ParsedJpeg : jpeg::FrameHeader, jpeg::Geometry, jpeg::Tables {
    uint8_t td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};    // the scan's table of every component
    size_t scan_begin = 0;
};
// The headers of a file with ONE interleaved sequential Huffman scan, up to that scan's first byte; anything else is refused
// (a progressive file with MethodNotImplemented "... (only baseline Huffman)", which sends the ABI shim to jpeg_read.cpp).
int parse_jpeg(const uint8_t* d, size_t len, ParsedJpeg* out);

struct ScanSegments {                                // the restart segments of an un-stuffed scan
    std::vector<uint32_t> mcu0, mcus, nsub, first_word;      // first MCU, MCUs; packed form: sub-sequences, first word in the block
    std::vector<uint64_t> bits;                              // packed form: bits of data
    uint64_t n_sub = 0;                                      // packed form: sub-sequences in all
    void clear() { mcu0.clear(); mcus.clear(); nsub.clear(); first_word.clear(); bits.clear(); n_sub = 0; }
};
// Un-stuffs the scan (runs between 0xFF bytes are copied whole) and cuts it at restart markers into segments.
// Returns the number of MCUs the segments cover (fewer than the image has: the scan ended early).
uint32_t unstuff_scan(const uint8_t* d, size_t len, const ParsedJpeg& P, std::vector<std::vector<uint8_t>>* seg_bytes, ScanSegments* segs);
// The same walk, straight into the staging buffer the device reads: every restart segment starts on a sub-sequence boundary
// and is zero-padded to the next one (an empty segment still takes one sub-sequence).  No per-segment vectors: a prepared
// file used to cost a 400 KB vector grown by doubling, a copy out of it and a free that glibc answered with madvise() -- 40 %
// of the host CPU of an ABI job (round 5, profiles/r5_abi_jobs_host_cpu_slots32.txt).  `cap` bytes are available at dst
// (packed_scan_bound); returns the MCUs covered.
size_t packed_scan_bound(size_t len, const ParsedJpeg& P);
uint32_t unstuff_scan_packed(const uint8_t* d, size_t len, const ParsedJpeg& P, uint8_t* dst, size_t cap, ScanSegments* segs);

}  // namespace ifhip
