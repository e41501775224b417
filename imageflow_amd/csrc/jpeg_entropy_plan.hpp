// jpeg_entropy_plan.hpp -- the host half of the baseline JPEG entropy stage's handles: what is prepared of one file, and how a
// batch of prepared files is laid out in the one table block the kernels read.  Pure functions over host memory: nothing here
// calls the HIP runtime, so a wrong offset is a finding of tests/jpeg_entropy_plan_check.cpp under the host sanitizers, not a
// fault on a device.  jpeg_entropy.hip allocates, uploads and launches what is decided here.
#pragma once
#include <vector>

#include "jpeg_entropy_tables.hpp"

namespace ifhip {

// One file, prepared on the host: parsed, its decode tables derived, its scan un-stuffed and cut at the restart markers (the
// packed words themselves belong to whoever owns the staging block: ifhip_jpeg_prepared keeps them in pinned memory).
struct PreparedHost {
    ParsedJpeg P;
    uint16_t qt[192];
    ScanSegments seg;                                // per restart segment, and the sub-sequences of them all
    FastTabs ftabs, ptabs, ctabs;
    SearchTab stabs[6];
    uint32_t pool_limit = kPoolEntries;
};
// The two steps of a preparation, in the order prepare_impl runs them around its allocation of the staging block.
// Headers, quantisation tables and the decode tables of `file` (R may be a recycled record).
int prepare_tables(PreparedHost* R, const uint8_t* file, size_t len, uint32_t pool_limit);
// The scan, un-stuffed into `dst` (`cap` >= packed_scan_bound(len, R->P) bytes) as big-endian words, every segment padded to
// 1 024 bits; *n_words of them.  Refuses a scan that ends early (`index_for_messages`: the file's place in its batch).
int prepare_scan(PreparedHost* R, const uint8_t* file, size_t len, uint32_t* dst, size_t cap, uint32_t index_for_messages, size_t* n_words);

// The batch's tables -- segments, sub-sequence -> segment, three look-up tables and six search tables per image, the dispatch
// order of the synchronisation launch -- lie in ONE block that goes to the device in one copy; each region 256-aligned.
struct BatchPlan {
    size_t o_segs = 0, o_sub = 0, o_ftabs = 0, o_ptabs = 0, o_ctabs = 0, o_stabs = 0, o_order = 0, table_bytes = 0;
    size_t n_segs = 0, n_words = 0;                  // n_words: the batch's scan words + lookahead slack behind the last segment
    uint32_t total_subs = 0, n_wg = 0;               // n_wg: workgroups of the synchronisation launch (kOwnSubs sub-sequences each)
    std::vector<uint32_t> first_sub_of;              // [image]
    EntropyGeom g;
    uint32_t uniform_tables = 0;                     // every image carries the same Huffman tables (e.g. the standard ones)
};
// Checks (one batch = one geometry, at most 512 MB of scan data) and sizes.
int plan_batch(const PreparedHost* const* prep, uint32_t n_images, BatchPlan* out);
// Writes the seven regions into `block` (plan.table_bytes bytes; the gaps between regions are not written).
void fill_batch_tables(const PreparedHost* const* prep, uint32_t n_images, const BatchPlan& plan, uint8_t* block);

}  // namespace ifhip
