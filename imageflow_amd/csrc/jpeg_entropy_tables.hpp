// jpeg_entropy_tables.hpp -- what the host and the kernels of the baseline JPEG entropy stage (jpeg_entropy.hip) both read: the
// formats of the Huffman decode tables, the batch's geometry and segment records, and the sizes the host lays a batch out by.
// For the gfx950 kernels AND for a plain host compiler: jpeg_entropy_tables.cpp derives the tables, jpeg_entropy_plan.cpp lays
// out a batch, jpeg_scan_report.cpp walks a scan with them on the host -- none of the three needs HIP.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <exception>
#include <new>

#include "common.hpp"
#include "jpeg_parse.hpp"

// (always_inline spelled out: the host files of the library are built by hipcc too, without the header that defines __forceinline__)
#if defined(__HIPCC__)
#define IFHIP_ENTROPY_HD __host__ __device__ inline __attribute__((always_inline))
#define IFHIP_ENTROPY_UNROLL _Pragma("unroll")
#else
#define IFHIP_ENTROPY_HD inline
#define IFHIP_ENTROPY_UNROLL
#endif

namespace ifhip {

constexpr uint32_t kLutBits = 9;          // (kSubBits, the bits of a sub-sequence: jpeg_parse.hpp, the un-stuffer pads to it)

// Huffman tables in the form every pass reads.  Everything a pass needs from a symbol sits in one 32-bit entry, found
// with ONE lookup by the next kLutBits bits of the stream -- or two for the 2 % of the symbols whose code is longer:
//   bits 0-7   bits to skip (code length + magnitude bits); 0 = the code is longer than the lookup
//   bits 8-15  zigzag advance: DC 1; AC coefficient run + 1; ZRL 16; EOB 64 (reaching 64 ends the block)
//   bits 16-23 code length (32: no such code), bits 24-31 the symbol.
// A first-level entry with skip 0 points into the image's second level (`pool`): bits 16-31 the offset of a sub-table
// indexed by the n bits that follow the first kLutBits (n = longest code with this prefix - kLutBits), bits 8-15 hold
// 32 - n.  jdhuff.c's slow path (the serial "first l with code_l <= maxcode[l]" search) survives only for sub-tables
// that did not fit the pool (first-level entry 0): it reads SearchTab from global memory and no real file gets there.
constexpr uint32_t kLutEntries = 1u << kLutBits;
constexpr uint32_t kPoolEntries = 768;
static_assert(kLutBits >= 8u && kLutBits <= 11u, "first-level lookup: the pair entries assume a code + magnitude of < 32 bits behind it");
static_assert(kPoolEntries >= 128u && kPoolEntries <= 65535u, "a first-level pointer holds the pool offset in 16 bits; one sub-table is up to 128 entries");
struct FastTabs {                                    // one image: [comp][dc, ac] and their shared second level
    uint32_t lut[6][kLutEntries];
    uint32_t pool[kPoolEntries];
};
struct SearchTab {                                   // jdhuff.c jpeg_make_d_derived_tbl, global memory only
    int32_t maxcode[18];                             // largest code of each length (monotone, see derive_search_table)
    int32_t valoff[18];                              // huffval index of the first code of each length minus that code
    uint8_t val[256];
};
IFHIP_ENTROPY_HD uint32_t fast_entry(bool ac, uint32_t len, uint32_t sym) {
    const uint32_t sz = sym & 15u, r = sym >> 4;
    const uint32_t adv = ac ? (sz ? r + 1u : (r == 15u ? 16u : 64u)) : 1u;
    return (sym << 24) | (len << 16) | (adv << 8) | (len + sz);
}
// A bit pattern no code starts with (corrupt data, or a speculative decode off the symbol grid): 16 bits are skipped as
// symbol 0, the length field says 32 (a bit no real length has) and the write pass reports it.
// The synchronisation rounds only track the decoder state, and at q85 a symbol is ~6 bits: their tables (`ptabs`) carry in
// bits 16-31 the skip and zigzag advance of this symbol AND the next one where the next code still lies inside the lookup
// window (both AC, same table; 31 % fewer table reads on 4K q85 files), else a copy of bits 0-15.  The pair applies when
// the first symbol neither ends the block nor the sub-sequence.
IFHIP_ENTROPY_HD uint32_t pair_entry(uint32_t first, uint32_t both) { return (first & 0xffffu) | (both << 16); }
IFHIP_ENTROPY_HD uint32_t invalid_entry(bool ac) { return (32u << 16) | ((ac ? 64u : 1u) << 8) | 16u; }

// Entry of a symbol whose code is longer than the first-level lookup (e = that lookup's entry, skip field 0); S the six
// search tables of the image.  One statement for the kernels and for the host walk of the scan report.
// kPairs: 0 plain entries, 1 pair entries everywhere (ptabs), 2 pair entries in the AC tables only (ctabs)
template <int kPairs = 0, typename Tabs>
IFHIP_ENTROPY_HD uint32_t long_entry(const Tabs* T, const SearchTab* S, uint32_t slot, uint32_t e, uint32_t bits) {
    if (e != 0u) return T->pool[(e >> 16) + ((bits << kLutBits) >> ((e >> 8) & 255u))];
    // jdhuff.c's slow path "l = min{l : code_l <= maxcode[l]}" without its dependent chain: all candidate lengths are
    // compared at once (the host stores a monotone maxcode, see derive_search_table)
    const SearchTab* t = S + slot;
    const bool ac = (slot & 1u) != 0u;
    uint32_t l = kLutBits + 1u;
    IFHIP_ENTROPY_UNROLL
    for (uint32_t k = kLutBits + 1u; k <= 16u; ++k)
        l += static_cast<int32_t>(bits >> (32u - k)) > t->maxcode[k] ? 1u : 0u;
    uint32_t r = invalid_entry(ac);
    if (l <= 16u) {
        const int32_t code = static_cast<int32_t>(bits >> (32u - l));
        const uint32_t sym = t->val[(code + t->valoff[l]) & 255];
        if (ac || sym <= 11u) r = fast_entry(ac, l, sym);
    }
    return (kPairs == 1 || (kPairs == 2 && ac)) ? pair_entry(r, r) : r;
}

struct EntropyGeom {
    uint32_t ncomp, blocks_per_mcu, mcus_w, mcus_h;
    uint32_t bw[3], bh[3];
    uint8_t kcomp[kMaxBlocksInMcu], kdx[kMaxBlocksInMcu], kdy[kMaxBlocksInMcu];   // block k of an MCU: component and offset inside the MCU
    uint32_t kcomp_packed;                           // kcomp as 2-bit fields: the per-symbol lookup is a shift, not a load
    uint32_t hs[3], vs[3];
};
EntropyGeom entropy_geom(const ParsedJpeg& P);

struct Segment {                                     // an independently decodable run: (image, restart interval)
    uint32_t first_sub, n_sub;
    uint32_t bit_end;                                // absolute bit index one past the segment's data
    uint32_t n_blocks;                               // blocks it must produce
    uint32_t image, first_mcu;
};

// ---- what the host sizes a batch by (the kernels: jpeg_entropy.hip) ------------------------------------------------------
constexpr uint32_t kSyncLanes = 1024;               // sub-sequences per workgroup in the synchronisation and count passes
// (No cap below the workgroup's own length on the fixpoint inside a workgroup: the loop ends as soon as nothing is pending, and
// a chain of corrections that is cut short costs a host round trip, more launches and a REPEATED count + write pass.  With a
// cap of 24 that was half of all 64-file decodes of BASELINE cfg4's files -- noise files re-synchronise with p ~ 0.4 per
// sub-sequence, 430 000 sub-sequences: the longest chain of a batch is ~ ln 430 000 / ln (1 / 0.6) = 25 -- round 6,
// profiles/r6_entropy_rounds.txt.)
constexpr uint32_t kInnerRounds = 1024;
// The first kWarmLanes lanes of a workgroup decode the sub-sequences IN FRONT of its own range in round 0 and discard the
// result: the workgroup's first own sub-sequence then starts from a state that has had kWarmLanes sub-sequences to
// synchronise (one fails to with probability ~0.4), so corrections across workgroup boundaries -- a whole extra launch
// of lone walks -- all but disappear.  Later rounds run without them.
constexpr uint32_t kWarmLanes = 16;
constexpr uint32_t kOwnSubs = kSyncLanes - kWarmLanes;                         // sub-sequences a workgroup owns
static_assert(kWarmLanes < kSyncLanes && kSyncLanes % 64u == 0u && kSyncLanes <= 1024u, "whole waves, one workgroup");
constexpr uint32_t kFlagWords = 18;                                             // changed[16], errors, unsettled
constexpr uint32_t kChunkSubs = 512;                                            // sub-sequences per workgroup of the write pass

// ---- the tables of one file (jpeg_entropy_tables.cpp) ---------------------------------------------------------------------
void derive_search_table(const HuffSpec& h, SearchTab* t);
// First level of one table into F->lut[slot], its second level appended to the image's pool (*pool_used entries taken).
void derive_fast_table(const HuffSpec& h, bool ac, FastTabs* F, uint32_t slot, uint32_t* pool_used, uint32_t pool_limit);
// The pair form of an image's tables (see pair_entry): same first-level pointers and pool layout, every entry carries its
// own skip / advance twice unless the next AC code is visible in the rest of the lookup window.
void derive_pair_tables(const FastTabs& F, int ncomp, FastTabs* Pt);
// The count pass's form: pair entries in the AC tables, the DC tables (and their parts of the pool) as they are.
void derive_count_tables(const FastTabs& F, const FastTabs& Pt, FastTabs* Ct);
// The six tables of one image; components that name the same table share its second level.
void derive_image_tables(const ParsedJpeg& P, FastTabs* F, SearchTab* S6, uint32_t pool_limit, uint32_t* pool_used_out = nullptr);

// test hooks: the rarely taken paths (serial code search for sub-tables that overflow the pool; further rounds after an
// unsettled count pass) are forced by shrinking the pool / the iterations per launch
inline uint32_t test_hook_u32(const char* name, uint32_t dflt, uint32_t hi) {
    const char* v = debug_switch(name);
    return v ? std::min<uint32_t>(static_cast<uint32_t>(std::strtoul(v, nullptr, 10)), hi) : dflt;
}
// Nothing C++ crosses the C ABI: the stage's C entry points run their bodies through here (`during`: how the out-of-memory
// message goes on, e.g. " while preparing the scan").
template <typename Body>
int c_entry(const char* during, Body&& body) {
    try { return body(); }
    catch (const std::bad_alloc&) { return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: host memory%s", during); }
    catch (const std::exception& ex) { return fail(IFHIP_INVALID_STATE, "InvalidState: %s", ex.what()); }
}

}  // namespace ifhip
