// jpeg_markers.hpp -- the JPEG marker syntax (ITU-T T.81 Annex B, as libjpeg's jdmarker.c reads it), once: the walk from segment
// to segment, the readers of the segments a decoder needs, the frame geometry and the refusals the decoders share.  The four
// walks over a file's markers -- parse_jpeg, the EXIF and the ICC reader (jpeg_parse.cpp), read_jpeg (jpeg_read.cpp) -- are
// built on it; which of them asks what, in which order and with which words, is theirs ("One JPEG marker walk").
// Nothing here reports an error or allocates, and the three headers below are all it needs: tests/jpeg_markers_sanitize.cpp, a
// program with its own main, runs it over untrusted bytes under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace ifhip::jpeg {
// zigzag position -> natural (row-major) position of a coefficient: the host's one copy
inline constexpr uint8_t kNaturalOrder[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                                              15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint32_t kMaxBlocksInMcu = 10;        // libjpeg's D_MAX_BLOCKS_IN_MCU
enum : uint8_t { kDHT = 0xC4, kEOI = 0xD9, kSOS = 0xDA, kDQT = 0xDB, kDRI = 0xDD, kAPP1 = 0xE1, kAPP2 = 0xE2, kAPP14 = 0xEE };
inline bool is_sof(uint8_t m) { return m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC; }
inline bool has_soi(const uint8_t* d, size_t len) { return d && len >= 4 && d[0] == 0xFF && d[1] == 0xD8; }

// ---- the walk ------------------------------------------------------------------------------------------------------------------
struct Segment { uint8_t marker; const uint8_t* data; size_t size; };          // the payload behind the two length bytes
enum class Step { Segment, End, NotAMarker, Truncated };
// The segment at or behind d[*at] (fill bytes and the markers without a payload -- SOI, RSTn, TEM -- are passed over) and *at
// behind it.  End: EOI, or fewer than 4 bytes left.  NotAMarker: d[*at] is not FF.  Truncated: the length is below 2 or runs
// over `len`; seg->marker says whose.  A walk starts at 2, behind the SOI that has_soi() saw.
inline Step next_segment(const uint8_t* d, size_t len, size_t* at, Segment* seg) {
    size_t i = *at;
    while (i + 4 <= len) {
        if (d[i] != 0xFF) { *at = i; return Step::NotAMarker; }
        while (i < len && d[i] == 0xFF) ++i;                                   // fill bytes
        if (i >= len) break;
        const uint8_t m = d[i++];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;      // no payload
        if (m == kEOI || i + 2 > len) break;
        const size_t n = (static_cast<size_t>(d[i]) << 8) | d[i + 1];
        seg->marker = m;
        if (n < 2 || i + n > len) return Step::Truncated;
        seg->data = d + i + 2; seg->size = n - 2;
        *at = i + n;
        return Step::Segment;
    }
    return Step::End;
}

// ---- the segments: each reader returns false for a segment that breaks the syntax and writes only through its arguments ----------
// DQT: any number of tables, 8- or 16-bit entries, into natural order
inline bool read_dqt(const Segment& s, uint16_t qt[4][64], bool present[4]) {
    const uint8_t* q = s.data;
    for (size_t k = 0; k < s.size;) {
        const int pq = q[k] >> 4, t = q[k] & 15;
        ++k;
        if (t > 3 || k + (pq ? 128u : 64u) > s.size) return false;
        for (int z = 0; z < 64; ++z, k += pq ? 2 : 1) qt[t][kNaturalOrder[z]] = pq ? static_cast<uint16_t>((q[k] << 8) | q[k + 1]) : q[k];
        present[t] = true;
    }
    return true;
}
struct HuffSpec { uint8_t bits[17]; uint8_t vals[256]; bool present = false; };
// DHT: any number of tables, a tail too short for another one's 17 bytes is ignored.  *defined: bit th (DC) / 4 + th (AC) per table read.
// (Inlined by force, like the geometry below: a header parse takes a quarter of a microsecond, and a call per segment shows in it.)
[[gnu::always_inline]] inline bool read_dht(const Segment& s, HuffSpec dc[4], HuffSpec ac[4], uint32_t* defined) {
    const uint8_t* q = s.data;
    *defined = 0;
    for (size_t k = 0; k + 17 <= s.size;) {
        const int tc = q[k] >> 4, th = q[k] & 15;
        if (tc > 1 || th > 3) return false;
        HuffSpec& h = tc ? ac[th] : dc[th];
        h.bits[0] = 0;
        size_t total = 0;
        for (int l = 1; l <= 16; ++l) { h.bits[l] = q[k + l]; total += q[k + l]; }
        k += 17;
        if (total > 256 || k + total > s.size) return false;
        std::memset(h.vals, 0, sizeof h.vals);
        std::memcpy(h.vals, q + k, total);
        k += total;
        h.present = true;
        *defined |= 1u << (4 * tc + th);
    }
    return true;
}
struct FrameHeader {                                 // a SOFn body
    uint8_t process = 0;                             // the marker: C0 baseline, C1 extended sequential, C2 progressive, ...
    int precision = 0, ncomp = 0;
    uint32_t width = 0, height = 0;
    uint8_t comp_id[3] = {0, 0, 0}, hs[3] = {0, 0, 0}, vs[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
    bool progressive() const { return process == 0xC2; }
};
struct Tables {                                      // what the table segments in front of a scan leave behind
    uint16_t qt[4][64];
    bool qt_present[4] = {false, false, false, false};
    HuffSpec dc[4], ac[4];
    uint32_t restart_interval = 0;
    int adobe_transform = -1;                        // APP14 "Adobe" colour transform flag, -1: no such marker
};
enum class Sof { Ok, Precision, ComponentCount, Short };
// 8-bit frames of 1 or 3 components; else what stands in the way, in the order the decoders report it.  A zero dimension is the caller's.
inline Sof read_sof(const Segment& s, FrameHeader* f) {
    const uint8_t* q = s.data;
    f->process = s.marker;
    f->precision = s.size ? q[0] : 0;
    if (s.size < 6 || q[0] != 8) return Sof::Precision;
    f->height = (q[1] << 8) | q[2];
    f->width = (q[3] << 8) | q[4];
    f->ncomp = q[5];
    if (f->ncomp != 1 && f->ncomp != 3) return Sof::ComponentCount;
    if (s.size < 6u + 3u * f->ncomp) return Sof::Short;
    for (int c = 0; c < f->ncomp; ++c) { f->comp_id[c] = q[6 + 3 * c]; f->hs[c] = q[7 + 3 * c] >> 4; f->vs[c] = q[7 + 3 * c] & 15; f->tq[c] = q[8 + 3 * c] & 3; }
    return Sof::Ok;
}
inline bool read_dri(const Segment& s, uint32_t* interval) {
    if (s.size >= 2) *interval = (s.data[0] << 8) | s.data[1];
    return s.size >= 2;
}
// APP14 "Adobe": the colour transform flag (0: RGB / CMYK stored as is, 1: YCbCr, 2: YCCK); false: not that marker
inline bool read_adobe(const Segment& s, int* transform) {
    if (s.marker != kAPP14 || s.size < 12 || std::memcmp(s.data, "Adobe", 5) != 0) return false;
    *transform = s.data[11];
    return true;
}

// ---- the frame: refusals (each caller asks them in its own order and words them itself) and geometry -------------------------------
inline bool factors_in_range(const FrameHeader& f, int c) { return f.hs[c] >= 1 && f.hs[c] <= 2 && f.vs[c] >= 1 && f.vs[c] <= 2; }
// libjpeg's colour-space guess (jdapimin.c default_decompress_parms): the pixel stage converts YCbCr only
inline bool rgb_coded(const FrameHeader& f, int adobe) { return f.ncomp == 3 && (adobe == 0 || (adobe < 0 && f.comp_id[0] == 'R' && f.comp_id[1] == 'G' && f.comp_id[2] == 'B')); }
struct Geometry {
    uint32_t hmax = 1, vmax = 1, mcus_w = 0, mcus_h = 0, blocks_per_mcu = 0;
    uint32_t bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};   // MCU-padded plane sizes in blocks
    uint32_t wb[3] = {0, 0, 0}, hb[3] = {0, 0, 0};   // jdinput.c width_in_blocks / height_in_blocks (what a non-interleaved scan covers)
};
// jdinput.c initial_setup / per_scan_setup, for factors in range (1 or 2: an MCU is 8 or 16 pixels a side, a division is a shift).
// A single component is never interleaved: its factors become 1x1.
[[gnu::always_inline]] inline void frame_geometry(FrameHeader* f, Geometry* g) {
    if (f->ncomp == 1) f->hs[0] = f->vs[0] = 1;
    g->hmax = g->vmax = 1; g->blocks_per_mcu = 0;
    for (int c = 0; c < f->ncomp; ++c) { if (f->hs[c] > g->hmax) g->hmax = f->hs[c]; if (f->vs[c] > g->vmax) g->vmax = f->vs[c]; }
    const uint32_t xs = 2 + g->hmax, ys = 2 + g->vmax, xr = (1u << xs) - 1, yr = (1u << ys) - 1;
    g->mcus_w = (f->width + xr) >> xs;
    g->mcus_h = (f->height + yr) >> ys;
    for (int c = 0; c < f->ncomp; ++c) {
        g->bw[c] = g->mcus_w * f->hs[c]; g->bh[c] = g->mcus_h * f->vs[c];
        g->wb[c] = (f->width * f->hs[c] + xr) >> xs; g->hb[c] = (f->height * f->vs[c] + yr) >> ys;      // (65 535 x 2: no overflow)
        g->blocks_per_mcu += f->hs[c] * f->vs[c];
    }
}
// The pixel stage's whitelist (make_geom): luma carries the maximum factors, chroma is 1x1 -- 4:4:4, 4:2:2, 4:4:0, 4:2:0.
[[gnu::always_inline]] inline bool chroma_is_1x1(const FrameHeader& f, const Geometry& g) { return f.ncomp != 3 || (f.hs[0] == g.hmax && f.vs[0] == g.vmax && f.hs[1] == 1 && f.vs[1] == 1 && f.hs[2] == 1 && f.vs[2] == 1); }
// libjpeg refuses more than D_MAX_BLOCKS_IN_MCU blocks (2x2 / 2x2 / 2x2 has 12); the entropy stage's per-MCU tables are sized by it.
inline bool within_block_limit(const Geometry& g) { return g.blocks_per_mcu <= kMaxBlocksInMcu; }

// What the C entry points report of a frame: null pointers are skipped, a component the frame does not have reads 0 -- and so
// does the quantisation table of one whose DQT has not come (ifhip_jpeg_frame_info can meet that; parse_jpeg refuses it).
inline void report_frame(const FrameHeader& f, const Geometry& g, uint32_t* width, uint32_t* height, int* n_components, uint8_t* h_samp3,
                         uint8_t* v_samp3, uint32_t* blocks_w3 = nullptr, uint32_t* blocks_h3 = nullptr) {
    if (width) *width = f.width;
    if (height) *height = f.height;
    if (n_components) *n_components = f.ncomp;
    for (int c = 0; c < 3; ++c) {
        if (h_samp3) h_samp3[c] = c < f.ncomp ? f.hs[c] : 0;
        if (v_samp3) v_samp3[c] = c < f.ncomp ? f.vs[c] : 0;
        if (blocks_w3) blocks_w3[c] = c < f.ncomp ? g.bw[c] : 0;
        if (blocks_h3) blocks_h3[c] = c < f.ncomp ? g.bh[c] : 0;
    }
}
inline void report_quant_tables(const FrameHeader& f, const Tables& t, uint16_t* qt3x64) {
    for (int c = 0; qt3x64 && c < 3; ++c) {
        if (c < f.ncomp && t.qt_present[f.tq[c]]) std::memcpy(qt3x64 + 64 * c, t.qt[f.tq[c]], 128);
        else std::memset(qt3x64 + 64 * c, 0, 128);
    }
}

}  // namespace ifhip::jpeg
