// jpeg_parse.cpp -- the host front end of the baseline JPEG path, on the one marker walk of jpeg_markers.hpp: the headers of a
// single-scan file and its un-stuffed scan for the entropy stage (jpeg_entropy.hip), the EXIF orientation and the embedded ICC
// profile as the reference's decoder reads them.  Everything here reads untrusted bytes and nothing here touches the device.
#include "jpeg_parse.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <utility>

#include "common.hpp"

namespace ifhip {
using jpeg::Step;

int parse_jpeg(const uint8_t* d, size_t len, ParsedJpeg* out) {
    ParsedJpeg& P = *out;
    if (!jpeg::has_soi(d, len)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: not a JPEG (no SOI)");
    size_t i = 2;
    bool have_sof = false;
    jpeg::Segment s;
    for (Step step; (step = jpeg::next_segment(d, len, &i, &s)) != Step::End;) {
        if (step == Step::NotAMarker) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: marker expected at byte %zu", i);
        if (step == Step::Truncated) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: truncated marker segment FF%02X", s.marker);
        const uint8_t m = s.marker;
        uint32_t defined = 0;
        if (m == jpeg::kDQT) {
            if (!jpeg::read_dqt(s, P.qt, P.qt_present)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad DQT");
        } else if (m == jpeg::kDHT) {
            if (!jpeg::read_dht(s, P.dc, P.ac, &defined)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad DHT");
        } else if (m == 0xC0 || m == 0xC1) {                                   // baseline / extended sequential, Huffman; a later one overwrites
            const jpeg::Sof sof = jpeg::read_sof(s, &P);
            if (sof == jpeg::Sof::Precision) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: %d-bit JPEG", P.precision);
            if (sof == jpeg::Sof::ComponentCount) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: %d-component JPEG", P.ncomp);
            if (sof == jpeg::Sof::Short) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad SOF");
            have_sof = true;
        } else if (jpeg::is_sof(m)) {                                          // (the shim's fall-back to jpeg_read.cpp keys on this code)
            return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: JPEG process SOF%d (only baseline Huffman)", m - 0xC0);
        } else if (m == jpeg::kDRI) {
            jpeg::read_dri(s, &P.restart_interval);
        } else if (m == jpeg::kSOS) {                                          // the first scan ends the walk: it must be the only one
            const uint8_t* q = s.data;
            if (!have_sof) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: SOS before SOF");
            if (s.size < 1 || q[0] != P.ncomp || s.size < 4u + 2u * P.ncomp)
                return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: non-interleaved / multi-scan JPEG");
            for (int c = 0; c < P.ncomp; ++c) {
                int named = -1;
                for (int k = 0; k < P.ncomp; ++k) if (P.comp_id[k] == q[1 + 2 * c]) named = k;
                if (named != c) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: scan component order");
                P.td[c] = q[2 + 2 * c] >> 4; P.ta[c] = q[2 + 2 * c] & 15;
                if (P.td[c] > 3 || P.ta[c] > 3) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad SOS");
            }
            P.scan_begin = i;
            break;
        } else {
            jpeg::read_adobe(s, &P.adobe_transform);
        }
    }
    // the frame is judged behind the scan header (read_jpeg judges it at the SOF): a zero dimension counts as no frame
    if (!have_sof || !P.scan_begin || P.width == 0 || P.height == 0) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: no frame / scan found");
    if (jpeg::rgb_coded(P, P.adobe_transform)) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: RGB-coded JPEG (no YCbCr transform)");
    for (int c = 0; c < P.ncomp; ++c) {
        if (!jpeg::factors_in_range(P, c)) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: sampling factor %dx%d", P.hs[c], P.vs[c]);
        if (!P.qt_present[P.tq[c]] || !P.dc[P.td[c]].present || !P.ac[P.ta[c]].present)
            return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: missing quantisation or Huffman table");
    }
    jpeg::frame_geometry(&P, &P);
    if (!jpeg::chroma_is_1x1(P, P))
        return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: sampling %dx%d,%dx%d,%dx%d (chroma must be 1x1)", P.hs[0], P.vs[0], P.hs[1], P.vs[1], P.hs[2], P.vs[2]);
    if (!jpeg::within_block_limit(P)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: %u blocks per MCU (limit %u)", P.blocks_per_mcu, kMaxBlocksInMcu);
    return IFHIP_OK;
}

// ---- un-stuffing: one walk over a scan's bytes.  The sink says where a run between two FFs and a stuffed FF go, what opens a restart
// segment and what its end does with its MCUs (false: stop): lambdas of the two callers below, inlined into the walk -- no call per run.
template <typename Begin, typename Run, typename Stuffed, typename End>
static uint32_t unstuff_walk(const uint8_t* d, size_t len, const ParsedJpeg& P, Begin begin_segment, Run run, Stuffed stuffed_ff, End end_segment) {
    const uint32_t total_mcus = P.mcus_w * P.mcus_h;
    const uint32_t per_seg = P.restart_interval ? P.restart_interval : total_mcus;
    uint32_t mcu0 = 0;
    size_t i = P.scan_begin;
    bool more = true;
    while (more && mcu0 < total_mcus) {
        begin_segment();
        more = false;
        while (i < len) {
            const uint8_t* ff = static_cast<const uint8_t*>(std::memchr(d + i, 0xFF, len - i));
            const size_t run_end = ff ? static_cast<size_t>(ff - d) : len;
            run(d + i, run_end - i);
            i = run_end;
            if (i >= len) break;
            ++i;                                                           // the 0xFF
            while (i < len && d[i] == 0xFF) ++i;                           // fill bytes before a marker
            if (i >= len) break;
            const uint8_t m = d[i++];
            if (m == 0x00) { stuffed_ff(); continue; }
            more = m >= 0xD0 && m <= 0xD7;                                 // restart: next segment; EOI or any other marker: the scan ends
            break;
        }
        const uint32_t mcus = std::min(per_seg, total_mcus - mcu0);
        more = end_segment(mcu0, mcus) && more;
        mcu0 += mcus;
    }
    return mcu0;
}

uint32_t unstuff_scan(const uint8_t* d, size_t len, const ParsedJpeg& P, std::vector<std::vector<uint8_t>>* seg_bytes, ScanSegments* segs) {
    return unstuff_walk(d, len, P, [&] { seg_bytes->emplace_back(); },
                        [&](const uint8_t* p, size_t n) { seg_bytes->back().insert(seg_bytes->back().end(), p, p + n); },
                        [&] { seg_bytes->back().push_back(0xFF); },
                        [&](uint32_t first, uint32_t n) { segs->mcu0.push_back(first); segs->mcus.push_back(n); return true; });
}
size_t packed_scan_bound(size_t len, const ParsedJpeg& P) {
    const uint32_t total_mcus = P.mcus_w * P.mcus_h;
    const uint32_t per_seg = P.restart_interval ? P.restart_interval : total_mcus;
    const size_t max_segs = per_seg ? (static_cast<size_t>(total_mcus) + per_seg - 1) / per_seg : 1;
    return (len > P.scan_begin ? len - P.scan_begin : 0) + (max_segs + 1) * (kSubBits / 8u);
}
uint32_t unstuff_scan_packed(const uint8_t* d, size_t len, const ParsedJpeg& P, uint8_t* dst, size_t cap, ScanSegments* segs) {
    constexpr size_t kSubBytes = kSubBits / 8u;
    uint64_t& subs = segs->n_sub;
    uint8_t* out = nullptr;                                                // the open segment: where it starts, its bytes so far, its room
    size_t nb = 0, room = 0;                                               // (the bound leaves a sub-sequence per segment beyond the scan's bytes)
    return unstuff_walk(d, len, P, [&] { out = dst + subs * kSubBytes; nb = 0; room = cap - static_cast<size_t>(subs) * kSubBytes; },
        [&](const uint8_t* p, size_t n) {
            if (nb + n + 1 + kSubBytes > room) throw std::length_error("scan staging bound exceeded");
            std::memcpy(out + nb, p, n); nb += n;
        },
        [&] { out[nb++] = 0xFF; },
        [&](uint32_t first, uint32_t n) __attribute__((noinline)) {       // (out of line: its vectors' registers stay out of the run loop, 2 % of a 4K scan)
            const uint64_t bits = static_cast<uint64_t>(nb) * 8u, ns = std::max<uint64_t>(1, (bits + kSubBits - 1) / kSubBits);
            std::memset(out + nb, 0, static_cast<size_t>(ns) * kSubBytes - nb);               // pad to the 1 024-bit boundary
            segs->mcu0.push_back(first); segs->mcus.push_back(n); segs->bits.push_back(bits);
            segs->nsub.push_back(static_cast<uint32_t>(ns)); segs->first_word.push_back(static_cast<uint32_t>(subs * kSubWords));
            subs += ns;
            return subs * kSubBits + 4096 < (1ull << 32);                  // (else the caller refuses: more than 512 MB of scan data)
        });
}

// Does an ICC profile describe sRGB itself (see ifhip_jpeg_icc_profile_kind in include/imageflow_hip.h: an RGB matrix profile
// with the sRGB primaries within 0.003 after D50 adaptation and the sRGB tone curve)?  Shared by the JPEG (APP2) and the PNG
// (iCCP) readers.
bool icc_describes_srgb(const uint8_t* profile, size_t profile_bytes) {
    const uint8_t* const icc = profile;
    // ICC.1 header: size (0..3), colour space (16..19), PCS (20..23); tag table at 128: count, then {sig, offset, size}
    auto be32 = [&](size_t o) { return (static_cast<uint32_t>(icc[o]) << 24) | (static_cast<uint32_t>(icc[o + 1]) << 16) | (static_cast<uint32_t>(icc[o + 2]) << 8) | icc[o + 3]; };
    if (profile_bytes < 132 || std::memcmp(&icc[16], "RGB ", 4) != 0 || std::memcmp(&icc[20], "XYZ ", 4) != 0) return false;
    const uint32_t tags = be32(128);
    if (tags > 200 || 132 + static_cast<size_t>(tags) * 12 > profile_bytes) return false;
    auto find = [&](const char* sig, size_t* off, size_t* size) {
        for (uint32_t t = 0; t < tags; ++t) {
            const size_t e = 132 + static_cast<size_t>(t) * 12;
            if (std::memcmp(&icc[e], sig, 4) != 0) continue;
            *off = be32(e + 4); *size = be32(e + 8);
            return *off + *size <= profile_bytes && *size >= 8;
        }
        return false;
    };
    // primaries, D50-adapted (IEC 61966-2-1 through Bradford, as every sRGB profile carries them)
    static const double want[3][3] = {{0.4360, 0.2225, 0.0139}, {0.3851, 0.7169, 0.0971}, {0.1431, 0.0606, 0.7141}};
    const char* xyz_sig[3] = {"rXYZ", "gXYZ", "bXYZ"};
    for (int c = 0; c < 3; ++c) {
        size_t off = 0, size = 0;
        if (!find(xyz_sig[c], &off, &size) || size < 20 || std::memcmp(&icc[off], "XYZ ", 4) != 0) return false;
        for (int k = 0; k < 3; ++k) {
            const double v = static_cast<int32_t>(be32(off + 8 + 4 * static_cast<size_t>(k))) / 65536.0;
            if (std::fabs(v - want[c][k]) > 0.003) return false;
        }
    }
    // tone curves: the sRGB parametric form (type 3: g 2.4, a 1/1.055, b 0.055/1.055, c 1/12.92, d 0.04045) or a sampled curve
    // whose entries follow the sRGB function (checked at every entry; 2 of 65535 is the 16-bit tables' own rounding)
    const char* trc_sig[3] = {"rTRC", "gTRC", "bTRC"};
    for (int c = 0; c < 3; ++c) {
        size_t off = 0, size = 0;
        if (!find(trc_sig[c], &off, &size) || size < 12) return false;
        if (std::memcmp(&icc[off], "para", 4) == 0) {
            if (size < 12 + 20 || ((static_cast<uint32_t>(icc[off + 8]) << 8) | icc[off + 9]) != 3u) return false;
            static const double p[5] = {2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.04045};
            for (int k = 0; k < 5; ++k)
                if (std::fabs(static_cast<int32_t>(be32(off + 12 + 4 * static_cast<size_t>(k))) / 65536.0 - p[k]) > 0.002) return false;
        } else if (std::memcmp(&icc[off], "curv", 4) == 0) {
            const uint32_t n = be32(off + 8);
            if (n < 256 || 12 + static_cast<size_t>(n) * 2 > size) return false;      // (a single gamma value is not the sRGB curve)
            for (uint32_t k = 0; k < n; ++k) {
                const double x = static_cast<double>(k) / (n - 1), y = x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4);
                const double got = ((static_cast<uint32_t>(icc[off + 12 + 2 * static_cast<size_t>(k)]) << 8) | icc[off + 13 + 2 * static_cast<size_t>(k)]) / 65535.0;
                if (std::fabs(got - y) > 2.0 / 65535.0 + 1e-4) return false;
            }
        } else {
            return false;
        }
    }
    return true;
}

// The embedded ICC profile (see include/imageflow_hip.h).  libjpeg's jpeg_read_icc_profile rule: APP2 markers whose data starts
// with "ICC_PROFILE\0", then a 1-based sequence number and the marker count; every number must occur exactly once with the
// same count.  A chunk set that breaks the rule -- inconsistent counts, a sequence number out of range or twice, a missing
// chunk, nothing but empty chunks -- is NO profile to the reference (read_icc_profile returns None,
// mozjpeg_decoder_helpers.rs:42-83: the frame is decoded without a transform) and kind 0 here; so is a GRAY profile on a
// colour frame (mozjpeg_decoder.rs:391-395 -> SourceProfile::Srgb).  Like the EXIF reader's, the walk never fails behind the SOI
// check: it ends at the scan (jpeg_read_header stops there) and at whatever the strict walks refuse.
int jpeg_icc_profile(const uint8_t* d, size_t len, int* kind, std::vector<uint8_t>* profile) {
    if (!kind) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *kind = 0;
    std::vector<uint8_t>& icc = *profile;
    icc.clear();
    if (!jpeg::has_soi(d, len)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: not a JPEG (no SOI)");
    std::vector<std::pair<const uint8_t*, size_t>> chunk(256, {nullptr, 0});
    uint32_t count = 0, seen = 0;
    bool broken = false;
    int frame_components = 0;
    size_t i = 2;
    for (jpeg::Segment s; jpeg::next_segment(d, len, &i, &s) == Step::Segment && s.marker != jpeg::kSOS;) {
        const uint8_t* q = s.data;
        if (jpeg::is_sof(s.marker) && s.size >= 6) frame_components = q[5];                                        // any SOFn: P, Y, X, Nf
        if (s.marker != jpeg::kAPP2 || s.size < 14 || std::memcmp(q, "ICC_PROFILE\0", 12) != 0) continue;
        const uint32_t seq = q[12], num = q[13];
        if (seq == 0 || num == 0 || seq > num || (count && num != count) || chunk[seq].first) { broken = true; continue; }
        count = num;
        chunk[seq] = {q + 14, s.size - 14};
        ++seen;
    }
    if (!seen || broken || seen != count) return IFHIP_OK;              // no profile, or a chunk set the reference drops
    for (uint32_t k = 1; k <= count; ++k) icc.insert(icc.end(), chunk[k].first, chunk[k].first + chunk[k].second);
    if (icc.empty()) return IFHIP_OK;                                    // only empty markers: None
    if (icc.size() >= 20 && std::memcmp(&icc[16], "GRAY", 4) == 0 && frame_components != 1) { icc.clear(); return IFHIP_OK; }   // -> SourceProfile::Srgb
    *kind = icc_describes_srgb(icc.data(), icc.size()) ? 1 : 2;
    return IFHIP_OK;
}

}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_jpeg_parse_headers(const uint8_t* jpeg, size_t len, uint32_t* width, uint32_t* height, int* n_components, uint8_t* h_samp3,
                             uint8_t* v_samp3, uint32_t* blocks_w3, uint32_t* blocks_h3, uint16_t* qt3x64, uint32_t* restart_interval) {
    ParsedJpeg P;
    if (int rc = parse_jpeg(jpeg, len, &P)) return rc;
    jpeg::report_frame(P, P, width, height, n_components, h_samp3, v_samp3, blocks_w3, blocks_h3);
    jpeg::report_quant_tables(P, P, qt3x64);
    if (restart_interval) *restart_interval = P.restart_interval;
    return IFHIP_OK;
}

// EXIF orientation of a JPEG as MozJpegDecoder reads it (codecs/mozjpeg_decoder_helpers.rs:107-202; the decoder saves
// APP1 and APP2 markers up to 0xffff bytes, mozjpeg_decoder.rs:551-558): the FIRST saved marker whose data starts with
// "Exif\0\0" decides -- shorter than 32 bytes: none; the TIFF header is looked for at offsets 0..15; IFD0's entries are
// walked for tag 0x0112, rejected only if its type is not SHORT AND its count is not 1 (sic, `&&`), values above 8 are none.
// Every read behind the data's end is the reference's io error, i.e. none.  *flag: -1 none, else 0..8.
int ifhip_jpeg_exif_orientation(const uint8_t* d, size_t len, int* flag) {
    if (!flag) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *flag = -1;
    if (!jpeg::has_soi(d, len)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: not a JPEG (no SOI)");
    size_t i = 2;
    for (jpeg::Segment s; jpeg::next_segment(d, len, &i, &s) == Step::Segment && s.marker != jpeg::kSOS;) {
        const uint8_t* q = s.data;
        const size_t n = s.size;
        if ((s.marker != jpeg::kAPP1 && s.marker != jpeg::kAPP2) || n < 6 || std::memcmp(q, "Exif\0\0", 6) != 0) continue;
        if (n < 32) return IFHIP_OK;                                             // "EXIF too short"
        size_t tiff = 16;
        bool little = false;
        for (size_t t = 0; t < 16 && tiff == 16; ++t) {
            if (std::memcmp(q + t, "II\x2a\0", 4) == 0) { tiff = t; little = true; }
            else if (std::memcmp(q + t, "MM\0\x2a", 4) == 0) { tiff = t; little = false; }
        }
        if (tiff == 16) return IFHIP_OK;
        const uint8_t* r = q + tiff + 4;
        const uint64_t rn = n - tiff - 4;
        uint64_t pos = 0;
        bool eof = false;
        auto rd = [&](uint32_t bytes) -> uint32_t {
            if (eof || pos + bytes > rn) { eof = true; return 0; }
            uint32_t v = 0;
            for (uint32_t k = 0; k < bytes; ++k) v |= static_cast<uint32_t>(r[pos + k]) << (little ? 8u * k : 8u * (bytes - 1u - k));
            pos += bytes;
            return v;
        };
        const uint32_t offset = rd(4);
        if (eof) return IFHIP_OK;
        pos = static_cast<uint64_t>(std::max<uint32_t>(4u, offset)) - 4u;
        const uint32_t tags = rd(2);
        for (uint32_t k = 0; k < tags && !eof; ++k) {
            if (rd(2) == 0x112u && !eof) {
                const uint32_t type = rd(2), count = rd(4);
                if (eof || (type != 3u && count != 1u)) return IFHIP_OK;
                const uint32_t v = rd(2);
                if (!eof && v <= 8u) *flag = static_cast<int>(v);
                return IFHIP_OK;
            }
            pos += 10;
        }
        return IFHIP_OK;
    }
    return IFHIP_OK;
}

int ifhip_jpeg_icc_profile_kind(const uint8_t* d, size_t len, int* kind) {
    std::vector<uint8_t> icc;
    return ifhip::jpeg_icc_profile(d, len, kind, &icc);
}

}  // extern "C"
