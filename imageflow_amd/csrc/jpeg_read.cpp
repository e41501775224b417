// jpeg_read.cpp -- host-side entropy decoding of the Huffman JPEGs the GPU entropy stage does not take: progressive (SOF2)
// files -- what the reference's own `mozjpeg` encoder preset writes (codecs/mozjpeg.rs:121-123) and MozJpegDecoder reads back
// (codecs/mozjpeg_decoder.rs:295-420 -> libjpeg jdphuff.c) -- and sequential files with several or non-interleaved scans.
// Output = the quantised coefficient planes of the pixel stage ([blocks_h][blocks_w][64] int16, natural order, MCU-padded:
// the layout of jpeg_read_coefficients and of csrc/jpeg_entropy.hip), so everything behind the entropy stage -- IDCT,
// up-sampling, colour, the fused resample -- is the GPU path unchanged.  The scans are serial bit streams with state that
// spans the whole image (successive approximation refines coefficients of earlier scans): host work, like the reference's.
//
// Follows libjpeg's published decoder (jdmarker.c marker syntax, jdhuff.c decode_mcu, jdphuff.c decode_mcu_DC_first /
// _AC_first / _DC_refine / _AC_refine, jdinput.c per-scan geometry).  Pinned by tests/test_jpeg_progressive.py: files this
// library's own progressive WRITER produced from known coefficients (byte-identical to libjpeg-turbo's) decode to
// exactly those coefficients, and Pillow-written progressive files decode, through the GPU pixel stage, to Pillow's pixels.
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "common.hpp"
#include "jpeg_markers.hpp"

namespace ifhip {
namespace {

constexpr auto& kZig = jpeg::kNaturalOrder;
struct HuffTab {                       // jdhuff.c jpeg_make_d_derived_tbl: canonical codes by length
    bool present = false;
    const uint8_t* vals = nullptr;     // the specification's, in the frame
    int32_t maxcode[18];               // largest code of length l, -1 if none
    int32_t valoff[17];                // huffval index of the first code of length l minus that code
    uint8_t look_len[256], look_sym[256];      // 8-bit lookahead: code length (0: longer than 8) and symbol
    void derive(const jpeg::HuffSpec& h) {
        const uint8_t* bits = h.bits;
        present = true;
        vals = h.vals;
        int32_t code = 0;
        int k = 0;
        std::memset(look_len, 0, sizeof look_len);
        for (int l = 1; l <= 16; ++l) {
            valoff[l] = k - code;
            for (int i = 0; i < bits[l]; ++i, ++k, ++code)
                if (l <= 8) {
                    const int first = code << (8 - l);
                    for (int f = 0; f < (1 << (8 - l)); ++f)
                        if (first + f < 256) { look_len[first + f] = static_cast<uint8_t>(l); look_sym[first + f] = vals[k & 255]; }
                }
            maxcode[l] = bits[l] ? code - 1 : -1;
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
    }
};

struct Frame : jpeg::FrameHeader, jpeg::Geometry, jpeg::Tables {
    uint16_t qt_latched[3][64];                               // jdinput.c latch_quant_tables: a component's table as it stood at its FIRST scan
    bool latched[3] = {false, false, false};
};

struct BitReader {                     // jdhuff.c fill_bit_buffer: bytes with FF00 un-stuffed, zeros behind a marker
    const uint8_t* d;
    size_t len, pos;
    uint64_t acc = 0;
    int n = 0;
    bool hit_marker = false;
    void fill() {
        while (n <= 56) {
            uint32_t b = 0;
            if (!hit_marker && pos < len) {
                b = d[pos];
                if (b == 0xFF) {
                    size_t q = pos + 1;
                    while (q < len && d[q] == 0xFF) ++q;                 // fill bytes
                    if (q < len && d[q] == 0x00) { pos = q + 1; }
                    else { hit_marker = true; b = 0; }                    // a marker: the scan's data ends here (pos stays on the FF)
                } else ++pos;
            }
            acc |= static_cast<uint64_t>(b) << (56 - n);
            n += 8;
        }
    }
    uint32_t peek(int k) { if (n < k) fill(); return static_cast<uint32_t>(acc >> (64 - k)); }
    void drop(int k) { acc <<= k; n -= k; }
    uint32_t get(int k) { if (k == 0) return 0; const uint32_t v = peek(k); drop(k); return v; }
    void align_to_marker() { acc = 0; n = 0; hit_marker = false; }
};

inline int32_t extend(uint32_t r, int s) { return r < (1u << (s - 1)) ? static_cast<int32_t>(r) - ((1 << s) - 1) : static_cast<int32_t>(r); }

int decode_symbol(BitReader& br, const HuffTab& t, int* sym) {
    const uint32_t look = br.peek(8);
    if (t.look_len[look]) { br.drop(t.look_len[look]); *sym = t.look_sym[look]; return 0; }
    int l = 9;
    int32_t code = static_cast<int32_t>(br.peek(9));
    while (l <= 16 && code > t.maxcode[l]) { ++l; code = static_cast<int32_t>(br.peek(l)); }
    if (l > 16) return -1;                                                // no such code (jdhuff.c JWRN_HUFF_BAD_CODE)
    br.drop(l);
    *sym = t.vals[(code + t.valoff[l]) & 255];
    return 0;
}

struct ScanComp { int ci, td, ta; };

}  // namespace

// The frame checks and the geometry of a frame whose header has been read: at the SOF, and again at an Adobe marker behind it
// (parse_jpeg asks the same questions behind the scan header, RGB-coded first: jpeg_parse.cpp).
static int finish_frame(Frame& F) {
    for (int c = 0; c < F.ncomp; ++c)
        if (!jpeg::factors_in_range(F, c)) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: sampling factor %dx%d", F.hs[c], F.vs[c]);
    jpeg::frame_geometry(&F, &F);
    if (!jpeg::chroma_is_1x1(F, F))
        return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: sampling %dx%d,%dx%d,%dx%d (chroma must be 1x1)", F.hs[0], F.vs[0], F.hs[1], F.vs[1], F.hs[2], F.vs[2]);
    if (jpeg::rgb_coded(F, F.adobe_transform)) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: RGB-coded JPEG (no YCbCr transform)");
    return IFHIP_OK;
}

// One pass over the markers.  coef == nullptr: stop at the first SOS (frame facts only).
static int read_jpeg(const uint8_t* d, size_t len, Frame* out, int16_t* const coef[3]) {
    Frame& F = *out;
    if (!jpeg::has_soi(d, len)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: not a JPEG (no SOI)");
    HuffTab dc[4], ac[4];                                                 // derived from F.dc / F.ac as they arrive
    bool have_sof = false, any_scan = false;
    // (jdphuff.c's coef_bits bookkeeping only WARNS about scripts that send bits out of order -- JWRN_BOGUS_PROGRESSION -- and
    // decodes them anyway; there is no warning channel here, so such scans are decoded as libjpeg decodes them)
    size_t i = 2;
    jpeg::Segment seg;
    for (jpeg::Step step; (step = jpeg::next_segment(d, len, &i, &seg)) != jpeg::Step::End;) {
        if (step == jpeg::Step::NotAMarker) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: marker expected at byte %zu", i);
        if (step == jpeg::Step::Truncated) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: truncated marker segment FF%02X", seg.marker);
        const uint8_t m = seg.marker, *q = seg.data;
        const size_t n = seg.size;
        if (m == jpeg::kDQT) {
            if (!jpeg::read_dqt(seg, F.qt, F.qt_present)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad DQT");
        } else if (m == jpeg::kDHT) {
            uint32_t defined = 0;
            if (!jpeg::read_dht(seg, F.dc, F.ac, &defined)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad DHT");
            for (int t = 0; t < 4; ++t) {
                if (defined & (1u << t)) dc[t].derive(F.dc[t]);
                if (defined & (16u << t)) ac[t].derive(F.ac[t]);
            }
        } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {                 // one frame header, judged where it stands
            if (have_sof) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: two frame headers");
            const jpeg::Sof sof = jpeg::read_sof(seg, &F);
            if (sof == jpeg::Sof::Precision) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: %d-bit JPEG", F.precision);
            if (sof == jpeg::Sof::ComponentCount) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: %d-component JPEG", F.ncomp);
            if (sof == jpeg::Sof::Short || F.width == 0 || F.height == 0) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad SOF");
            if (int rc = finish_frame(F)) return rc;
            have_sof = true;
        } else if (jpeg::is_sof(m)) {
            return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: JPEG process SOF%d (Huffman sequential and progressive only)", m - 0xC0);
        } else if (m == jpeg::kDRI) {
            jpeg::read_dri(seg, &F.restart_interval);
        } else if (jpeg::read_adobe(seg, &F.adobe_transform)) {
            if (have_sof) if (int rc = finish_frame(F)) return rc;
        } else if (m == jpeg::kSOS) {
            if (!have_sof) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: SOS before SOF");
            if (!coef) return IFHIP_OK;                                   // frame facts only
            if (n < 1) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad SOS");
            const int ns = q[0];
            if (ns < 1 || ns > F.ncomp || n < 4u + 2u * ns) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad SOS");
            ScanComp sc[3];
            for (int s = 0; s < ns; ++s) {
                int c = -1;
                for (int k = 0; k < F.ncomp; ++k) if (F.comp_id[k] == q[1 + 2 * s]) c = k;
                if (c < 0) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: scan names an unknown component");
                sc[s] = ScanComp{c, q[2 + 2 * s] >> 4, q[2 + 2 * s] & 15};
                if (sc[s].td > 3 || sc[s].ta > 3) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad SOS");
            }
            const int Ss = q[1 + 2 * ns], Se = q[2 + 2 * ns], Ah = q[3 + 2 * ns] >> 4, Al = q[3 + 2 * ns] & 15;
            if (F.progressive()) {                                          // jdphuff.c start_pass_phuff_decoder's checks
                const bool dc_scan = Ss == 0;
                if ((dc_scan && Se != 0) || (!dc_scan && (Se < Ss || Se > 63 || ns != 1)) || Al > 13 || (Ah != 0 && Ah - 1 != Al))
                    return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad progressive scan parameters Ss=%d Se=%d Ah=%d Al=%d", Ss, Se, Ah, Al);
            } else if (Ss != 0 || Se != 63 || Ah != 0 || Al != 0) {
                return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: bad sequential scan parameters");
            }
            for (int s = 0; s < ns; ++s) {                                // jdinput.c latch_quant_tables (start of every scan's input pass)
                const int c = sc[s].ci;
                if (F.latched[c]) continue;                               // a DQT that redefines the table later does not reach this component
                if (!F.qt_present[F.tq[c]]) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: missing quantisation table");
                std::memcpy(F.qt_latched[c], F.qt[F.tq[c]], 128);
                F.latched[c] = true;
            }
            for (int s = 0; s < ns; ++s) {
                const bool need_dc = !F.progressive() || (Ss == 0 && Ah == 0), need_ac = !F.progressive() || Ss != 0;
                if ((need_dc && !dc[sc[s].td].present) || (need_ac && !ac[sc[s].ta].present))
                    return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: missing Huffman table");
            }
            // per-scan geometry (jdinput.c per_scan_setup): one component -> its own block raster; several -> MCUs
            const bool interleaved = ns > 1;
            const uint32_t mcus_w = interleaved ? F.mcus_w : F.wb[sc[0].ci], mcus_h = interleaved ? F.mcus_h : F.hb[sc[0].ci];
            BitReader br{d, len, i};
            int32_t last_dc[3] = {0, 0, 0};
            const uint32_t restart_interval = F.restart_interval;
            uint32_t eobrun = 0, restarts_left = restart_interval;
            const uint64_t total_mcus = static_cast<uint64_t>(mcus_w) * mcus_h;
            for (uint64_t mi = 0; mi < total_mcus; ++mi) {
                if (restart_interval && restarts_left == 0) {            // process_restart: the marker, then fresh state
                    size_t p = br.pos;
                    br.align_to_marker();
                    while (p + 1 < len && !(d[p] == 0xFF && d[p + 1] >= 0xD0 && d[p + 1] <= 0xD7)) {
                        if (d[p] == 0xFF && d[p + 1] != 0x00 && d[p + 1] != 0xFF) break;     // another marker: the scan ended early
                        ++p;
                    }
                    if (p + 1 < len && d[p] == 0xFF && d[p + 1] >= 0xD0 && d[p + 1] <= 0xD7) p += 2;
                    br.pos = p;
                    last_dc[0] = last_dc[1] = last_dc[2] = 0;
                    eobrun = 0;
                    restarts_left = restart_interval;
                }
                const uint32_t my = static_cast<uint32_t>(mi / mcus_w), mx = static_cast<uint32_t>(mi % mcus_w);
                for (int s = 0; s < ns; ++s) {
                    const int ci = sc[s].ci;
                    const uint32_t nh = interleaved ? F.hs[ci] : 1u, nv = interleaved ? F.vs[ci] : 1u;
                    for (uint32_t dy = 0; dy < nv; ++dy)
                        for (uint32_t dx = 0; dx < nh; ++dx) {
                            const uint32_t bx = mx * nh + dx, by = my * nv + dy;
                            int16_t* blk = coef[ci] + (static_cast<size_t>(by) * F.bw[ci] + bx) * 64u;
                            int sym = 0;
                            if (!F.progressive()) {                         // jdhuff.c decode_mcu
                                if (decode_symbol(br, dc[sc[s].td], &sym)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: corrupt entropy-coded data");
                                int32_t diff = 0;
                                if (sym) { if (sym > 15) sym = 15; diff = extend(br.get(sym), sym); }
                                last_dc[ci] += diff;
                                blk[0] = static_cast<int16_t>(last_dc[ci]);
                                for (int k = 1; k < 64;) {
                                    if (decode_symbol(br, ac[sc[s].ta], &sym)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: corrupt entropy-coded data");
                                    const int r = sym >> 4, sz = sym & 15;
                                    if (sz) {
                                        k += r;
                                        const int32_t v = extend(br.get(sz), sz);
                                        blk[kZig[k > 63 ? 63 : k]] = static_cast<int16_t>(v);   // (jpeg_natural_order's 16 extra entries: a corrupt run lands on 63)
                                        ++k;
                                    } else { if (r != 15) break; k += 16; }
                                }
                            } else if (Ss == 0 && Ah == 0) {              // decode_mcu_DC_first
                                if (decode_symbol(br, dc[sc[s].td], &sym)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: corrupt entropy-coded data");
                                int32_t diff = 0;
                                if (sym) { if (sym > 15) sym = 15; diff = extend(br.get(sym), sym); }
                                last_dc[ci] += diff;
                                blk[0] = static_cast<int16_t>(static_cast<uint32_t>(last_dc[ci]) << Al);
                            } else if (Ss == 0) {                         // decode_mcu_DC_refine
                                if (br.get(1)) blk[0] = static_cast<int16_t>(blk[0] | (1 << Al));
                            } else if (Ah == 0) {                         // decode_mcu_AC_first
                                if (eobrun > 0) { --eobrun; continue; }
                                for (int k = Ss; k <= Se; ++k) {
                                    if (decode_symbol(br, ac[sc[s].ta], &sym)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: corrupt entropy-coded data");
                                    const int r = sym >> 4, sz = sym & 15;
                                    if (sz) {
                                        k += r;
                                        const int32_t v = extend(br.get(sz), sz);
                                        blk[kZig[k > 63 ? 63 : k]] = static_cast<int16_t>(static_cast<uint32_t>(v) << Al);   // (likewise; jdphuff.c does not clamp to Se either)
                                    } else if (r == 15) k += 15;
                                    else {
                                        eobrun = 1u << r;
                                        if (r) eobrun += br.get(r);
                                        --eobrun;
                                        break;
                                    }
                                }
                            } else {                                      // decode_mcu_AC_refine
                                const int32_t p1 = 1 << Al, m1 = -(1 << Al);
                                int k = Ss;
                                auto correct = [&](int16_t* c) {          // one correction bit for a coefficient that is already nonzero
                                    if (br.get(1) && (*c & p1) == 0) *c = static_cast<int16_t>(*c >= 0 ? *c + p1 : *c + m1);
                                };
                                if (eobrun == 0) {
                                    for (; k <= Se; ++k) {
                                        if (decode_symbol(br, ac[sc[s].ta], &sym)) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: corrupt entropy-coded data");
                                        int r = sym >> 4;
                                        int32_t v = 0;
                                        if (sym & 15) v = br.get(1) ? p1 : m1;     // (size must be 1: a newly nonzero coefficient)
                                        else if (r != 15) {
                                            eobrun = 1u << r;
                                            if (r) eobrun += br.get(r);
                                            break;                        // the rest of the block: the end-of-band logic below
                                        }
                                        do {                              // over nonzero history and r zeros, correction bits on the way
                                            int16_t* c = blk + kZig[k];
                                            if (*c != 0) correct(c);
                                            else if (--r < 0) break;
                                            ++k;
                                        } while (k <= Se);
                                        if (v && k <= 63) blk[kZig[k]] = static_cast<int16_t>(v);
                                    }
                                }
                                if (eobrun > 0) {
                                    for (; k <= Se; ++k) { int16_t* c = blk + kZig[k]; if (*c != 0) correct(c); }
                                    --eobrun;
                                }
                            }
                        }
                }
                if (restart_interval) --restarts_left;
            }
            any_scan = true;
            // behind the scan: skip to the next marker (pad bits, stuffing)
            size_t p = br.pos;
            while (p + 1 < len && !(d[p] == 0xFF && d[p + 1] != 0x00 && d[p + 1] != 0xFF && !(d[p + 1] >= 0xD0 && d[p + 1] <= 0xD7))) ++p;
            i = p;
        }
    }
    if (!have_sof) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: no frame found");
    if (coef && !any_scan) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: no scan found");
    return IFHIP_OK;
}

}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_jpeg_frame_info(const uint8_t* jpeg, size_t len, uint32_t* width, uint32_t* height, int* n_components, uint8_t* h_samp3,
                          uint8_t* v_samp3, uint32_t* blocks_w3, uint32_t* blocks_h3, uint16_t* qt3x64, int* progressive) {
    try {
        Frame F;
        if (int rc = read_jpeg(jpeg, len, &F, nullptr)) return rc;
        jpeg::report_frame(F, F, width, height, n_components, h_samp3, v_samp3, blocks_w3, blocks_h3);
        jpeg::report_quant_tables(F, F, qt3x64);
        if (progressive) *progressive = F.progressive() ? 1 : 0;
        return IFHIP_OK;
    } catch (const std::exception& ex) { return fail(IFHIP_INVALID_STATE, "InvalidState: %s", ex.what()); }
}

int ifhip_jpeg_read_coefficients_host(const uint8_t* jpeg, size_t len, int16_t* coef0, int16_t* coef1, int16_t* coef2, uint16_t* qt3x64) {
    try {
        Frame F;
        if (int rc = read_jpeg(jpeg, len, &F, nullptr)) return rc;       // geometry first: the planes are cleared to it
        int16_t* coef[3] = {coef0, coef1, coef2};
        for (int c = 0; c < F.ncomp; ++c) {
            if (!coef[c]) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null coefficient plane");
            std::memset(coef[c], 0, static_cast<size_t>(F.bw[c]) * F.bh[c] * 128u);
        }
        Frame G;
        if (int rc = read_jpeg(jpeg, len, &G, coef)) return rc;
        // (quantisation tables may arrive between scans: a component's table is the one in force at its first scan, as libjpeg
        // latches it; a later DQT with the same id only reaches components whose first scan is still to come)
        for (int c = 0; c < G.ncomp; ++c) {
            if (!G.latched[c]) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: component %d has no scan", c);
            if (qt3x64) std::memcpy(qt3x64 + 64 * c, G.qt_latched[c], 128);
        }
        return IFHIP_OK;
    } catch (const std::bad_alloc&) { return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: host memory");
    } catch (const std::exception& ex) { return fail(IFHIP_INVALID_STATE, "InvalidState: %s", ex.what()); }
}

}  // extern "C"
