// jpeg_progressive_read.cpp -- the host front end of the device progressive JPEG decoder: one walk over the markers with
// jpeg_markers.hpp, as read_jpeg (jpeg_read.cpp) walks them, that decodes nothing.  It keeps what the kernels of
// csrc/jpeg_progressive_decode.hip need -- per scan its kind, components, band, Al, a snapshot of the Huffman tables in force at
// its SOS (a DHT between scans redefines slots), the restart interval in force (a DRI may stand between scans) and its raster
// (jdinput.c per_scan_setup) -- un-stuffs every scan and cuts it at the restart markers into streams, and gives every scan its
// dependency level: one more than the highest level of an earlier scan that touches one of its (component, coefficient) pairs.
//
// It accepts well-formed progressions only: every (component, index) first coded by exactly one Ah = 0 scan, every refinement
// with Ah equal to the Al the index stands at and Al = Ah - 1, no band over indices that stand at different Al, no AC scan of a
// component whose DC has not come (what jdphuff.c decodes with JWRN_BOGUS_PROGRESSION is left to the host reader).  Everything
// else -- sequential files, what read_jpeg refuses, tables that are no prefix code -- answers IFHIP_METHOD_NOT_IMPLEMENTED.
//
// The cut.  read_jpeg's bit reader treats FF+ 00 as a data byte FF, stops at any other marker and, at a restart boundary,
// searches forward from where it stands for the next RSTn; this walk cuts at exactly those places, so stream k holds the bytes
// read_jpeg reads for interval k.  Where they part -- a stream with fewer bits than its MCUs need, which read_jpeg pads with
// zeros -- the device raises kProgOutOfBits and the caller asks the host reader.  Fill bytes before an RSTn and pad bits of any
// value pass: a stream ends by its MCU count.
#include "jpeg_progressive_read.hpp"

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "jpeg_markers.hpp"

namespace ifhip {
namespace {

int refuse(const char* why) { return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: device progressive JPEG decoder: %s", why); }

struct Walk {
    jpeg::FrameHeader F;
    jpeg::Geometry G;
    jpeg::Tables T;
    bool have_sof = false;
    bool latched[3] = {false, false, false};
    int table_at[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};   // the slot's current definition in out->tables; -1: not derived yet
    int8_t al[3][64];                                            // the Al an index stands at, -1: not coded yet
    int level[3][64];                                            // the level of the last scan that touched it, -1: none
};

bool frame_ok(jpeg::FrameHeader& F, jpeg::Geometry& G, int adobe) {
    for (int c = 0; c < F.ncomp; ++c)
        if (!jpeg::factors_in_range(F, c)) return false;
    jpeg::frame_geometry(&F, &G);
    return jpeg::chroma_is_1x1(F, G) && !jpeg::rgb_coded(F, adobe);
}

}  // namespace

int prog_prepare(const uint8_t* d, size_t len, ProgPrepared* out) {
    if (!jpeg::has_soi(d, len)) return refuse("not a JPEG");
    if (len >= (1u << 28)) return refuse("a file of 256 MB or more");
    Walk W;
    std::memset(W.al, -1, sizeof W.al);
    for (auto& row : W.level) for (int& v : row) v = -1;
    jpeg::FrameHeader& F = W.F;
    jpeg::Tables& T = W.T;
    ProgPrepared& P = *out;
    P = ProgPrepared();
    size_t i = 2;
    jpeg::Segment seg;
    for (jpeg::Step step; (step = jpeg::next_segment(d, len, &i, &seg)) != jpeg::Step::End;) {
        if (step != jpeg::Step::Segment) return refuse("marker syntax");
        const uint8_t m = seg.marker, *q = seg.data;
        const size_t n = seg.size;
        if (m == jpeg::kDQT) {
            if (!jpeg::read_dqt(seg, T.qt, T.qt_present)) return refuse("bad DQT");
        } else if (m == jpeg::kDHT) {
            uint32_t defined = 0;
            if (!jpeg::read_dht(seg, T.dc, T.ac, &defined)) return refuse("bad DHT");
            for (int t = 0; t < 4; ++t) {
                if (defined & (1u << t)) W.table_at[0][t] = -1;
                if (defined & (16u << t)) W.table_at[1][t] = -1;
            }
        } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
            if (W.have_sof) return refuse("two frame headers");
            if (jpeg::read_sof(seg, &F) != jpeg::Sof::Ok || F.width == 0 || F.height == 0) return refuse("frame header");
            if (!F.progressive()) return refuse("sequential file");
            if (!frame_ok(F, W.G, T.adobe_transform)) return refuse("sampling or colour space");
            W.have_sof = true;
        } else if (jpeg::is_sof(m)) {
            return refuse("JPEG process");
        } else if (m == jpeg::kDRI) {
            jpeg::read_dri(seg, &T.restart_interval);
        } else if (jpeg::read_adobe(seg, &T.adobe_transform)) {
            if (W.have_sof && !frame_ok(F, W.G, T.adobe_transform)) return refuse("sampling or colour space");
        } else if (m == jpeg::kSOS) {
            if (!W.have_sof || n < 1) return refuse("bad SOS");
            const jpeg::Geometry& G = W.G;
            const uint32_t ns = q[0];
            if (ns < 1 || ns > static_cast<uint32_t>(F.ncomp) || n < 4u + 2u * ns) return refuse("bad SOS");
            ProgScanRec sc;
            std::memset(&sc, 0, sizeof sc);
            uint32_t td[3], ta[3];
            for (uint32_t s = 0; s < ns; ++s) {
                int c = -1;
                for (int k = 0; k < F.ncomp; ++k) if (F.comp_id[k] == q[1 + 2 * s]) c = k;
                if (c < 0) return refuse("scan names an unknown component");
                for (uint32_t e = 0; e < s; ++e) if (sc.comp[e] == c) return refuse("a component twice in one scan");
                sc.comp[s] = static_cast<uint8_t>(c);
                td[s] = q[2 + 2 * s] >> 4; ta[s] = q[2 + 2 * s] & 15;
                if (td[s] > 3 || ta[s] > 3) return refuse("bad SOS");
            }
            const uint32_t Ss = q[1 + 2 * ns], Se = q[2 + 2 * ns], Ah = q[3 + 2 * ns] >> 4, Al = q[3 + 2 * ns] & 15;
            const bool dc_scan = Ss == 0;
            if ((dc_scan && Se != 0) || (!dc_scan && (Se < Ss || Se > 63 || ns != 1)) || Al > 13 || (Ah != 0 && Ah - 1 != Al))
                return refuse("bad progressive scan parameters");
            for (uint32_t s = 0; s < ns; ++s) {                              // jdinput.c latch_quant_tables
                const int c = sc.comp[s];
                if (W.latched[c]) continue;
                if (!T.qt_present[F.tq[c]]) return refuse("missing quantisation table");
                std::memcpy(P.qt[c], T.qt[F.tq[c]], 128);
                W.latched[c] = true;
            }
            // the progression: what this scan may assume of the coefficients it touches, and its level
            int lvl = 0;
            for (uint32_t s = 0; s < ns; ++s) {
                const int c = sc.comp[s];
                if (!dc_scan && W.al[c][0] < 0) return refuse("an AC scan before the component's DC scan");
                for (uint32_t z = Ss; z <= Se; ++z) {
                    if (Ah == 0 ? W.al[c][z] >= 0 : W.al[c][z] != static_cast<int>(Ah)) return refuse("not a well-formed progression");
                    lvl = std::max(lvl, W.level[c][z] + 1);
                }
            }
            for (uint32_t s = 0; s < ns; ++s)
                for (uint32_t z = Ss; z <= Se; ++z) { W.al[sc.comp[s]][z] = static_cast<int8_t>(Al); W.level[sc.comp[s]][z] = lvl; }
            sc.kind = dc_scan ? (Ah ? kProgDcRefine : kProgDcFirst) : (Ah ? kProgAcRefine : kProgAcFirst);
            sc.ns = ns; sc.Ss = Ss; sc.Se = Se; sc.Al = Al;
            // the tables in force: a snapshot (derived once per definition of a slot)
            for (uint32_t s = 0; s < ns && sc.kind != kProgDcRefine; ++s) {
                const int cls = dc_scan ? 0 : 1;
                const uint32_t slot = dc_scan ? td[s] : ta[s];
                const jpeg::HuffSpec& h = dc_scan ? T.dc[slot] : T.ac[slot];
                if (!h.present) return refuse("missing Huffman table");
                if (W.table_at[cls][slot] < 0) {
                    ProgTable t;
                    if (!prog_build_table(h.bits, h.vals, &t)) return refuse("a Huffman table that is no prefix code");
                    W.table_at[cls][slot] = static_cast<int>(P.tables.size());
                    P.tables.push_back(t);
                }
                sc.tab[s] = static_cast<uint32_t>(W.table_at[cls][slot]);
            }
            // the raster (jdinput.c per_scan_setup): one component -> its own real blocks; several -> MCUs
            const bool interleaved = ns > 1;
            uint32_t raster_h;
            if (interleaved) {
                sc.raster_w = G.mcus_w; raster_h = G.mcus_h;
                uint32_t k = 0;
                for (uint32_t s = 0; s < ns; ++s) {
                    const int c = sc.comp[s];
                    sc.nh[s] = F.hs[c]; sc.nv[s] = F.vs[c];
                    for (uint32_t dy = 0; dy < F.vs[c]; ++dy)
                        for (uint32_t dx = 0; dx < F.hs[c]; ++dx, ++k) {
                            if (k >= kProgMaxBlocksInMcu) return refuse("blocks in an MCU");
                            sc.kslot[k] = static_cast<uint8_t>(s); sc.kdx[k] = static_cast<uint8_t>(dx); sc.kdy[k] = static_cast<uint8_t>(dy);
                        }
                }
                sc.bpm = k;
            } else {
                sc.raster_w = G.wb[sc.comp[0]]; raster_h = G.hb[sc.comp[0]];
                sc.nh[0] = sc.nv[0] = 1; sc.bpm = 1;
            }
            const uint64_t total = static_cast<uint64_t>(sc.raster_w) * raster_h;
            const uint32_t ri = T.restart_interval;
            const uint64_t n_intervals = ri ? (total + ri - 1u) / ri : 1u;
            const uint32_t scan_index = static_cast<uint32_t>(P.scans.size());
            uint64_t interval = 0;
            std::vector<uint8_t> cur;
            auto flush = [&]() {
                if (interval < n_intervals) {
                    ProgStreamRec st;
                    st.scan = scan_index;
                    st.n_bits = static_cast<uint32_t>(cur.size() * 8u);
                    st.word0 = P.words.size();
                    st.first_mcu = static_cast<uint32_t>(interval * (ri ? ri : 0u));
                    st.n_mcu = static_cast<uint32_t>(ri ? std::min<uint64_t>(ri, total - interval * ri) : total);
                    for (size_t b = 0; b < cur.size(); b += 4) {
                        uint32_t wv = 0;
                        for (size_t e = 0; e < 4; ++e) wv = (wv << 8) | (b + e < cur.size() ? cur[b + e] : 0u);
                        P.words.push_back(wv);
                    }
                    P.streams.push_back(st);
                }
                ++interval;
                cur.clear();
            };
            size_t at = i;
            for (;;) {
                if (at >= len) break;
                const uint8_t b = d[at];
                if (b != 0xFF) { cur.push_back(b); ++at; continue; }
                size_t r = at + 1;
                while (r < len && d[r] == 0xFF) ++r;                         // fill bytes
                if (r >= len) { at = len; break; }
                if (d[r] == 0x00) { cur.push_back(0xFF); at = r + 1; continue; }
                if (d[r] >= 0xD0 && d[r] <= 0xD7) { flush(); at = r + 1; continue; }
                at = r - 1;                                                  // another marker: the scan ends in front of it
                break;
            }
            flush();
            while (interval < n_intervals) flush();                          // intervals the file does not have: empty streams
            i = at;
            P.scans.push_back(sc);
            P.scan_level.push_back(static_cast<uint32_t>(lvl));
            P.n_levels = std::max(P.n_levels, static_cast<uint32_t>(lvl) + 1u);
        }
    }
    if (!W.have_sof || P.scans.empty()) return refuse("no frame or no scan");
    for (int c = 0; c < F.ncomp; ++c)
        if (!W.latched[c]) return refuse("a component without a scan");
    P.width = F.width; P.height = F.height; P.ncomp = static_cast<uint32_t>(F.ncomp);
    for (int c = 0; c < F.ncomp; ++c) { P.hs[c] = F.hs[c]; P.vs[c] = F.vs[c]; P.bw[c] = W.G.bw[c]; P.bh[c] = W.G.bh[c]; }
    return IFHIP_OK;
}

ProgArgs ProgLayout::args(uint8_t* block, uint32_t* status) const {
    ProgArgs a;
    a.files = reinterpret_cast<const ProgFileRec*>(block + files_off);
    a.scans = reinterpret_cast<const ProgScanRec*>(block + scans_off);
    a.streams = reinterpret_cast<const ProgStreamRec*>(block + streams_off);
    a.tables = reinterpret_cast<const ProgTable*>(block + tables_off);
    a.words = reinterpret_cast<const uint32_t*>(block + words_off);
    a.n_words = n_words;
    a.status = status;
    a.n_files = n_files;
    return a;
}

bool prog_layout_batch(const ProgPrepared* const* files, uint32_t n, void* const* coef, const size_t* plane_bytes, ProgLayout* L) {
    auto pad16 = [](size_t v) { return (v + 15u) & ~static_cast<size_t>(15); };
    size_t n_scans = 0, n_streams = 0, n_tables = 0, n_words = 0;
    uint32_t n_levels = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const ProgPrepared& P = *files[i];
        n_scans += P.scans.size(); n_streams += P.streams.size(); n_tables += P.tables.size(); n_words += P.words.size();
        n_levels = std::max(n_levels, P.n_levels);
    }
    if (n_streams > 0xFFFFFFFFull) return false;
    n_words += kProgSlackWords;
    L->n_files = n; L->n_streams = static_cast<uint32_t>(n_streams); L->n_words = n_words;
    L->files_off = 0;
    L->scans_off = pad16(n * sizeof(ProgFileRec));
    L->streams_off = pad16(L->scans_off + n_scans * sizeof(ProgScanRec));
    L->tables_off = pad16(L->streams_off + n_streams * sizeof(ProgStreamRec));
    L->words_off = pad16(L->tables_off + n_tables * sizeof(ProgTable));
    L->blob.assign(pad16(L->words_off + n_words * 4u), 0);
    L->max_plane_blocks = 0;
    uint8_t* b = L->blob.data();
    ProgFileRec* fr = reinterpret_cast<ProgFileRec*>(b + L->files_off);
    ProgScanRec* sr = reinterpret_cast<ProgScanRec*>(b + L->scans_off);
    ProgStreamRec* tr = reinterpret_cast<ProgStreamRec*>(b + L->streams_off);
    ProgTable* tb = reinterpret_cast<ProgTable*>(b + L->tables_off);
    uint32_t* wd = reinterpret_cast<uint32_t*>(b + L->words_off);
    // streams by level: count, then place in file order
    std::vector<uint32_t> next(n_levels + 1u, 0u);
    for (uint32_t i = 0; i < n; ++i)
        for (const ProgStreamRec& st : files[i]->streams) ++next[files[i]->scan_level[st.scan] + 1u];
    for (uint32_t l = 0; l < n_levels; ++l) next[l + 1u] += next[l];
    L->level_first = next;
    size_t scan_base = 0, table_base = 0, word_base = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const ProgPrepared& P = *files[i];
        ProgFileRec& f = fr[i];
        f.ncomp = P.ncomp;
        for (uint32_t c = 0; c < P.ncomp; ++c) {
            const uint64_t blocks = static_cast<uint64_t>(P.bw[c]) * P.bh[c];
            void* p = coef[3u * i + c];
            if (!p || (reinterpret_cast<uintptr_t>(p) & 7u) || plane_bytes[3u * i + c] < blocks * 128u) return false;
            f.coef[c] = reinterpret_cast<uint64_t>(p);
            f.plane_blocks[c] = blocks;                                      // (what the frame needs of the caller's plane; the rest of it stays untouched)
            f.bw[c] = P.bw[c];
            L->max_plane_blocks = std::max(L->max_plane_blocks, blocks);
        }
        for (size_t s = 0; s < P.scans.size(); ++s) {
            ProgScanRec sc = P.scans[s];
            sc.file = i;
            for (uint32_t t = 0; t < 3; ++t) sc.tab[t] += static_cast<uint32_t>(table_base);
            sr[scan_base + s] = sc;
        }
        for (const ProgStreamRec& st0 : P.streams) {
            ProgStreamRec st = st0;
            const uint32_t l = P.scan_level[st.scan];
            st.scan += static_cast<uint32_t>(scan_base);
            st.word0 += word_base;
            tr[next[l]++] = st;
        }
        if (!P.tables.empty()) std::memcpy(tb + table_base, P.tables.data(), P.tables.size() * sizeof(ProgTable));
        if (!P.words.empty()) std::memcpy(wd + word_base, P.words.data(), P.words.size() * 4u);
        scan_base += P.scans.size(); table_base += P.tables.size(); word_base += P.words.size();
    }
    return true;
}

}  // namespace ifhip
