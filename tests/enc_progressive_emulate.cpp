// enc_progressive_emulate.cpp -- test infrastructure, not part of the product: the passes of the device entropy coder's
// optimised-table and progressive forms (csrc/jpeg_encode_progressive.hip) run pass by pass and lane by lane on the CPU
// with the SAME routines (csrc/jpeg_encode_progressive_core.hpp): statistics and flags per item, the run walk wave by wave
// (64 lanes as arrays), jpeg_gen_optimal_table with its lane-parallel minimum searches, bit counts, the per-scan prefix
// sums, the write pass in a scrambled order with the word stream's ownership rule checked, 0xFF counts, stuffing and the
// placement of every segment.  Also returns how many runs were cut at 0x7FFF blocks and how many by the correction-bit
// bound.  Built by tests/test_jpeg_device_coder_progressive.py with g++.
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "../imageflow_amd/csrc/jpeg_encode_progressive_core.hpp"

using namespace ifhip;

namespace {
uint32_t* g_words = nullptr;
std::vector<uint8_t>* g_mark = nullptr;      // 1: stored plainly (owned), 2: ORed (shared)
int g_violations = 0;

struct HostStore {
    static void shared(uint32_t* p, uint32_t v) {
        uint8_t& m = (*g_mark)[static_cast<size_t>(p - g_words)];
        if (m == 1) ++g_violations;
        m = 2;
        *p |= v;
    }
    static void owned(uint32_t* p, uint32_t v) {
        uint8_t& m = (*g_mark)[static_cast<size_t>(p - g_words)];
        if (m != 0 || *p != 0) ++g_violations;
        m = 1;
        *p = v;
    }
};
struct HostAdd { static void add(uint32_t* p, uint32_t v) { *p += v; } };

struct PlaneCoef {                            // a block of the plane (natural order) seen as the kernels stage it
    const int16_t* b;
    int32_t operator()(int k) const { return b[enc_zigzag(k)]; }
    uint32_t pair(int j) const {
        const uint16_t lo = static_cast<uint16_t>(b[enc_zigzag(static_cast<int>(enc_position_of_slot(2u * j)))]);
        const uint16_t hi = static_cast<uint16_t>(b[enc_zigzag(static_cast<int>(enc_position_of_slot(2u * j + 1u)))]);
        return static_cast<uint32_t>(lo) | static_cast<uint32_t>(hi) << 16;
    }
};

template <class Out>
uint32_t item(const ProgScan& sc, const PlaneCoef& coef, int32_t pred, uint32_t eobrun, Out& out) {
    if (sc.kind == kProgDcFirst) return prog_dc_first(coef(0), pred, sc.Al, out);
    if (sc.kind == kProgDcRefine) { out.raw(static_cast<uint32_t>(coef(0) >> sc.Al) & 1u, 1u); return 0u; }
    if (sc.kind == kProgAcFirst) return prog_ac_first(coef, sc.Ss, sc.Se, sc.Al, eobrun, out);
    return prog_ac_refine(coef, sc.Ss, sc.Se, sc.Al, eobrun, out);
}

struct HostWave {                             // 64 lanes as arrays
    const uint16_t* flags;
    uint16_t* eob;
    uint32_t* hist;                           // the scan's AC histogram
    int* cuts;                                // [2]
    uint32_t tail[64], pb[64], prev = 0;
    uint64_t H = 0, T = 0;
    void load(uint32_t base, uint32_t nv) {
        H = T = 0;
        uint32_t sum = 0;
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t f = l < nv ? flags[base + l] : 0u;
            tail[l] = (f >> 1) & 1u;
            H |= static_cast<uint64_t>(f & 1u) << l;
            T |= static_cast<uint64_t>(tail[l]) << l;
            sum += tail[l] ? prog_ncorr(f) : 0u;
            pb[l] = sum;
        }
        prev = base ? (flags[base - 1u] >> 1) & 1u : 0u;
    }
    uint64_t heads() const { return H; }
    uint64_t tails() const { return T; }
    bool prev_tail() const { return prev != 0u; }
    uint32_t incl_bits(uint32_t l) const { return pb[l]; }
    uint64_t crossing(uint32_t q, uint32_t h, uint32_t len0, uint32_t bits0, uint32_t ptq, uint32_t pbq) const {
        uint64_t m = 0;
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t pt = static_cast<uint32_t>(__builtin_popcountll(T & prog_below(l + 1u)));
            if (prog_run_crosses(l, q, h, tail[l] != 0u, pt, pb[l], ptq, pbq, len0, bits0)) m |= 1ull << l;
        }
        return m;
    }
    void emit(uint32_t start, uint32_t len, uint32_t by) {
        if (eob[start] != 0) ++g_violations;              // a run's first block is written once
        eob[start] = static_cast<uint16_t>(len);
        hist[(31u - static_cast<uint32_t>(__builtin_clz(len))) << 4]++;
        if (by < 2u) cuts[by]++;
    }
};
}  // namespace

extern "C" int enc_progressive_emulate(const int16_t* c0, const int16_t* c1, const int16_t* c2, uint32_t width, uint32_t height, int ncomp,
                                       const uint8_t* hs, const uint8_t* vs, const uint32_t* bw, const uint32_t* bh, const uint8_t* header,
                                       uint32_t header_len, int flags, uint8_t* out, size_t capacity, size_t* len, uint32_t* status,
                                       int* violations, int* cuts) {
    EncGeom g;
    if (enc_make_geom(width, height, ncomp, hs, vs, bw, bh, &g)) return 1;
    ProgPlan P;
    prog_make_plan(g, width, height, flags, &P);
    if (header_len < P.header0_len) return 2;
    const int16_t* planes[3] = {c0, c1, c2};
    cuts[0] = cuts[1] = 0;
    g_violations = 0;
    auto ref = [&](const ProgScan& sc, uint32_t s) { return prog_locate(g, sc, s); };
    auto block = [&](const EncBlockRef& r) { return PlaneCoef{planes[r.comp] + static_cast<size_t>(r.offset) * 64u}; };
    auto pred_of = [&](const EncBlockRef& r) -> int32_t { return r.pred_offset == 0xFFFFFFFFu ? 0 : planes[r.comp][static_cast<size_t>(r.pred_offset) * 64u]; };
    std::vector<uint16_t> fl(P.n_items, 0), eob(P.n_items, 0), nbits(P.n_items, 0);
    std::vector<uint32_t> hist(kProgMaxSlots * 256u, 0), codes(kProgMaxSlots * 256u, 0), dht_len(kProgMaxSlots, 0);
    std::vector<uint8_t> dht(kProgMaxSlots * kProgDhtPitch, 0);
    uint32_t ident[256];
    for (uint32_t i = 0; i < 256u; ++i) ident[i] = i;
    auto slot_tab = [&](std::vector<uint32_t>& v, const ProgScan& sc, uint32_t comp, bool ac) -> uint32_t* {
        const uint32_t slot = sc.slot[(comp ? 2u : 0u) + (ac ? 1u : 0u)];
        return slot == kProgNoSlot ? nullptr : v.data() + slot * 256u;
    };
    // pass A: statistics + flags
    for (uint32_t j = 0; j < P.nscans; ++j) {
        const ProgScan& sc = P.scan[j];
        if (sc.kind == kProgDcRefine) continue;
        for (uint32_t s = 0; s < sc.nblocks; ++s) {
            const EncBlockRef r = ref(sc, s);
            if (sc.kind == kProgSeq) {
                EncStatSink<HostAdd> sink{slot_tab(hist, sc, r.comp, false), slot_tab(hist, sc, r.comp, true)};
                enc_block(block(r), pred_of(r), ident, ident, sink);
            } else {
                ProgCounted<HostAdd> o{slot_tab(hist, sc, r.comp, sc.kind >= kProgAcFirst)};
                const uint32_t f = item(sc, block(r), pred_of(r), 0u, o);
                if (sc.kind >= kProgAcFirst) fl[sc.item0 + s] = static_cast<uint16_t>(f);
            }
        }
    }
    // run pass: one wave per chunk, the chunks in reverse order (any order must do)
    for (uint32_t j = 0; j < P.nscans; ++j) {
        const ProgScan& sc = P.scan[j];
        if (sc.kind < kProgAcFirst) continue;
        const uint32_t nchunks = (sc.nblocks + kProgRunChunk - 1u) / kProgRunChunk;
        for (uint32_t c = nchunks; c-- > 0u;) {
            HostWave w{fl.data() + sc.item0, eob.data() + sc.item0, slot_tab(hist, sc, sc.comp, true), cuts};
            prog_run_chunk(w, c * kProgRunChunk, std::min(sc.nblocks, (c + 1u) * kProgRunChunk), sc.nblocks);
        }
    }
    // tables: one wave per slot
    for (uint32_t slot = 0; slot < P.nslots; ++slot) {
        uint32_t freq[257], codesize[257], bits[33];
        int32_t others[257];
        uint8_t vals[256] = {0};
        for (uint32_t lane = 0; lane < 64u; ++lane) huff_init(hist.data() + slot * 256u, lane, freq, codesize, others);
        for (;;) {
            uint64_t k1 = ~0ull, k2 = ~0ull;
            for (uint32_t lane = 0; lane < 64u; ++lane) k1 = std::min(k1, huff_lane_key(freq, lane, 0xFFFFFFFFu));
            const uint32_t a = huff_key_index(k1);
            for (uint32_t lane = 0; lane < 64u; ++lane) k2 = std::min(k2, huff_lane_key(freq, lane, a));
            if (k2 == ~0ull) break;
            huff_merge(a, huff_key_index(k2), freq, codesize, others);
        }
        huff_limit(codesize, bits);
        for (uint32_t i = 0; i < 256u; ++i) if (codesize[i] && codesize[i] <= 32u) vals[huff_rank(codesize, i)] = static_cast<uint8_t>(i);
        dht_len[slot] = huff_emit(bits, vals, P.slot_id[slot], dht.data() + slot * kProgDhtPitch, codes.data() + slot * 256u);
    }
    // count pass + per-workgroup sums, then the per-scan prefix sums
    std::vector<uint32_t> wg(P.n_wg, 0);
    uint32_t st = 0;
    auto code_item = [&](const ProgScan& sc, uint32_t s, auto& sink) -> uint32_t {
        const EncBlockRef r = ref(sc, s);
        if (sc.kind == kProgSeq) return enc_block(block(r), pred_of(r), slot_tab(codes, sc, r.comp, false), slot_tab(codes, sc, r.comp, true), sink);
        ProgCoded<std::remove_reference_t<decltype(sink)>> o{sink, slot_tab(codes, sc, r.comp, sc.kind >= kProgAcFirst)};
        return item(sc, block(r), pred_of(r), sc.kind >= kProgAcFirst ? eob[sc.item0 + s] : 0u, o) & kProgBad;
    };
    for (uint32_t j = 0; j < P.nscans; ++j) {
        const ProgScan& sc = P.scan[j];
        for (uint32_t s = 0; s < sc.nblocks; ++s) {
            EncCountSink sink;
            if (code_item(sc, s, sink)) st |= kEncBadCoef;
            nbits[sc.item0 + s] = static_cast<uint16_t>(sink.bits);
            wg[sc.wg0 + s / kEncBlocksPerWg] += sink.bits;
        }
    }
    std::vector<uint32_t> bytes(P.nscans), chunk0(P.nscans + 1u), data_off(P.nscans);
    uint32_t chunk_at = 0;
    for (uint32_t j = 0; j < P.nscans; ++j) {
        const ProgScan& sc = P.scan[j];
        const uint32_t n = (sc.nblocks + kEncBlocksPerWg - 1u) / kEncBlocksPerWg;
        uint32_t carry = 0;
        for (uint32_t i = 0; i < n; ++i) { const uint32_t v = wg[sc.wg0 + i]; wg[sc.wg0 + i] = carry; carry += v; }
        bytes[j] = (carry + 7u) >> 3;
        chunk0[j] = chunk_at;
        chunk_at += (bytes[j] + kEncChunkBytes - 1u) / kEncChunkBytes;
    }
    chunk0[P.nscans] = chunk_at;
    *status = st;
    *violations = g_violations;
    if (st) { *len = 0; return 0; }
    std::vector<uint32_t> words(static_cast<size_t>(chunk_at + 1u) * kEncChunkBytes / 4u, 0u);
    std::vector<uint8_t> mark(words.size(), 0);
    g_words = words.data(); g_mark = &mark;
    // write pass: workgroups and the items inside each in a scrambled order
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto scramble = [&](std::vector<uint32_t>& v) {
        for (size_t i = v.size(); i > 1; --i) {
            rng = rng * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(v[i - 1], v[static_cast<size_t>((rng >> 33) % i)]);
        }
    };
    std::vector<uint32_t> wgs(P.n_wg);
    for (uint32_t i = 0; i < P.n_wg; ++i) wgs[i] = i;
    scramble(wgs);
    for (uint32_t w : wgs) {
        uint32_t j = 0;
        while (j + 1u < P.nscans && w >= P.scan[j + 1u].wg0) ++j;
        const ProgScan& sc = P.scan[j];
        const uint32_t s0 = (w - sc.wg0) * kEncBlocksPerWg, s1 = std::min(sc.nblocks, s0 + kEncBlocksPerWg);
        std::vector<uint32_t> order(s1 - s0);
        for (uint32_t i = 0; i < s1 - s0; ++i) order[i] = s0 + i;
        scramble(order);
        for (uint32_t s : order) {
            uint32_t off = chunk0[j] * kEncChunkBytes * 8u + wg[w];
            for (uint32_t q = s0; q < s; ++q) off += nbits[sc.item0 + q];
            EncWordSink<HostStore> sink(words.data(), off);
            code_item(sc, s, sink);
            if (s == sc.nblocks - 1u) {
                const uint32_t pad = (8u - sink.bits_in_last_byte()) & 7u;
                if (pad) sink.put((1u << pad) - 1u, pad);
            }
            sink.finish();
        }
    }
    *violations = g_violations;
    // 0xFF counts per chunk, scan, segment offsets
    std::vector<uint32_t> ff(chunk_at, 0);
    for (uint32_t c = 0; c < chunk_at; ++c) {
        uint32_t j = 0;
        while (j + 1u < P.nscans && c >= chunk0[j + 1u]) ++j;
        for (uint32_t at = (c - chunk0[j]) * kEncChunkBytes; at < (c - chunk0[j] + 1u) * kEncChunkBytes && at < bytes[j]; at += 4u)
            ff[c] += enc_count_ff(words[(static_cast<size_t>(chunk0[j]) * kEncChunkBytes + at) >> 2]);
    }
    uint32_t tot_ff = 0;
    for (uint32_t c = 0; c < chunk_at; ++c) { const uint32_t v = ff[c]; ff[c] = tot_ff; tot_ff += v; }
    size_t off = P.header0_len;
    for (uint32_t j = 0; j < P.nscans; ++j) {
        const ProgScan& sc = P.scan[j];
        for (uint32_t i = 0; i < sc.ndht; ++i) off += dht_len[sc.dht[i]];
        off += sc.sos_len;
        data_off[j] = static_cast<uint32_t>(off);
        off += bytes[j] + ((j + 1u < P.nscans ? ff[chunk0[j + 1u]] : tot_ff) - ff[chunk0[j]]);
    }
    const size_t file_len = off + 2u;
    *len = file_len;
    if (file_len > capacity) { *status = kEncFileOverflow; *len = 0; return 0; }
    std::memcpy(out, header, P.header0_len);
    if (P.progressive) out[P.sof_marker_at] = 0xC2;
    const uint8_t* stream = reinterpret_cast<const uint8_t*>(words.data());
    for (uint32_t j = 0; j < P.nscans; ++j) {
        const ProgScan& sc = P.scan[j];
        uint32_t at = data_off[j] - sc.sos_len;
        std::memcpy(out + at, sc.sos, sc.sos_len);
        for (uint32_t k = sc.ndht; k-- > 0u;) {
            at -= dht_len[sc.dht[k]];
            std::memcpy(out + at, dht.data() + sc.dht[k] * kProgDhtPitch, dht_len[sc.dht[k]]);
        }
        for (uint32_t c = chunk0[j]; c < chunk0[j + 1u]; ++c) {
            const uint32_t rel = c - chunk0[j];
            uint32_t lane_ff = 0;
            for (uint32_t a = rel * kEncChunkBytes; a < (rel + 1u) * kEncChunkBytes && a < bytes[j]; a += 16u) {
                uint8_t* d = out + data_off[j] + a + (ff[c] - ff[chunk0[j]]) + lane_ff;
                for (uint32_t q = 0; q < 16u && a + q < bytes[j]; ++q) {
                    const uint8_t b = stream[static_cast<size_t>(chunk0[j]) * kEncChunkBytes + a + q];
                    *d++ = b;
                    if (b == 255u) { *d++ = 0; ++lane_ff; }
                }
            }
        }
    }
    out[file_len - 2u] = 0xFF; out[file_len - 1u] = 0xD9;
    return 0;
}
