// vp8_read.cpp -- the host stage of the lossy WebP decoder: a VP8 key frame's header and its bool-coded partitions (RFC 6386
// 9, 13, 19.2-19.3) into the records of csrc/vp8_decode_core.hpp, and the ALPH chunk's header.  Runs on the job's thread, as
// webp_prepare_job does for a lossless file; everything that touches a pixel is the device's (csrc/vp8_decode.hip).
//
// Pinned to libwebp 1.6.0 through Pillow where the RFC leaves a choice:
//   * the colour-space and clamp bits are read and ignored, profiles 0..3 decode alike, the scale bits are ignored;
//   * a partition size beyond the chunk is cut to what is there, the last partition must hold a byte;
//   * the bool reader yields zeros behind the end of a partition and notes the first time it NEEDS a byte from there (it
//     loads a byte when fewer than eight bits are left, not before); that mark is looked at after every row of modes and
//     after every macroblock's tokens, so a stream cut inside its last few bits still decodes;
//   * inner edges are filtered where a macroblock is 4x4-mode or any DEQUANTISED coefficient is non-zero -- for a 16x16-mode
//     macroblock that is asked of the inverse WHT's outputs, not of the Y2 levels.
// Plain C++ (no device header): tests/vp8_decode_emulate.cpp includes this file.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>         // the library compiles every unit as HIP, and the shared headers then want its qualifiers
#endif

#include "vp8_read.hpp"

#include <cstring>

#include "webp_decode_core.hpp"

namespace ifhip {
namespace {

#include "vp8_tables.inc"

struct BoolReader {
    const uint8_t* p = nullptr;
    const uint8_t* end = nullptr;
    uint64_t value = 0;
    uint32_t range = 254;                // the range minus one
    int bits = -8;                       // bits held below the eight in use
    bool eof = false;

    void start(const uint8_t* data, size_t len) { p = data; end = data + len; value = 0; range = 254; bits = -8; eof = false; load(); }
    void load() {
        if (p < end) { value = value << 8 | *p++; bits += 8; }
        else if (!eof) { value <<= 8; bits += 8; eof = true; }
        else bits = 0;
    }
    uint32_t bit(uint32_t prob) {
        if (bits < 0) load();
        const uint32_t split = (range * prob) >> 8;
        const uint64_t v = value >> bits;
        uint32_t r, out;
        if (v > split) { r = range - split; value -= static_cast<uint64_t>(split + 1u) << bits; out = 1u; }
        else { r = split + 1u; out = 0u; }
        const int shift = 7 ^ (31 - __builtin_clz(r));
        r <<= shift;
        bits -= shift;
        range = r - 1u;
        return out;
    }
    uint32_t get(uint32_t n) { uint32_t v = 0; while (n-- > 0u) v |= bit(128) << n; return v; }
    int get_signed(uint32_t n) { const int v = static_cast<int>(get(n)); return get(1) ? -v : v; }
};

int clip(int v, int m) { return v < 0 ? 0 : v > m ? m : v; }

struct Header {
    bool use_segment = false, update_map = false, absolute_delta = true;
    int quantizer[4] = {0, 0, 0, 0}, filter_strength[4] = {0, 0, 0, 0};
    uint8_t segment_prob[3] = {255, 255, 255};
    bool simple = false, use_lf_delta = false;
    int level = 0, sharpness = 0, ref_lf_delta[4] = {0, 0, 0, 0}, mode_lf_delta[4] = {0, 0, 0, 0};
    bool use_skip = false;
    uint8_t skip_p = 0;
    uint8_t coeff[4][8][3][11];
};
struct Strength { uint8_t limit, ilevel, hev; };

int large_value(BoolReader& br, const uint8_t* p) {
    if (!br.bit(p[3])) return !br.bit(p[4]) ? 2 : 3 + static_cast<int>(br.bit(p[5]));
    if (!br.bit(p[6])) {
        if (!br.bit(p[7])) return 5 + static_cast<int>(br.bit(159));
        int v = 7 + 2 * static_cast<int>(br.bit(165));
        return v + static_cast<int>(br.bit(145));
    }
    const uint32_t bit1 = br.bit(p[8]), bit0 = br.bit(p[9u + bit1]), cat = 2u * bit1 + bit0;
    static const uint8_t* const cats[4] = {kVp8Cat3, kVp8Cat4, kVp8Cat5, kVp8Cat6};
    int v = 0;
    for (const uint8_t* tab = cats[cat]; *tab; ++tab) v += v + static_cast<int>(br.bit(*tab));
    return v + 3 + (8 << cat);
}
// One block's tokens from coefficient n on: levels at their raster positions; returns the position behind the last non-zero one.
int coefficients(BoolReader& br, const uint8_t (*prob)[3][11], uint32_t ctx, int n, int16_t* out) {
    const uint8_t* p = prob[kVp8Bands[n]][ctx];
    for (; n < 16; ++n) {
        if (!br.bit(p[0])) return n;
        while (!br.bit(p[1])) {
            p = prob[kVp8Bands[++n]][0];
            if (n == 16) return 16;
        }
        const uint8_t (*next)[11] = prob[kVp8Bands[n + 1]];
        int v;
        if (!br.bit(p[2])) { v = 1; p = next[1]; }
        else { v = large_value(br, p); p = next[2]; }
        out[kVp8Zigzag[n]] = static_cast<int16_t>(br.bit(128) ? -v : v);
    }
    return 16;
}

}  // namespace

uint32_t vp8_read_frame(const uint8_t* d, size_t len, Vp8Frame* out) {
    Vp8Frame& F = *out;
    auto fail = [&](uint32_t st) { F.status = st; F.mbs.clear(); F.levels.clear(); return st; };
    if (len < 10u) return fail(kVp8DecFrameHeader);
    const uint32_t tag = d[0] | static_cast<uint32_t>(d[1]) << 8 | static_cast<uint32_t>(d[2]) << 16;
    const uint32_t first_len = tag >> 5;
    if ((tag & 1u) || ((tag >> 1) & 7u) > 3u || !((tag >> 4) & 1u)) return fail(kVp8DecFrameHeader);   // no key frame, profile, not shown
    if (d[3] != 0x9Du || d[4] != 0x01u || d[5] != 0x2Au) return fail(kVp8DecFrameHeader);
    F.w = (d[6] | static_cast<uint32_t>(d[7]) << 8) & 0x3FFFu;
    F.h = (d[8] | static_cast<uint32_t>(d[9]) << 8) & 0x3FFFu;
    if (!F.w || !F.h) return fail(kVp8DecFrameHeader);
    if (first_len >= len || first_len > len - 10u) return fail(kVp8DecPartitions);
    F.mbw = (F.w + 15u) >> 4; F.mbh = (F.h + 15u) >> 4;

    BoolReader br;
    br.start(d + 10, first_len);
    Header H;
    br.get(1); br.get(1);                                                 // colour space, clamp type
    H.use_segment = br.get(1) != 0u;
    if (H.use_segment) {
        H.update_map = br.get(1) != 0u;
        if (br.get(1)) {
            H.absolute_delta = br.get(1) != 0u;
            for (int s = 0; s < 4; ++s) H.quantizer[s] = br.get(1) ? br.get_signed(7) : 0;
            for (int s = 0; s < 4; ++s) H.filter_strength[s] = br.get(1) ? br.get_signed(6) : 0;
        }
        if (H.update_map) for (int s = 0; s < 3; ++s) H.segment_prob[s] = br.get(1) ? static_cast<uint8_t>(br.get(8)) : 255u;
    }
    if (br.eof) return fail(kVp8DecFrameHeader);
    H.simple = br.get(1) != 0u;
    H.level = static_cast<int>(br.get(6));
    H.sharpness = static_cast<int>(br.get(3));
    H.use_lf_delta = br.get(1) != 0u;
    if (H.use_lf_delta && br.get(1)) {
        for (int i = 0; i < 4; ++i) if (br.get(1)) H.ref_lf_delta[i] = br.get_signed(6);
        for (int i = 0; i < 4; ++i) if (br.get(1)) H.mode_lf_delta[i] = br.get_signed(6);
    }
    if (br.eof) return fail(kVp8DecFrameHeader);
    F.filter = H.level == 0 ? kVp8FilterNone : H.simple ? kVp8FilterSimple : kVp8FilterNormal;

    // the token partitions behind the first one: a table of 24-bit sizes, the last partition takes the rest
    const uint8_t* buf = d + 10 + first_len;
    const uint8_t* const buf_end = d + len;
    const uint32_t n_parts = 1u << br.get(2);
    size_t size_left = static_cast<size_t>(buf_end - buf);
    if (size_left < 3u * (n_parts - 1u)) return fail(kVp8DecPartitions);
    BoolReader parts[8];
    const uint8_t* part = buf + 3u * (n_parts - 1u);
    size_left -= 3u * (n_parts - 1u);
    for (uint32_t p = 0; p + 1u < n_parts; ++p) {
        size_t psize = buf[3u * p] | static_cast<size_t>(buf[3u * p + 1u]) << 8 | static_cast<size_t>(buf[3u * p + 2u]) << 16;
        if (psize > size_left) psize = size_left;
        parts[p].start(part, psize);
        part += psize; size_left -= psize;
    }
    if (part >= buf_end) return fail(kVp8DecPartitions);
    parts[n_parts - 1u].start(part, size_left);

    // quantisers
    const int base_q0 = static_cast<int>(br.get(7));
    const int dqy1_dc = br.get(1) ? br.get_signed(4) : 0, dqy2_dc = br.get(1) ? br.get_signed(4) : 0, dqy2_ac = br.get(1) ? br.get_signed(4) : 0;
    const int dquv_dc = br.get(1) ? br.get_signed(4) : 0, dquv_ac = br.get(1) ? br.get_signed(4) : 0;
    for (int s = 0; s < 4; ++s) {
        int q;
        if (H.use_segment) q = H.quantizer[s] + (H.absolute_delta ? 0 : base_q0);
        else if (s > 0) { F.quant[s] = F.quant[0]; continue; }
        else q = base_q0;
        Vp8Quant& Q = F.quant[s];
        Q.y1[0] = kVp8DcTable[clip(q + dqy1_dc, 127)];
        Q.y1[1] = kVp8AcTable[clip(q, 127)];
        Q.y2[0] = static_cast<uint16_t>(kVp8DcTable[clip(q + dqy2_dc, 127)] * 2);
        Q.y2[1] = static_cast<uint16_t>((kVp8AcTable[clip(q + dqy2_ac, 127)] * 101581) >> 16);
        if (Q.y2[1] < 8u) Q.y2[1] = 8u;
        Q.uv[0] = kVp8DcTable[clip(q + dquv_dc, 117)];
        Q.uv[1] = kVp8AcTable[clip(q + dquv_ac, 127)];
    }
    br.get(1);                                                            // refresh entropy probabilities: nothing follows a key frame here
    for (int t = 0; t < 4; ++t)
        for (int b = 0; b < 8; ++b)
            for (int c = 0; c < 3; ++c)
                for (int p = 0; p < 11; ++p)
                    H.coeff[t][b][c][p] = br.bit(kVp8CoeffUpdateProba[t][b][c][p]) ? static_cast<uint8_t>(br.get(8)) : kVp8CoeffProba0[t][b][c][p];
    H.use_skip = br.get(1) != 0u;
    if (H.use_skip) H.skip_p = static_cast<uint8_t>(br.get(8));

    // filter strengths per segment and kind of macroblock (libwebp's PrecomputeFilterStrengths)
    Strength strength[4][2];
    std::memset(strength, 0, sizeof strength);
    if (F.filter != kVp8FilterNone)
        for (int s = 0; s < 4; ++s) {
            int base = H.level;
            if (H.use_segment) { base = H.filter_strength[s]; if (!H.absolute_delta) base += H.level; }
            for (int i4 = 0; i4 < 2; ++i4) {
                int level = base;
                if (H.use_lf_delta) { level += H.ref_lf_delta[0]; if (i4) level += H.mode_lf_delta[0]; }
                level = clip(level, 63);
                if (level == 0) continue;
                int ilevel = level;
                if (H.sharpness > 0) {
                    ilevel >>= H.sharpness > 4 ? 2 : 1;
                    if (ilevel > 9 - H.sharpness) ilevel = 9 - H.sharpness;
                }
                if (ilevel < 1) ilevel = 1;
                strength[s][i4] = {static_cast<uint8_t>(2 * level + ilevel), static_cast<uint8_t>(ilevel), static_cast<uint8_t>(level >= 40 ? 2 : level >= 15 ? 1 : 0)};
            }
        }

    // the first partition: segment, skip flag and modes of every macroblock, a row at a time
    const size_t n_mb = static_cast<size_t>(F.mbw) * F.mbh;
    F.mbs.assign(n_mb, Vp8Mb());
    std::vector<uint8_t> intra_t(4u * F.mbw, 0u), skips(n_mb, 0u);
    for (uint32_t my = 0; my < F.mbh; ++my) {
        uint8_t left[4] = {0, 0, 0, 0};
        for (uint32_t mx = 0; mx < F.mbw; ++mx) {
            Vp8Mb& mb = F.mbs[static_cast<size_t>(my) * F.mbw + mx];
            std::memset(&mb, 0, sizeof mb);
            uint8_t* top = intra_t.data() + 4u * mx;
            if (H.update_map) mb.segment = static_cast<uint8_t>(!br.bit(H.segment_prob[0]) ? br.bit(H.segment_prob[1]) : br.bit(H.segment_prob[2]) + 2u);
            if (H.use_skip) skips[static_cast<size_t>(my) * F.mbw + mx] = static_cast<uint8_t>(br.bit(H.skip_p));
            if (br.bit(145)) {
                const uint8_t ymode = static_cast<uint8_t>(br.bit(156) ? (br.bit(128) ? 1u : 3u) : (br.bit(163) ? 2u : 0u));
                mb.ymode = ymode;
                std::memset(top, ymode, 4); std::memset(left, ymode, 4);
            } else {
                mb.ymode = static_cast<uint8_t>(kVp8ModeB);
                for (int y = 0; y < 4; ++y) {
                    int ymode = left[y];
                    for (int x = 0; x < 4; ++x) {
                        const uint8_t* prob = kVp8BModesProba[top[x]][ymode];
                        int i = kVp8BModeTree[br.bit(prob[0])];
                        while (i > 0) i = kVp8BModeTree[2 * i + static_cast<int>(br.bit(prob[i]))];
                        ymode = -i;
                        top[x] = static_cast<uint8_t>(ymode);
                        mb.imodes[4 * y + x] = static_cast<uint8_t>(ymode);
                    }
                    left[y] = static_cast<uint8_t>(ymode);
                }
            }
            mb.uvmode = static_cast<uint8_t>(!br.bit(142) ? 0u : !br.bit(114) ? 2u : br.bit(183) ? 1u : 3u);
        }
        if (br.eof) return fail(kVp8DecEndOfModes);
    }

    // the token partitions: row r in partition r mod N
    F.levels.assign(n_mb * kVp8MbLevels, 0);
    std::vector<uint8_t> top_nz(F.mbw, 0u), top_dc(F.mbw, 0u);
    for (uint32_t my = 0; my < F.mbh; ++my) {
        BoolReader& tr = parts[my & (n_parts - 1u)];
        uint32_t left_nz = 0, left_dc = 0;
        for (uint32_t mx = 0; mx < F.mbw; ++mx) {
            const size_t at = static_cast<size_t>(my) * F.mbw + mx;
            Vp8Mb& mb = F.mbs[at];
            int16_t* lv = F.levels.data() + at * kVp8MbLevels;
            const bool i4 = mb.ymode == kVp8ModeB;
            const Vp8Quant& Q = F.quant[mb.segment];
            bool coded = false;                                           // any dequantised coefficient is non-zero
            if (skips[at]) {
                top_nz[mx] = 0; left_nz = 0;
                if (!i4) { top_dc[mx] = 0; left_dc = 0; }
            } else {
                const uint8_t (*ac)[3][11] = H.coeff[3];
                int first = 0;
                if (!i4) {
                    const int nz = coefficients(tr, H.coeff[1], top_dc[mx] + left_dc, 0, lv + 16 * 24);
                    top_dc[mx] = static_cast<uint8_t>(nz > 0); left_dc = nz > 0 ? 1u : 0u;
                    if (nz > 0) mb.nz |= 1u << 24;
                    if (nz > 0)
                        for (uint32_t b = 0; b < 16u && !coded; ++b) coded = vp8_wht_one(lv + 16 * 24, Q.y2[0], Q.y2[1], b) != 0;
                    first = 1;
                    ac = H.coeff[0];
                }
                uint32_t tnz = top_nz[mx] & 0x0Fu, lnz = left_nz & 0x0Fu;
                for (uint32_t y = 0; y < 4u; ++y) {
                    uint32_t l = lnz & 1u;
                    for (uint32_t x = 0; x < 4u; ++x) {
                        const uint32_t b = 4u * y + x;
                        const int nz = coefficients(tr, ac, l + (tnz & 1u), first, lv + 16u * b);
                        l = nz > first ? 1u : 0u;
                        tnz = (tnz >> 1) | (l << 7);
                        if (l) mb.nz |= 1u << b;
                        if (nz <= 1) mb.dc_only |= 1u << b; else if (nz <= 3) mb.ac3 |= 1u << b;
                        if (nz > 1 || (nz == 1 && !first && static_cast<int16_t>(lv[16u * b] * Q.y1[0]) != 0)) coded = true;
                    }
                    tnz >>= 4;
                    lnz = (lnz >> 1) | (l << 7);
                }
                uint32_t out_t = tnz, out_l = lnz >> 4;
                for (uint32_t ch = 0; ch < 4u; ch += 2u) {
                    tnz = top_nz[mx] >> (4u + ch); lnz = left_nz >> (4u + ch);
                    bool plane_full = false;                              // a second level anywhere in the plane: the full transform for its four blocks
                    for (uint32_t y = 0; y < 2u; ++y) {
                        uint32_t l = lnz & 1u;
                        for (uint32_t x = 0; x < 2u; ++x) {
                            const uint32_t b = 16u + 2u * ch + 2u * y + x;
                            const int nz = coefficients(tr, H.coeff[2], l + (tnz & 1u), 0, lv + 16u * b);
                            l = nz > 0 ? 1u : 0u;
                            tnz = (tnz >> 1) | (l << 3);
                            if (l) mb.nz |= 1u << b;
                            if (nz > 1) plane_full = true;
                            if (nz > 1 || (nz == 1 && static_cast<int16_t>(lv[16u * b] * Q.uv[0]) != 0)) coded = true;
                        }
                        tnz >>= 2;
                        lnz = (lnz >> 1) | (l << 5);
                    }
                    if (!plane_full) mb.dc_only |= 0xFu << (16u + 2u * ch);
                    out_t |= (tnz << 4) << ch;
                    out_l |= (lnz & 0xF0u) << ch;
                }
                top_nz[mx] = static_cast<uint8_t>(out_t); left_nz = out_l & 0xFFu;
            }
            const Strength& S = strength[mb.segment][i4 ? 1 : 0];
            mb.limit = S.limit; mb.ilevel = S.ilevel; mb.hev = S.hev;
            mb.inner = static_cast<uint8_t>(i4 || coded);
            if (tr.eof) return fail(kVp8DecEndOfTokens);
        }
    }
    F.status = kVp8DecOk;
    return kVp8DecOk;
}

uint32_t vp8_read_alpha(const uint8_t* alph, size_t len, Vp8Frame* out) {
    Vp8Frame& F = *out;
    auto fail = [&](uint32_t st) { if (!F.status) F.status = st; return st; };
    if (len < 1u) return fail(kVp8DecAlphaHeader);
    const uint32_t method = alph[0] & 3u, filter = (alph[0] >> 2) & 3u, pre = (alph[0] >> 4) & 3u, reserved = alph[0] >> 6;
    if (method > 1u || pre > 1u || reserved != 0u) return fail(kVp8DecAlphaHeader);
    F.alpha_filter = filter;
    F.alpha_data = alph + 1; F.alpha_len = len - 1u;
    if (method == 0u) {
        if (F.alpha_len < static_cast<size_t>(F.w) * F.h) return fail(kVp8DecAlphaStream);
        F.alpha_kind = kVp8AlphaRaw;
        return kVp8DecOk;
    }
    if (F.alpha_len > 0x7FFF0000u) return fail(kVp8DecAlphaStream);
    F.alpha_kind = kVp8AlphaVp8l;
    F.alpha_prepared = std::make_shared<WebpPrepared>();
    WebpPrepared& P = *F.alpha_prepared;
    const uint32_t n = static_cast<uint32_t>(F.alpha_len);
    P.payload.assign((static_cast<size_t>(n) + 15u) / 16u + 1u, WebpQuad{0u, 0u, 0u, 0u});
    std::memcpy(P.payload.data(), F.alpha_data, n);
    WebpHeadReader reader(reinterpret_cast<const uint8_t*>(P.payload.data()), n);
    F.alpha_vp8l_status = reader.prepare_headless(F.w, F.h, &P);
    if (F.alpha_vp8l_status) return fail(kVp8DecAlphaStream);
    return kVp8DecOk;
}

const char* vp8_status_text(uint32_t s) {
    switch (s) {
    case kVp8DecNotLossy: return "UNSUPPORTED_FEATURE (not a lossy WebP)";
    case kVp8DecFrameHeader: return "BITSTREAM_ERROR (the VP8 frame header: no shown key frame of profile 0..3 with its start code)";
    case kVp8DecPartitions: return "NOT_ENOUGH_DATA (a VP8 partition reaches beyond the chunk)";
    case kVp8DecEndOfModes: return "NOT_ENOUGH_DATA (premature end of the first VP8 partition)";
    case kVp8DecEndOfTokens: return "NOT_ENOUGH_DATA (premature end of a VP8 token partition)";
    case kVp8DecAlphaHeader: return "BITSTREAM_ERROR (the ALPH chunk's header)";
    case kVp8DecAlphaStream: return "BITSTREAM_ERROR (the ALPH chunk's stream)";
    default: return "BITSTREAM_ERROR (the container did not parse)";
    }
}

}  // namespace ifhip
