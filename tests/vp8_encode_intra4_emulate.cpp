// vp8_encode_intra4_emulate.cpp -- the device lossy WebP coder of a stage with flags on the CPU: the passes of csrc/vp8_encode.hip
// with vp8e_code4_kernel of csrc/vp8_encode_intra4.hip in the code kernel's place where IFHIP_VP8_ENC_INTRA4 is set (skew 2,
// vp8e_code_mb4), from the same core header.  With flags 0 it is tests/vp8_encode_emulate.cpp's schedule and must give its bytes.
// Besides the file it writes the BGRA it expects a decoder to produce.  tests/test_vp8_encode_intra4_core.py builds it with
// g++ as a library and -- with -DVP8_ENC4_EMU_MAIN -- as a stand-alone program for the sanitizers.
//
// A test-only switch, bit 8 of `flags` (kNaiveY2): the Y2 contexts are taken from the neighbouring macroblock's own bit 24, as
// they could be while every macroblock had a Y2 block, instead of from the two chains (vp8e_ctx_left / vp8e_ctx_above).  Such a
// file is wrong wherever a B_PRED macroblock lies between two 16x16 ones; the test shows that the streams differ.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../imageflow_amd/csrc/vp8_encode_core.hpp"
#include "webp_emulate.cpp"

using namespace ifhip;

constexpr uint32_t kNaiveY2 = 1u << 8;

extern "C" {

uint64_t vp8e4_emu_max_file_bytes(uint32_t w, uint32_t h, int alpha, uint32_t flags) { return vp8e_max_file_bytes(w, h, alpha ? webp_max_file_bytes(w, h) : 0u, flags & kVp8eIntra4); }
uint32_t vp8e4_emu_mode_bytes(uint32_t flags) { return vp8e_mb_mode_bytes(flags); }
uint32_t vp8e4_emu_dearest_leaf(void) { return vp8e_host_tables().bmode_dearest; }

// BGRA rows -> the file and the BGRA a decoder makes of it (expect: w * h dwords, may be null).  penalty < 0: the coder's own
// kVp8eIntra4Penalty; else the member of its family to measure.
// stats[16]: [0] internal inconsistencies (must be 0), [1] quantiser index, [2] coefficient probabilities updated,
// [3] macroblocks skipped, [4] the file carries ALPH, [5] token partitions, [6] filter level, [7..10] macroblocks per 16x16 luma
// mode, [11] the first partition's bytes, [12] skip probability, [13] the largest |level|, [14] n_i4: B_PRED macroblocks,
// [15] pairs of a B_PRED and a 16x16 macroblock adjacent in a row | in a column << 16.
// modes (nullable): a byte per macroblock, 0..3 or 4 for B_PRED.
// Returns 0, 1 for a refused geometry or flag, or 2 when the file does not fit cap (*len is then what it needs).
int vp8e4_emu_encode(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful, float quality, uint32_t flags, int penalty, uint8_t* out, size_t cap,
                     size_t* len, uint32_t* expect, uint32_t* stats, uint8_t* modes) {
    std::memset(stats, 0, 16 * sizeof(uint32_t));
    if (w == 0 || h == 0 || w > kVp8eMaxDim || h > kVp8eMaxDim || (flags & ~(kVp8eIntra4 | kNaiveY2))) return 1;
    const bool intra4 = (flags & kVp8eIntra4) != 0u;
    const Vp8eTables& T = vp8e_host_tables();
    const uint32_t mbw = (w + 15u) / 16u, mbh = (h + 15u) / 16u;
    const size_t n_mbs = static_cast<size_t>(mbw) * mbh;
    Vp8eParams p = vp8e_params(T, vp8e_quality_to_index(quality), mbh, kVp8eFilterNum);
    if (penalty >= 0) p.i4_penalty = static_cast<uint8_t>(penalty);
    stats[1] = p.index; stats[5] = p.n_parts; stats[6] = p.filter_level;
    // 1. convert
    std::vector<uint8_t> sy(n_mbs * 256u), su(n_mbs * 64u), sv(n_mbs * 64u), ry(n_mbs * 256u), ru(n_mbs * 64u), rv(n_mbs * 64u);
    std::vector<uint32_t> grey(static_cast<size_t>(w) * h);
    const Vp8eSource S{bgra, stride, w, h, alpha_meaningful ? 1u : 0u, sy.data(), su.data(), sv.data(), grey.data(), mbw, mbh};
    uint32_t translucent = 0;
    for (uint32_t cy = 0; cy < mbh * 8u; ++cy)
        for (uint32_t cx = 0; cx < mbw * 8u; ++cx) translucent |= vp8e_convert_quad(S, cx, cy);
    stats[4] = translucent;
    // 2. the wavefront: macroblock (x, y) in step x + y, or in step x + 2y where the 4x4 modes are tried
    std::vector<Vp8Mb> mbs(n_mbs);
    std::vector<int16_t> levels(n_mbs * kVp8MbLevels);
    Vp8eFrame F{};
    F.src = Vp8Planes{sy.data(), su.data(), sv.data(), mbw * 16u, mbw * 8u, mbw, mbh};
    F.rec = Vp8Planes{ry.data(), ru.data(), rv.data(), mbw * 16u, mbw * 8u, mbw, mbh};
    F.mbs = mbs.data(); F.levels = levels.data(); F.p = p;
    auto W = std::make_unique<Vp8eMb4Work>();
    const uint32_t skew = intra4 ? 2u : 1u;
    for (uint32_t s = 0; s < mbw + skew * (mbh - 1u); ++s)
        for (uint32_t y = 0; y < mbh && skew * y <= s; ++y) {
            const uint32_t x = s - skew * y;
            if (x >= mbw) continue;
            if (intra4) vp8e_code_mb4(T, F, *W, x, y, 0u, 1u, [] {});
            else vp8e_code_mb(T, F, W->w, x, y, 0u, 1u, [] {});
        }
    if (flags & kNaiveY2)
        for (size_t m = 0; m < n_mbs; ++m) mbs[m].pad = (mbs[m].nz >> 24) & 1u ? 3u : 0u;
    // 3. statistics and probabilities
    std::vector<uint32_t> counts(2u * kVp8eProbs, 0u);
    Vp8eCountSink cs{counts.data()};
    uint32_t skipped = 0;
    for (size_t m = 0; m < n_mbs; ++m) {
        const uint32_t x = static_cast<uint32_t>(m % mbw);
        const bool i4 = mbs[m].ymode == kVp8ModeB;
        if (modes) modes[m] = mbs[m].ymode;
        if (i4) stats[14]++; else stats[7 + mbs[m].ymode]++;
        if (x && i4 != (mbs[m - 1u].ymode == kVp8ModeB)) stats[15] += 1u;
        if (m >= mbw && i4 != (mbs[m - mbw].ymode == kVp8ModeB)) stats[15] += 1u << 16;
        if (i4 && (mbs[m].nz >> 24 || !mbs[m].inner)) stats[0]++;
        for (uint32_t i = 0; i < kVp8MbLevels; ++i) stats[13] = std::max<uint32_t>(stats[13], static_cast<uint32_t>(vp8_abs(levels[m * kVp8MbLevels + i])));
        if (vp8e_mb_skipped(mbs[m])) { ++skipped; continue; }
        vp8e_mb_tokens(T, levels.data() + m * kVp8MbLevels, mbs[m], m >= mbw ? vp8e_ctx_above(mbs[m - mbw]) : 0u, x ? vp8e_ctx_left(mbs[m - 1u]) : 0u, cs);
    }
    std::vector<uint8_t> probs(kVp8eProbs), updated(kVp8eProbs);
    for (uint32_t i = 0; i < kVp8eProbs; ++i) {
        uint32_t u;
        probs[i] = static_cast<uint8_t>(vp8e_decide_prob(counts[2u * i], counts[2u * i + 1u], T.proba0[i], T.update[i], &u));
        updated[i] = static_cast<uint8_t>(u); stats[2] += u;
    }
    const uint32_t skip_p = vp8e_skip_prob(skipped, static_cast<uint32_t>(n_mbs));
    stats[3] = skipped; stats[12] = skip_p;
    // 4. bool coding: the first partition and every token partition, each a stream of its own
    Vp8eLayout L{};
    L.w = w; L.h = h; L.alpha = translucent; L.n_parts = p.n_parts;
    std::vector<uint8_t> first(std::min<uint64_t>(vp8e_first_cap(n_mbs, flags & kVp8eIntra4), kVp8eFirstPartMax));
    L.first_len = vp8e_first_partition(T, p, probs.data(), updated.data(), skip_p, mbs.data(), n_mbs, first.data(), static_cast<uint32_t>(first.size()), mbw);
    L.first = first.data();
    stats[11] = L.first_len;
    bool overflow = L.first_len > first.size();
    std::vector<std::vector<uint8_t>> parts(p.n_parts);
    for (uint32_t i = 0; i < p.n_parts; ++i) {
        parts[i].resize(vp8e_part_cap(mbw, mbh, p.n_parts));
        L.part_len[i] = vp8e_token_partition(T, probs.data(), mbs.data(), levels.data(), mbw, mbh, i, p.n_parts, parts[i].data(), static_cast<uint32_t>(parts[i].size()));
        L.part[i] = parts[i].data();
        if (L.part_len[i] > parts[i].size()) overflow = true;
    }
    // 5. the alpha plane: the grey frame through the lossless coder; its payload behind the five header bytes
    std::vector<uint8_t> inner;
    if (translucent) {
        inner.resize(webp_max_file_bytes(w, h));
        size_t inner_len = 0;
        uint32_t inner_stats[14];
        if (webp_emu_encode(reinterpret_cast<const uint8_t*>(grey.data()), w, h, w * 4u, 0, inner.data(), inner.size(), &inner_len, inner_stats) || inner_stats[0]) stats[0]++;
        const uint32_t payload = static_cast<uint32_t>(inner[16]) | inner[17] << 8 | inner[18] << 16 | static_cast<uint32_t>(inner[19]) << 24;
        L.alph_len = 1u + payload - 5u;
        L.alph_stream = inner.data() + kWebpRiff + 5u;
    }
    // 6. layout
    vp8e_layout_sizes(L);
    *len = L.file_len;
    if (overflow) { stats[0]++; return 2; }
    if (L.file_len > cap) return 2;
    if (L.file_len > vp8e_max_file_bytes(w, h, alpha_meaningful ? webp_max_file_bytes(w, h) : 0u, flags & kVp8eIntra4)) stats[0]++;
    for (uint32_t i = 0; i < L.file_len; ++i) out[i] = static_cast<uint8_t>(vp8e_file_byte(L, i));
    // 7. what a decoder makes of it: the loop filter over the reconstruction in raster order, then the conversion
    if (expect) {
        if (p.filter_level)
            for (uint32_t y = 0; y < mbh; ++y)
                for (uint32_t x = 0; x < mbw; ++x)
                    for (int vertical = 0; vertical < 2; ++vertical)
                        for (uint32_t lane = 0; lane < 32u; ++lane) vp8_filter_mb_line(F.rec, mbs[static_cast<size_t>(y) * mbw + x], kVp8FilterNormal, x, y, lane, vertical != 0);
        std::vector<uint8_t> A;
        if (translucent) { A.resize(grey.size()); for (size_t i = 0; i < grey.size(); ++i) A[i] = static_cast<uint8_t>(grey[i] >> 8); }
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) expect[static_cast<size_t>(y) * w + x] = vp8_bgra_pixel(F.rec, A.empty() ? nullptr : A.data(), w, h, x, y);
    }
    return 0;
}

}  // extern "C"

#ifdef VP8_ENC4_EMU_MAIN
// The sanitizer build: cases from a file (u32 w, h, alpha_meaningful, quality, flags, then w * h BGRA dwords), a line
// "status length file-checksum expected-checksum n_i4" per case.
#include <cstdio>
static uint32_t fnv(const uint8_t* p, size_t n) { uint32_t s = 0x811C9DC5u; for (size_t i = 0; i < n; ++i) s = (s ^ p[i]) * 0x01000193u; return s; }
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[5];
    while (std::fread(head, 4, 5, f) == 5) {
        const uint32_t w = head[0], h = head[1];
        std::vector<uint8_t> px(static_cast<size_t>(w) * h * 4u);
        if (std::fread(px.data(), 1, px.size(), f) != px.size()) return 2;
        std::vector<uint8_t> out(vp8e4_emu_max_file_bytes(w, h, head[2] != 0u, head[4]));       // exactly the bound: a byte beyond it is an error here
        std::vector<uint32_t> expect(static_cast<size_t>(w) * h);
        size_t len = 0;
        uint32_t stats[16];
        const int rc = vp8e4_emu_encode(px.data(), w, h, w * 4u, static_cast<int>(head[2]), static_cast<float>(head[3]), head[4], -1, out.data(), out.size(), &len, expect.data(),
                                        stats, nullptr);
        std::printf("%d %zu %u %u %u\n", rc || stats[0] ? 1 : 0, len, fnv(out.data(), len), fnv(reinterpret_cast<const uint8_t*>(expect.data()), expect.size() * 4u), stats[14]);
    }
    std::fclose(f);
    return 0;
}
#endif
