// webp_emulate.cpp -- the passes of csrc/webp_encode.hip (residuals, parse, codes, layout, emit, finish) on the CPU, from
// the same core header (csrc/webp_encode_core.hpp): the mode of a tile from the sums of its pixels, the greedy parse of a
// segment from the runs at the two distances (what the kernel's pointer jumping marks), a band's counts as the sum of its
// segments', the code construction, the layout's bit offsets and the bit placement into one zeroed stream.  Everything
// the kernels reduce in parallel is an integer sum, a maximum or an OR, so the order does not show.
// tests/test_webp_device_coder.py builds this with g++ and hands the files to libwebp (through Pillow) and to
// tests/vp8l_reader.py.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/webp_encode_core.hpp"

using namespace ifhip;

namespace {
constexpr uint32_t kLanes = 64;

// the five codes of a group (or of a sub-image) from its 1088 counts: tables, header stream, header bits
void build_codes(const uint32_t* cnt, uint32_t* tab, uint32_t* hdr, uint32_t* pos, uint32_t* stats, bool force_flat = false) {
    static WebpCodeWork W;
    for (uint32_t a = 0; a < 5u; ++a) {
        const uint32_t off = webp_alphabet_offset(a), n = webp_alphabet_size(a);
        for (uint32_t lane = 0; lane < kLanes; ++lane) code_rank_sort_lane(cnt + off, n, lane, kLanes, W.P.sorted);
        uint32_t fixed = 0;
        webp_build_code(W, cnt + off, a, tab + off, hdr, pos, &fixed, force_flat);
        stats[5] += fixed;
    }
}
}  // namespace

extern "C" {

uint64_t webp_emu_max_file_bytes(uint32_t w, uint32_t h) { return webp_max_file_bytes(w, h); }

// geometry[8]: the WebpShape of a frame
void webp_emu_shape(uint32_t w, uint32_t h, uint32_t* geometry) { const WebpShape s = webp_shape(w, h); std::memcpy(geometry, &s, sizeof s); }

uint32_t webp_emu_predict(uint32_t mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) { return webp_predict(mode, L, T, TL, TR); }
void webp_emu_prefix(uint32_t v, uint32_t* out3) { webp_prefix(v, out3, out3 + 1, out3 + 2); }

// BGRA rows -> the file.  stats[14]: [0] internal inconsistencies (must be 0), [1] matches one pixel back, [2] matches one
// row up, [3] groups, [4] segments, [5] fixed codes taken, [6] the payload's bits as the layout sums them, [7] tokens,
// [8] matches of 4096 pixels, [9] the bits of the main image's pixels, [10] bit offset of the second non-empty segment
// modulo 8 (0 when there is one), [11] the head's bits (everything in front of the first group's codes), [12] bands of one residual pixel throughout,
// [13] bands written as literals under flat codes.
// Returns 0, or 2 when the file does not fit cap (*len is then what it needs).
int webp_emu_encode(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful, uint8_t* out, size_t cap, size_t* len,
                    uint32_t* stats) {
    std::memset(stats, 0, 14 * sizeof(uint32_t));
    if (w == 0 || h == 0 || w > kWebpMaxDim || h > kWebpMaxDim) return 1;
    const WebpShape S = webp_shape(w, h);
    const uint32_t alpha_or = alpha_meaningful ? 0u : 0xFF000000u;
    const size_t N = static_cast<size_t>(w) * h;
    // 1. residuals: a tile's mode from the sums over its pixels
    std::vector<uint32_t> resid(N), modes(static_cast<size_t>(S.tiles_x) * S.tiles_y);
    for (uint32_t ty = 0; ty < S.tiles_y; ++ty)
        for (uint32_t tx = 0; tx < S.tiles_x; ++tx) {
            uint32_t sums[14] = {};
            const uint32_t x1 = std::min(w, (tx + 1u) * kWebpTile), y1 = std::min(h, (ty + 1u) * kWebpTile);
            for (uint32_t y = ty * kWebpTile; y < y1; ++y)
                for (uint32_t x = tx * kWebpTile; x < x1; ++x) {
                    const uint32_t px = webp_source(bgra, stride, x, y, alpha_or);
                    const WebpNeighbours nb = webp_neighbours(bgra, stride, w, x, y, alpha_or);
                    for (uint32_t m = 0; m < 14u; ++m) sums[m] += webp_residual_cost(webp_sub_pixels(px, webp_predict_at(m, x, y, nb)));
                }
            const uint32_t mode = webp_choose_mode(sums);
            modes[static_cast<size_t>(ty) * S.tiles_x + tx] = mode;
            for (uint32_t y = ty * kWebpTile; y < y1; ++y)
                for (uint32_t x = tx * kWebpTile; x < x1; ++x)
                    resid[static_cast<size_t>(y) * w + x] = webp_sub_pixels(webp_source(bgra, stride, x, y, alpha_or),
                                                                           webp_predict_at(mode, x, y, webp_neighbours(bgra, stride, w, x, y, alpha_or)));
        }
    // 2. parse: per segment, the runs at the two distances, the greedy walk, the counts
    std::vector<uint32_t> tok(N, 0u), seg_hist(static_cast<size_t>(S.n_segs) * kWebpSyms, 0u), seg_flat(2u * static_cast<size_t>(S.n_segs), 0u);
    for (uint32_t seg = 0; seg < S.n_segs; ++seg) {
        uint32_t start;
        const uint32_t n = webp_segment(S, seg, &start);
        std::vector<uint32_t> run1(n + 1u, 0u), runw(n + 1u, 0u);
        for (uint32_t i = n; i-- > 0u;) {
            const size_t g = static_cast<size_t>(start) + i;
            run1[i] = g >= 1u && resid[g] == resid[g - 1u] ? run1[i + 1u] + 1u : 0u;
            runw[i] = g >= w && resid[g] == resid[g - w] ? runw[i + 1u] + 1u : 0u;
        }
        uint32_t* hist = seg_hist.data() + static_cast<size_t>(seg) * kWebpSyms;
        seg_flat[2u * seg] = 1u; seg_flat[2u * seg + 1u] = n ? resid[start] : 0u;
        for (uint32_t k = 0; k < n; ++k) if (resid[start + k] != resid[start]) seg_flat[2u * seg] = 0u;
        uint32_t i = 0;
        while (i < n) {
            const uint32_t t = webp_choose_match(run1[i], runw[i], std::min(kWebpMaxMatch, n - i));
            tok[start + i] = t;
            const WebpTokenSymbols sy = webp_count_token(t, resid[start + i]);
            hist[sy.s0]++; hist[sy.s1]++;
            if (sy.n == 4u) { hist[sy.s2]++; hist[sy.s3]++; }
            stats[7]++;
            if ((t >> 16) == kWebpSelLeft) stats[1]++;
            if ((t >> 16) == kWebpSelRow) stats[2]++;
            if ((t & 0xFFFFu) == kWebpMaxMatch) stats[8]++;
            i += t & 0xFFFFu;
        }
        if (i != n) stats[0]++;
    }
    // 3. codes: a band's counts are the sum of its segments'; the exact bits of every segment
    std::vector<uint32_t> grp_tab(static_cast<size_t>(S.n_bands) * kWebpSyms), grp_hdr(static_cast<size_t>(S.n_bands) * kWebpGroupWords, 0u), grp_hbits(S.n_bands, 0u);
    std::vector<uint32_t> seg_bits(S.n_segs, 0u), literal_only(S.n_bands, 0u);
    WebpCodeWork flat_work;
    const uint32_t flat_group_bits = webp_flat_group_bits(flat_work);
    for (uint32_t b = 0; b < S.n_bands; ++b) {
        std::vector<uint32_t> cnt(kWebpSyms, 0u);
        for (uint32_t j = 0; j < S.segs_per_band; ++j)
            for (uint32_t s = 0; s < kWebpSyms; ++s) cnt[s] += seg_hist[(static_cast<size_t>(b) * S.segs_per_band + j) * kWebpSyms + s];
        // a band of one residual pixel throughout is coded as literals: five one-symbol codes, no bits for its pixels
        bool constant = true;
        uint32_t band_px = 0;
        const uint32_t value = seg_flat[2u * b * S.segs_per_band + 1u];
        for (uint32_t j = 0; j < S.segs_per_band; ++j) {
            const uint32_t seg = b * S.segs_per_band + j;
            uint32_t start;
            const uint32_t n = webp_segment(S, seg, &start);
            if (n && (!seg_flat[2u * seg] || seg_flat[2u * seg + 1u] != value)) constant = false;
            band_px += n;
        }
        if (constant) {
            std::fill(cnt.begin(), cnt.end(), 0u);
            const WebpTokenSymbols sy = webp_count_token(1u, value);
            cnt[sy.s0] = cnt[sy.s1] = cnt[sy.s2] = cnt[sy.s3] = band_px;
            stats[12]++;
        }
        uint32_t* tab = grp_tab.data() + static_cast<size_t>(b) * kWebpSyms;
        build_codes(cnt.data(), tab, grp_hdr.data() + static_cast<size_t>(b) * kWebpGroupWords, &grp_hbits[b], stats);
        if (grp_hbits[b] > kWebpGroupWords * 32u) stats[0]++;
        for (uint32_t j = 0; j < S.segs_per_band; ++j) {
            const uint32_t seg = b * S.segs_per_band + j;
            for (uint32_t s = 0; s < kWebpSyms; ++s) seg_bits[seg] += seg_hist[static_cast<size_t>(seg) * kWebpSyms + s] * webp_symbol_cost(tab, s);
            if (constant) seg_bits[seg] = 0;
        }
        // the band as literals under four flat codes, when that is smaller than its own codes with their headers
        uint64_t own = grp_hbits[b];
        for (uint32_t j = 0; j < S.segs_per_band; ++j) own += seg_bits[b * S.segs_per_band + j];
        literal_only[b] = constant ? 1u : 0u;
        if (!constant && flat_group_bits + 32ull * band_px < own) {
            literal_only[b] = 1u; stats[13]++;
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (uint32_t a = 0; a < 4u; ++a) for (uint32_t s = 0; s < 256u; ++s) cnt[webp_alphabet_offset(a) + s] = 1u;
            uint32_t* hdr = grp_hdr.data() + static_cast<size_t>(b) * kWebpGroupWords;
            std::fill(hdr, hdr + kWebpGroupWords, 0u);
            grp_hbits[b] = 0;
            build_codes(cnt.data(), tab, hdr, &grp_hbits[b], stats, true);
            if (grp_hbits[b] != flat_group_bits) stats[0]++;
            for (uint32_t j = 0; j < S.segs_per_band; ++j) {
                uint32_t start;
                seg_bits[b * S.segs_per_band + j] = 32u * webp_segment(S, b * S.segs_per_band + j, &start);
            }
        }
    }
    // 4. the head: front, the mode sub-image, middle, the entropy sub-image (literal only, one code set each)
    const uint32_t n_tiles = S.tiles_x * S.tiles_y, n_ent = S.ent_x * S.n_bands;
    std::vector<uint32_t> cnt(kWebpSyms, 0u), mode_tab(kWebpSyms), ent_tab(kWebpSyms), front(kWebpSubWords, 0u), middle(kWebpSubWords, 0u);
    uint32_t front_bits = 0, middle_bits = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) cnt[kWebpG + modes[t]]++;
    cnt[kWebpR] = cnt[kWebpB] = cnt[kWebpA + 255u] = n_tiles;
    webp_put_front(front.data(), &front_bits, w, h, alpha_meaningful ? 1u : 0u);
    build_codes(cnt.data(), mode_tab.data(), front.data(), &front_bits, stats);
    uint64_t mode_px_bits = 0, ent_px_bits = 0;
    for (uint32_t s = 0; s < kWebpSyms; ++s) mode_px_bits += static_cast<uint64_t>(cnt[s]) * (mode_tab[s] >> 16);
    std::fill(cnt.begin(), cnt.end(), 0u);
    for (uint32_t b = 0; b < S.n_bands; ++b) cnt[kWebpG + b] = S.ent_x;
    cnt[kWebpR] = cnt[kWebpB] = cnt[kWebpA + 255u] = n_ent;
    webp_put_middle(middle.data(), &middle_bits);
    build_codes(cnt.data(), ent_tab.data(), middle.data(), &middle_bits, stats);
    for (uint32_t s = 0; s < kWebpSyms; ++s) ent_px_bits += static_cast<uint64_t>(cnt[s]) * (ent_tab[s] >> 16);
    if (front_bits > kWebpSubWords * 32u || middle_bits > kWebpSubWords * 32u) stats[0]++;
    // 5. layout: one running sum over the head's pieces, the groups' headers and the segments
    const uint64_t at_mode_px = front_bits, at_middle = at_mode_px + mode_px_bits, at_ent_px = at_middle + middle_bits;
    uint64_t at = at_ent_px + ent_px_bits;
    stats[11] = static_cast<uint32_t>(at);
    std::vector<uint64_t> grp_off(S.n_bands), seg_off(S.n_segs);
    for (uint32_t b = 0; b < S.n_bands; ++b) { grp_off[b] = at; at += grp_hbits[b]; }
    uint32_t nonempty = 0;
    for (uint32_t seg = 0; seg < S.n_segs; ++seg) {
        seg_off[seg] = at; at += seg_bits[seg]; stats[9] += seg_bits[seg];
        uint32_t start;
        if (webp_segment(S, seg, &start) && ++nonempty == 2u) stats[10] = static_cast<uint32_t>(seg_off[seg] & 7u);
    }
    stats[3] = S.n_bands; stats[4] = S.n_segs; stats[6] = static_cast<uint32_t>(at);
    const uint64_t payload = (at + 7u) >> 3, file_len = kWebpRiff + payload + (payload & 1u);
    *len = file_len;
    if (file_len > cap) return 2;
    // 6. emit: everything is ORed into one zeroed stream
    std::vector<uint32_t> words(static_cast<size_t>(payload / 4u) + 4u, 0u);
    auto or_word = [](uint32_t* p, uint32_t v) { *p |= v; };
    auto or_stream = [&](const uint32_t* src, uint32_t bits, uint64_t where) {
        for (uint32_t i = 0; i < (bits + 31u) / 32u; ++i) or_bits(words.data(), where + 32ull * i, src[i], or_word);
    };
    auto emit_literals = [&](const uint32_t* tab, uint32_t count, uint64_t where, auto pixel) -> uint64_t {
        for (uint32_t i = 0; i < count; ++i) {
            uint64_t v;
            const uint32_t nb = webp_token_bits(tab, 1u, pixel(i), &v);
            if (nb) or_bits(words.data(), where, v, or_word);
            where += nb;
        }
        return where;
    };
    or_stream(front.data(), front_bits, 0);
    if (emit_literals(mode_tab.data(), n_tiles, at_mode_px, [&](uint32_t i) { return 0xFF000000u | (modes[i] << 8); }) != at_middle) stats[0]++;
    or_stream(middle.data(), middle_bits, at_middle);
    if (emit_literals(ent_tab.data(), n_ent, at_ent_px, [&](uint32_t i) { return 0xFF000000u | ((i / S.ent_x) << 8); }) != at_ent_px + ent_px_bits) stats[0]++;
    for (uint32_t b = 0; b < S.n_bands; ++b) or_stream(grp_hdr.data() + static_cast<size_t>(b) * kWebpGroupWords, grp_hbits[b], grp_off[b]);
    for (uint32_t seg = 0; seg < S.n_segs; ++seg) {
        uint32_t start;
        const uint32_t n = webp_segment(S, seg, &start);
        const uint32_t* tab = grp_tab.data() + static_cast<size_t>(seg / S.segs_per_band) * kWebpSyms;
        uint64_t where = seg_off[seg];
        if (seg_bits[seg] == 0u) continue;
        const bool literals = literal_only[seg / S.segs_per_band] != 0u;
        for (uint32_t i = 0; i < n; ++i) {
            if (!literals && !tok[start + i]) continue;
            uint64_t v;
            const uint32_t nb = webp_token_bits(tab, literals ? 1u : tok[start + i], resid[start + i], &v);
            if (nb) or_bits(words.data(), where, v, or_word);
            where += nb;
        }
        if (where != seg_off[seg] + seg_bits[seg]) stats[0]++;       // the layout's exact size is what the writer reaches
    }
    std::memset(out, 0, file_len);
    std::memcpy(out + kWebpRiff, words.data(), payload);
    if (webp_write_riff(out, static_cast<uint32_t>(payload)) != file_len) stats[0]++;
    return 0;
}

}  // extern "C"
