// webp_indexed_emulate.cpp -- the device lossless-WebP coder with its stage flags (csrc/webp_encode.hip and
// csrc/webp_encode_indexed.hip) on the CPU, from the same core header (csrc/webp_encode_core.hpp).  The coder has one back
// end -- the parse of 4096-pixel segments, a band's five codes, the layout's running sum, the bit placement -- and two front
// ends that hand it an image and the head that goes in front of its groups: the plain one (subtract green, a predictor per
// tile; what tests/webp_emulate.cpp does, and with flags 0 the file must be that one's byte for byte) and, with
// IFHIP_WEBP_ENC_COLOR_INDEXING, the indexed one for frames of at most 256 colours (the sorted palette, the bundled
// indices).  Both are sized exactly and the smaller file is written; a tie goes to the plain one.
// tests/test_webp_indexed_coder.py builds this with g++ and hands the files to libwebp (through Pillow) and to
// tests/vp8l_reader.py.
#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

#include "../imageflow_amd/csrc/webp_encode_core.hpp"

using namespace ifhip;

namespace {
constexpr uint32_t kLanes = 64;
constexpr uint32_t kStats = 20;
constexpr uint32_t kFlagIndexing = 1u;

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

// What a front end hands the back end: the image the groups code (S.w x S.h pixels), and the head's first sub-image -- the
// bits in front of its codes, its pixels (the modes of the tiles, or the colour table's differences).
struct Variant {
    WebpShape S;
    std::vector<uint32_t> px;
    std::vector<uint32_t> front = std::vector<uint32_t>(kWebpGroupWords, 0u);
    uint32_t front_bits = 0;
    std::vector<uint32_t> sub;                  // the sub-image's pixels, ARGB
    // filled by size()
    std::vector<uint32_t> tok, seg_hist, seg_bits, literal_only, grp_tab, grp_hdr, grp_hbits, sub_tab, ent_tab, middle;
    std::vector<uint64_t> grp_off, seg_off;
    uint32_t middle_bits = 0;
    uint64_t at_sub_px = 0, at_middle = 0, at_ent_px = 0, ent_px_bits = 0, total_bits = 0;
    uint32_t stats[kStats] = {};

    uint64_t file_len() const { const uint64_t payload = (total_bits + 7u) >> 3; return kWebpRiff + payload + (payload & 1u); }

    // parse, codes, the head's codes and the layout: everything but the bits themselves
    void size() {
        const uint32_t w = S.w;
        const size_t N = static_cast<size_t>(S.w) * S.h;
        tok.assign(N, 0u); seg_hist.assign(static_cast<size_t>(S.n_segs) * kWebpSyms, 0u);
        std::vector<uint32_t> seg_flat(2u * static_cast<size_t>(S.n_segs), 0u);
        for (uint32_t seg = 0; seg < S.n_segs; ++seg) {
            uint32_t start;
            const uint32_t n = webp_segment(S, seg, &start);
            std::vector<uint32_t> run1(n + 1u, 0u), runw(n + 1u, 0u);
            for (uint32_t i = n; i-- > 0u;) {
                const size_t g = static_cast<size_t>(start) + i;
                run1[i] = g >= 1u && px[g] == px[g - 1u] ? run1[i + 1u] + 1u : 0u;
                runw[i] = g >= w && px[g] == px[g - w] ? runw[i + 1u] + 1u : 0u;
            }
            uint32_t* hist = seg_hist.data() + static_cast<size_t>(seg) * kWebpSyms;
            seg_flat[2u * seg] = 1u; seg_flat[2u * seg + 1u] = n ? px[start] : 0u;
            for (uint32_t k = 0; k < n; ++k) if (px[start + k] != px[start]) seg_flat[2u * seg] = 0u;
            uint32_t i = 0;
            while (i < n) {
                const uint32_t t = webp_choose_match(run1[i], runw[i], std::min(kWebpMaxMatch, n - i));
                tok[start + i] = t;
                const WebpTokenSymbols sy = webp_count_token(t, px[start + i]);
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
        grp_tab.assign(static_cast<size_t>(S.n_bands) * kWebpSyms, 0u); grp_hdr.assign(static_cast<size_t>(S.n_bands) * kWebpGroupWords, 0u);
        grp_hbits.assign(S.n_bands, 0u); seg_bits.assign(S.n_segs, 0u); literal_only.assign(S.n_bands, 0u);
        WebpCodeWork flat_work;
        const uint32_t flat_group_bits = webp_flat_group_bits(flat_work);
        for (uint32_t b = 0; b < S.n_bands; ++b) {
            std::vector<uint32_t> cnt(kWebpSyms, 0u);
            for (uint32_t j = 0; j < S.segs_per_band; ++j)
                for (uint32_t s = 0; s < kWebpSyms; ++s) cnt[s] += seg_hist[(static_cast<size_t>(b) * S.segs_per_band + j) * kWebpSyms + s];
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
        // the head: the front with the first sub-image's codes, its pixels, the middle with the entropy sub-image's codes, its pixels
        const uint32_t n_ent = S.ent_x * S.n_bands;
        std::vector<uint32_t> cnt(kWebpSyms, 0u);
        sub_tab.assign(kWebpSyms, 0u); ent_tab.assign(kWebpSyms, 0u); middle.assign(kWebpSubWords, 0u);
        for (uint32_t p : sub) { const WebpTokenSymbols sy = webp_count_token(1u, p); cnt[sy.s0]++; cnt[sy.s1]++; cnt[sy.s2]++; cnt[sy.s3]++; }
        build_codes(cnt.data(), sub_tab.data(), front.data(), &front_bits, stats);
        uint64_t sub_px_bits = 0;
        for (uint32_t s = 0; s < kWebpSyms; ++s) sub_px_bits += static_cast<uint64_t>(cnt[s]) * (sub_tab[s] >> 16);
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (uint32_t b = 0; b < S.n_bands; ++b) cnt[kWebpG + b] = S.ent_x;
        cnt[kWebpR] = cnt[kWebpB] = cnt[kWebpA + 255u] = n_ent;
        webp_put_middle(middle.data(), &middle_bits);
        build_codes(cnt.data(), ent_tab.data(), middle.data(), &middle_bits, stats);
        for (uint32_t s = 0; s < kWebpSyms; ++s) ent_px_bits += static_cast<uint64_t>(cnt[s]) * (ent_tab[s] >> 16);
        if (front_bits > kWebpGroupWords * 32u || middle_bits > kWebpSubWords * 32u) stats[0]++;
        at_sub_px = front_bits; at_middle = at_sub_px + sub_px_bits; at_ent_px = at_middle + middle_bits;
        uint64_t at = at_ent_px + ent_px_bits;
        stats[11] = static_cast<uint32_t>(at);
        grp_off.assign(S.n_bands, 0); seg_off.assign(S.n_segs, 0);
        for (uint32_t b = 0; b < S.n_bands; ++b) { grp_off[b] = at; at += grp_hbits[b]; }
        uint32_t nonempty = 0;
        for (uint32_t seg = 0; seg < S.n_segs; ++seg) {
            seg_off[seg] = at; at += seg_bits[seg]; stats[9] += seg_bits[seg];
            uint32_t start;
            if (webp_segment(S, seg, &start) && ++nonempty == 2u) stats[10] = static_cast<uint32_t>(seg_off[seg] & 7u);
        }
        stats[3] = S.n_bands; stats[4] = S.n_segs; stats[6] = static_cast<uint32_t>(at);
        total_bits = at;
    }

    // everything is ORed into one zeroed stream
    void write(uint8_t* out) {
        const uint64_t payload = (total_bits + 7u) >> 3, len = file_len();
        const uint32_t n_ent = S.ent_x * S.n_bands;
        std::vector<uint32_t> words(static_cast<size_t>(payload / 4u) + 4u, 0u);
        auto or_word = [](uint32_t* p, uint32_t v) { *p |= v; };
        auto or_stream = [&](const uint32_t* src, uint32_t bits, uint64_t where) {
            for (uint32_t i = 0; i < (bits + 31u) / 32u; ++i) or_bits(words.data(), where + 32ull * i, src[i], or_word);
        };
        auto emit_literals = [&](const uint32_t* tab, uint32_t count, uint64_t where, const std::function<uint32_t(uint32_t)>& pixel) -> uint64_t {
            for (uint32_t i = 0; i < count; ++i) {
                uint64_t v;
                const uint32_t nb = webp_token_bits(tab, 1u, pixel(i), &v);
                if (nb) or_bits(words.data(), where, v, or_word);
                where += nb;
            }
            return where;
        };
        or_stream(front.data(), front_bits, 0);
        if (emit_literals(sub_tab.data(), static_cast<uint32_t>(sub.size()), at_sub_px, [&](uint32_t i) { return sub[i]; }) != at_middle) stats[0]++;
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
                const uint32_t nb = webp_token_bits(tab, literals ? 1u : tok[start + i], px[start + i], &v);
                if (nb) or_bits(words.data(), where, v, or_word);
                where += nb;
            }
            if (where != seg_off[seg] + seg_bits[seg]) stats[0]++;
        }
        std::memset(out, 0, len);
        std::memcpy(out + kWebpRiff, words.data(), payload);
        if (webp_write_riff(out, static_cast<uint32_t>(payload)) != len) stats[0]++;
    }
};

// the plain front end: a tile's mode from the sums over its pixels, the residuals
void plain_front(Variant& V, const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, uint32_t alpha_or) {
    V.S = webp_shape(w, h);
    const WebpShape& S = V.S;
    V.px.assign(static_cast<size_t>(w) * h, 0u);
    V.sub.assign(static_cast<size_t>(S.tiles_x) * S.tiles_y, 0u);
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
            V.sub[static_cast<size_t>(ty) * S.tiles_x + tx] = 0xFF000000u | (mode << 8);
            for (uint32_t y = ty * kWebpTile; y < y1; ++y)
                for (uint32_t x = tx * kWebpTile; x < x1; ++x)
                    V.px[static_cast<size_t>(y) * w + x] = webp_sub_pixels(webp_source(bgra, stride, x, y, alpha_or),
                                                                          webp_predict_at(mode, x, y, webp_neighbours(bgra, stride, w, x, y, alpha_or)));
        }
    webp_put_front(V.front.data(), &V.front_bits, w, h, alpha_or ? 0u : 1u);
}

// the indexed front end: the frame's colours in ascending order, the bundled indices.  false: more than 256 colours
bool indexed_front(Variant& V, const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, uint32_t alpha_or, uint32_t* n_colours, uint32_t* width_bits) {
    std::vector<uint32_t> pal;
    pal.reserve(static_cast<size_t>(w) * h);
    for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) pal.push_back(webp_argb(bgra, stride, x, y, alpha_or));
    std::sort(pal.begin(), pal.end());
    pal.erase(std::unique(pal.begin(), pal.end()), pal.end());
    if (pal.size() > kWebpMaxPalette) return false;
    const uint32_t n = static_cast<uint32_t>(pal.size()), bits = webp_index_width_bits(n), pw = webp_packed_width(w, bits);
    *n_colours = n; *width_bits = bits;
    V.S = webp_shape(pw, h);
    V.px.assign(static_cast<size_t>(pw) * h, 0u);
    for (uint32_t y = 0; y < h; ++y) for (uint32_t xp = 0; xp < pw; ++xp) V.px[static_cast<size_t>(y) * pw + xp] = webp_bundle(bgra, stride, w, xp, y, alpha_or, pal.data(), n, bits);
    V.sub.assign(n, 0u);
    for (uint32_t i = 0; i < n; ++i) V.sub[i] = webp_palette_delta(pal.data(), i);
    webp_put_front_indexed(V.front.data(), &V.front_bits, w, h, alpha_or ? 0u : 1u, n);
    return true;
}
}  // namespace

extern "C" {

uint32_t webp_ix_index_width_bits(uint32_t n_colours) { return webp_index_width_bits(n_colours); }

// BGRA rows -> the file under the stage flags.  stats[20]: [0..13] as tests/webp_emulate.cpp's, of the variant that was
// written; [14] 1 when that is the indexed one; [15] the frame's colours (0: more than 256, or the flag is off);
// [16] the width bits of the bundling; [17] the packed width; [18] the plain file's bytes; [19] the indexed file's (0: not sized).
// Returns 0, 1 for arguments out of range, or 2 when the file does not fit cap (*len is then what it needs).
int webp_ix_encode(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful, uint32_t flags, uint8_t* out, size_t cap, size_t* len,
                   uint32_t* stats) {
    std::memset(stats, 0, kStats * sizeof(uint32_t));
    if (w == 0 || h == 0 || w > kWebpMaxDim || h > kWebpMaxDim || (flags & ~kFlagIndexing)) return 1;
    const uint32_t alpha_or = alpha_meaningful ? 0u : 0xFF000000u;
    Variant plain, indexed;
    plain_front(plain, bgra, w, h, stride, alpha_or);
    plain.size();
    Variant* chosen = &plain;
    uint32_t n_colours = 0, width_bits = 0;
    uint64_t indexed_len = 0;
    if ((flags & kFlagIndexing) && indexed_front(indexed, bgra, w, h, stride, alpha_or, &n_colours, &width_bits)) {
        indexed.size();
        indexed_len = indexed.file_len();
        if (indexed_len < plain.file_len()) chosen = &indexed;
    }
    std::memcpy(stats, chosen->stats, 14 * sizeof(uint32_t));
    stats[14] = chosen == &indexed ? 1u : 0u; stats[15] = n_colours; stats[16] = width_bits; stats[17] = n_colours ? indexed.S.w : 0u;
    stats[18] = static_cast<uint32_t>(plain.file_len()); stats[19] = static_cast<uint32_t>(indexed_len);
    *len = chosen->file_len();
    if (*len <= cap) chosen->write(out);
    stats[0] = plain.stats[0] + indexed.stats[0];
    return *len > cap ? 2 : 0;
}

}  // extern "C"
