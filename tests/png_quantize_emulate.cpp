// png_quantize_emulate.cpp -- the passes of csrc/png_quantize.hip on the CPU from the same core header
// (csrc/png_quantize_core.hpp): the histogram with its posterise-and-re-run levels, palette growth and Lloyd refinement as
// 1024 lanes take their shares (in a scrambled order: every reduction is order-free), the file order of the palette, the
// Floyd-Steinberg remap in raster order -- what the device's skewed wavefront has to equal -- and the palette framing
// around the zlib stream of tests/png_emulate.cpp, with which this file is compiled.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/png_quantize_core.hpp"

using namespace ifhip;

extern "C" int png_emu_deflate(const uint8_t* stream, uint32_t n, uint32_t bpp, uint32_t pitch, int level, uint8_t* out, size_t cap, size_t* out_len,
                               uint32_t* stats);

namespace {
constexpr uint32_t kLanes = 1024;

struct Histogram { std::vector<uint32_t> key, w; uint32_t level = 0; };

bool histogram_level(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, bool alpha, uint32_t level, uint32_t max_entries, Histogram* out) {
    std::vector<uint32_t> slots(kPqSlots, 0u), counts(kPqSlots, 0u);
    uint32_t entries = 0;
    auto cas = [](uint32_t* p, uint32_t expect, uint32_t v) { const uint32_t held = *p; if (held == expect) *p = v; return held; };
    auto add = [](uint32_t* p, uint32_t v) { const uint32_t held = *p; *p += v; return held; };
    for (uint32_t y = h; y-- > 0u;)                                   // (bottom up: the order of arrival must not matter)
        for (uint32_t x = 0; x < w; ++x) {
            uint32_t px; std::memcpy(&px, bgra + static_cast<size_t>(y) * stride + 4u * x, 4);
            if (!pq_insert(slots.data(), counts.data(), &entries, max_entries, pq_posterize(pq_normalize(px, alpha), level), cas, add)) return false;
        }
    out->key.clear(); out->w.clear(); out->level = level;
    for (uint32_t s = 0; s < kPqSlots; ++s) if (slots[s]) { out->key.push_back(slots[s] ^ kPqSlotXor); out->w.push_back(counts[s]); }
    return true;
}
}  // namespace

extern "C" {

// status: 0, kPngFileOverflow or kPqQualityTooLow.  palette: kPqPaletteTap bytes (RGBA in file order, the count);
// indices: w * h; info[4]: histogram entries, posterise level, entries of alpha below 255, 0; err[2]: the summed error
// sum(weight * distance) before dithering, and the pixels.  file may be null (no file is built).
int pq_emu_quantize(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful, int quality, int min_quality, int speed_in,
                    uint32_t max_colors, int dither, int zlib_level, uint8_t* file, size_t cap, size_t* len, uint32_t* status, uint8_t* palette,
                    uint8_t* indices, uint32_t* info, uint64_t* err) {
    const uint32_t speed = static_cast<uint32_t>(std::min(10, std::max(1, speed_in < 0 ? 4 : speed_in)));
    const uint32_t target = static_cast<uint32_t>(std::min(100, std::max(0, quality < 0 ? 100 : quality)));
    const uint32_t minq = static_cast<uint32_t>(std::min<int>(target, std::max(0, min_quality < 0 ? 0 : min_quality)));
    const uint64_t bound_target = pq_quality_bound(target), bound_min = pq_quality_bound(minq), pixels = static_cast<uint64_t>(w) * h;
    const bool alpha = alpha_meaningful != 0;
    Histogram H;
    uint32_t level = 0;
    while (!histogram_level(bgra, w, h, stride, alpha, level, pq_speed_max_entries(speed), &H)) if (++level >= kPqLevels) return 1;
    const uint32_t n = static_cast<uint32_t>(H.key.size());
    std::vector<uint64_t> dmin(n, 0u);
    uint32_t keys[kPqMaxColors];
    PqColor pal[kPqMaxColors];
    uint32_t count = 1;
    {   // the heaviest colour, the lowest key on a tie
        uint64_t best = 0;
        for (uint32_t i = 0; i < n; ++i) best = std::max(best, (static_cast<uint64_t>(H.w[i]) << 32) | (~H.key[i]));
        keys[0] = ~static_cast<uint32_t>(best);
    }
    uint64_t total = 0;
    for (;;) {
        PqGrow g{0u, 0u, 0xFFFFFFFFu};
        for (uint32_t lane = kLanes; lane-- > 0u;) {
            PqGrow mine{0u, 0u, 0xFFFFFFFFu};
            pq_grow_lane(H.key.data(), H.w.data(), dmin.data(), n, lane, kLanes, keys[count - 1u], count == 1u, &mine);
            g.err += mine.err;
            pq_grow_better(&g, mine.score, mine.key);
        }
        total = g.err;
        if (total <= bound_target * pixels || count >= max_colors) break;
        keys[count++] = g.key;
    }
    for (uint32_t it = 0; it < pq_speed_iterations(speed); ++it) {
        for (uint32_t i = 0; i < count; ++i) pal[i] = pq_premultiply(keys[i]);
        std::vector<uint64_t> sums(kPqMaxColors * 5u, 0u);
        for (uint32_t i = n; i-- > 0u;) {
            uint64_t d;
            const uint32_t k = H.key[i], idx = pq_nearest(pal, count, pq_premultiply(k), &d);
            const uint64_t wt = H.w[i], wa = wt * (k >> 24);
            sums[idx * 5u + 0u] += wa * (k & 255u); sums[idx * 5u + 1u] += wa * ((k >> 8) & 255u); sums[idx * 5u + 2u] += wa * ((k >> 16) & 255u);
            sums[idx * 5u + 3u] += wa; sums[idx * 5u + 4u] += wt;
        }
        for (uint32_t i = 0; i < count; ++i) keys[i] = pq_centroid(&sums[i * 5u], keys[i]);
    }
    for (uint32_t i = 0; i < count; ++i) pal[i] = pq_premultiply(keys[i]);
    total = 0;
    for (uint32_t i = 0; i < n; ++i) { uint64_t d; pq_nearest(pal, count, pq_premultiply(H.key[i]), &d); total += d * H.w[i]; }
    uint32_t ordered[kPqMaxColors];
    const uint32_t n_trans = pq_order_palette(keys, count, ordered);
    for (uint32_t i = 0; i < count; ++i) pal[i] = pq_premultiply(ordered[i]);
    std::memset(palette, 0, kPqPaletteTap);
    for (uint32_t i = 0; i < count; ++i) {
        palette[4u * i] = static_cast<uint8_t>(ordered[i] >> 16); palette[4u * i + 1u] = static_cast<uint8_t>(ordered[i] >> 8);
        palette[4u * i + 2u] = static_cast<uint8_t>(ordered[i]); palette[4u * i + 3u] = static_cast<uint8_t>(ordered[i] >> 24);
    }
    std::memcpy(palette + 4u * kPqMaxColors, &count, 4);
    info[0] = n; info[1] = level; info[2] = n_trans; info[3] = 0;
    err[0] = total; err[1] = pixels;
    // the remap, raster order
    const uint32_t pitch = 1u + w;
    std::vector<uint8_t> stream(static_cast<size_t>(pitch) * h);
    std::vector<int32_t> above(4u * (w + 2u), 0), below(4u * (w + 2u), 0);
    for (uint32_t y = 0; y < h; ++y) {
        std::fill(below.begin(), below.end(), 0);
        int32_t right[4] = {0, 0, 0, 0};
        stream[static_cast<size_t>(y) * pitch] = 0;
        for (uint32_t x = 0; x < w; ++x) {
            uint32_t px; std::memcpy(&px, bgra + static_cast<size_t>(y) * stride + 4u * x, 4);
            int32_t in[4], e[4];
            for (int k = 0; k < 4; ++k) in[k] = right[k] + above[4u * (x + 1u) + k];
            const uint32_t idx = pq_remap_pixel(pal, ordered, count, pq_normalize(px, alpha), in, dither != 0, e);
            for (int k = 0; k < 4; ++k) {
                int32_t bl, b, br;
                pq_split_error(e[k], &right[k], &bl, &b, &br);
                below[4u * x + k] += bl; below[4u * (x + 1u) + k] += b; below[4u * (x + 2u) + k] += br;
            }
            stream[static_cast<size_t>(y) * pitch + 1u + x] = static_cast<uint8_t>(idx);
            indices[static_cast<size_t>(y) * w + x] = static_cast<uint8_t>(idx);
        }
        above.swap(below);
    }
    *len = 0;
    *status = 0;
    if (total > bound_min * pixels) { *status = kPqQualityTooLow; return 0; }
    if (!file) return 0;
    std::vector<uint8_t> z(stream.size() + stream.size() / 1000u + 4096u);
    size_t zlen = 0;
    uint32_t stats[10];
    if (png_emu_deflate(stream.data(), static_cast<uint32_t>(stream.size()), 1u, pitch, zlib_level, z.data(), z.size(), &zlen, stats) || stats[0]) return 2;
    const uint32_t head = pq_head_bytes(count, n_trans);
    if (head + 12u + zlen + 12u > cap) { *status = kPngFileOverflow; return 0; }
    uint8_t* c = file + pq_write_head(file, w, h, ordered, count, n_trans);
    std::memcpy(c + 8, z.data(), zlen);
    c += png_close_chunk(c, kPngIDAT, static_cast<uint32_t>(zlen));
    c += png_close_chunk(c, kPngIEND, 0);
    *len = static_cast<size_t>(c - file);
    return 0;
}

uint64_t pq_emu_quality_bound(uint32_t quality) { return pq_quality_bound(quality); }
uint64_t pq_emu_distance(uint32_t key_a, uint32_t key_b) { return pq_distance(pq_premultiply(key_a), pq_premultiply(key_b)); }

}  // extern "C"
