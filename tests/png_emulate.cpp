// png_emulate.cpp -- the passes of csrc/png_encode.hip (filter, finish) and csrc/png_deflate.hip (match, codes, layout,
// emit) on the CPU, lane by lane, from the same core header
// (csrc/png_encode_core.hpp): the filter choice of a wave per row, the round-based parse of a workgroup per chunk (hash
// table read before the round, pointer jumping for the greedy parse, highest position wins in the table), the code
// construction, the bit placement and the checksum combination over slices.  tests/test_png_device_coder.py builds this
// with g++ and hands the streams to zlib.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/png_encode_core.hpp"

using namespace ifhip;

namespace {
constexpr uint32_t kLanes = 64, kEmitThreads = 512;

struct Chunk {
    std::vector<uint32_t> tokens;
    std::vector<uint8_t> bytes;
    uint32_t adler = 1, crc = 0, type = 0;
};

uint32_t slice_checksum_crc(const uint8_t* p, uint32_t n, uint32_t threads) {
    // every lane: the CRC of its slice, shifted behind the bytes that follow it; the pieces meet by XOR
    const uint32_t per = (n + threads - 1u) / threads;
    uint32_t crc = 0;
    for (uint32_t t = 0; t < threads; ++t) {
        const uint32_t a = std::min(n, t * per), b = std::min(n, a + per);
        if (b > a) crc ^= png_crc_shift(png_crc32(p + a, b - a), n - b);
    }
    return crc;
}

void code_chunk(const uint8_t* stream, uint32_t total, uint32_t c, uint32_t n_chunks, uint32_t bpp, uint32_t pitch, bool stored_only, Chunk* out,
                uint32_t* stats) {
    const uint32_t start = c * kPngChunk, n = std::min(kPngChunk, total - start);
    const uint32_t win_start = start >= kPngWindow ? start - kPngWindow : 0u, woff = start - win_start, end = woff + n;
    std::vector<uint32_t> buf((kPngWindow + kPngChunk + 16u) / 4u, 0u);
    std::memcpy(buf.data(), stream + win_start, end);
    std::vector<uint32_t> table(1u << kPngHashBits, 0u);
    static PngCodeWork W;
    std::memset(&W, 0, sizeof W);
    // Adler-32: a slice per lane, then a tree of combinations
    {
        const uint32_t per = kPngChunk / kPngRound;
        std::vector<uint32_t> ad(kPngRound), ln(kPngRound);
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(buf.data()) + woff;
        for (uint32_t t = 0; t < kPngRound; ++t) {
            const uint32_t a = std::min(n, t * per), b = std::min(n, a + per);
            ad[t] = png_adler32(bytes + a, b - a); ln[t] = b - a;
        }
        for (uint32_t s = 1; s < kPngRound; s <<= 1)
            for (uint32_t t = 0; t < kPngRound; t += 2u * s) { ad[t] = png_adler_combine(ad[t], ad[t + s], ln[t + s]); ln[t] += ln[t + s]; }
        out->adler = ad[0];
    }
    if (!stored_only) {
        for (uint32_t lp = 0; lp < woff; ++lp) {                     // the window's positions enter the table: the highest wins
            if (lp + 3u > end) continue;
            uint32_t& e = table[png_hash3(png_load4(buf.data(), lp))];
            e = std::max(e, lp + 1u);
        }
        uint32_t covered = woff;
        std::vector<uint32_t> len(kPngRound), dist(kPngRound), nxt(kPngRound), nxt2(kPngRound);
        std::vector<uint8_t> mark(kPngRound), mark2(kPngRound);
        for (uint32_t base = woff; base < end; base += kPngRound) {
            for (uint32_t t = 0; t < kPngRound; ++t) {               // every lane against the table as it stood before the round
                const uint32_t lp = base + t;
                len[t] = 1; dist[t] = 0;
                if (lp >= end || lp < covered) continue;
                const uint32_t cand = lp + 3u <= end ? table[png_hash3(png_load4(buf.data(), lp))] : 0u;
                const uint32_t l = png_best_match(buf.data(), lp, std::min(kPngMaxMatch, end - lp), bpp, pitch, cand, &dist[t]);
                if (l) { len[t] = l; if (dist[t] == 1u || dist[t] == bpp || (dist[t] + bpp >= pitch && dist[t] <= pitch + bpp)) stats[1]++; else stats[2]++; }
            }
            for (uint32_t t = kPngRound; t-- > 0u;) {                // updates in a scrambled (here: reverse) order: max is order-free
                const uint32_t lp = base + t;
                if (lp + 3u > end) continue;
                uint32_t& e = table[png_hash3(png_load4(buf.data(), lp))];
                e = std::max(e, lp + 1u);
            }
            const uint32_t first = covered - base;                   // (covered >= base always)
            for (uint32_t t = 0; t < kPngRound; ++t) { nxt[t] = std::min(t + len[t], kPngRound); mark[t] = t == first; }
            for (int it = 0; it < 10; ++it) {                        // pointer jumping: marks double their reach every step
                mark2 = mark;
                for (uint32_t t = 0; t < kPngRound; ++t) {
                    const uint32_t j = nxt[t];
                    if (mark[t] && j < kPngRound) mark2[j] = 1;
                    nxt2[t] = j < kPngRound ? nxt[j] : kPngRound;
                }
                mark.swap(mark2); nxt.swap(nxt2);
            }
            for (uint32_t t = 0; t < kPngRound; ++t) {
                const uint32_t lp = base + t;
                if (!mark[t] || lp >= end) continue;
                const uint8_t byte = reinterpret_cast<const uint8_t*>(buf.data())[lp];
                if (len[t] >= kPngMinMatch) {
                    uint32_t s, eb, ev;
                    png_length_symbol(len[t], &s, &eb, &ev); W.cnt[s]++;
                    png_dist_symbol(dist[t], &s, &eb, &ev); W.cnt[kPngLL + s]++;
                    out->tokens.push_back(len[t] << 16 | dist[t]);
                    if (len[t] == kPngMinMatch) stats[8]++;
                    if (len[t] == kPngMaxMatch) stats[9]++;
                } else {
                    W.cnt[byte]++;
                    out->tokens.push_back(byte);
                }
                covered = std::max(covered, lp + len[t]);
            }
        }
        if (covered != end) stats[0]++;                              // the parse must tile the chunk exactly
    }
    W.cnt[256] = 1;
    for (uint32_t lane = 0; lane < kLanes; ++lane) code_rank_sort_lane(W.cnt, kPngLL, lane, kLanes, W.sorted);
    code_build_lengths(W, W.cnt, kPngLL, 15, W.len, 256, true);
    code_rank_sort_lane(W.cnt + kPngLL, kPngD, 0, 1, W.sorted);
    code_build_lengths(W, W.cnt + kPngLL, kPngD, 15, W.len + kPngLL, 0, false);
    const bool last = c + 1u == n_chunks;
    const uint32_t nbytes = png_plan_block(W, n, last, stored_only, &out->type);
    out->bytes.assign(nbytes, 0);
    if (out->type == 0u) {
        out->bytes[0] = last ? 1 : 0;
        out->bytes[1] = static_cast<uint8_t>(n); out->bytes[2] = static_cast<uint8_t>(n >> 8);
        out->bytes[3] = static_cast<uint8_t>(~n); out->bytes[4] = static_cast<uint8_t>(~n >> 8);
        std::memcpy(out->bytes.data() + 5, reinterpret_cast<const uint8_t*>(buf.data()) + woff, n);
    } else {
        std::vector<uint32_t> words(nbytes / 4u + 4u, 0u);
        for (uint32_t i = 0; i < (W.prefix_bits + 31u) / 32u; ++i) words[i] = W.prefix[i];
        uint32_t pos = W.prefix_bits;
        const uint32_t ntok = static_cast<uint32_t>(out->tokens.size());
        auto or_word = [](uint32_t* p, uint32_t v) { *p |= v; };
        for (uint32_t base = 0; base <= ntok; base += kEmitThreads) {
            uint32_t bits[kEmitThreads];
            uint64_t val[kEmitThreads];
            for (uint32_t t = 0; t < kEmitThreads; ++t) {
                const uint32_t i = base + t;
                bits[t] = 0; val[t] = 0;
                if (i < ntok) bits[t] = png_token_bits(W.tab, out->tokens[i], &val[t]);
                else if (i == ntok) { val[t] = W.tab[256] & 0xFFFFu; bits[t] = W.tab[256] >> 16; }
            }
            uint32_t ex = 0;
            std::vector<uint32_t> at(kEmitThreads);
            for (uint32_t t = 0; t < kEmitThreads; ++t) { at[t] = pos + ex; ex += bits[t]; }
            for (uint32_t t = kEmitThreads; t-- > 0u;) if (bits[t]) or_bits(words.data(), at[t], val[t], or_word);
            pos += ex;
        }
        const uint32_t coded = last ? (pos + 7u) >> 3 : ((pos + 3u + 7u) >> 3) + 4u;
        if (coded != nbytes) stats[0]++;                             // the plan's exact size is what the writer reaches
        std::memcpy(out->bytes.data(), words.data(), nbytes);
        if (!last) { out->bytes[nbytes - 2u] = 0xFF; out->bytes[nbytes - 1u] = 0xFF; }
    }
    out->crc = slice_checksum_crc(out->bytes.data(), nbytes, kEmitThreads);
    stats[3 + out->type]++;
}
}  // namespace

extern "C" {

// BGRA rows -> the filtered stream h * (1 + w * bpp), a wave per row
int png_emu_filter(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, uint32_t bpp, uint8_t* stream) {
    const uint32_t pitch = png_stream_pitch(w, bpp);
    auto px = [&](int64_t x, int64_t y) -> uint32_t {
        if (x < 0 || y < 0) return 0u;
        uint32_t v; std::memcpy(&v, bgra + y * stride + x * 4, 4); return v;
    };
    for (uint32_t y = 0; y < h; ++y) {
        uint32_t sums[5] = {0, 0, 0, 0, 0};
        for (uint32_t lane = 0; lane < kLanes; ++lane)
            for (uint32_t x = lane; x < w; x += kLanes) {
                const uint32_t cur = px(x, y), a = px(static_cast<int64_t>(x) - 1, y), b = px(x, static_cast<int64_t>(y) - 1), c = px(static_cast<int64_t>(x) - 1, static_cast<int64_t>(y) - 1);
                for (uint32_t ch = 0; ch < bpp; ++ch)
                    for (uint32_t f = 0; f < 5u; ++f)
                        sums[f] += png_filter_cost(png_filter_byte(f, png_channel(cur, ch), png_channel(a, ch), png_channel(b, ch), png_channel(c, ch)));
            }
        const uint32_t f = png_choose_filter(sums);
        uint8_t* row = stream + static_cast<size_t>(y) * pitch;
        row[0] = static_cast<uint8_t>(f);
        for (uint32_t x = 0; x < w; ++x) {
            const uint32_t cur = px(x, y), a = px(static_cast<int64_t>(x) - 1, y), b = px(x, static_cast<int64_t>(y) - 1), c = px(static_cast<int64_t>(x) - 1, static_cast<int64_t>(y) - 1);
            for (uint32_t ch = 0; ch < bpp; ++ch)
                row[1u + x * bpp + ch] = static_cast<uint8_t>(png_filter_byte(f, png_channel(cur, ch), png_channel(a, ch), png_channel(b, ch), png_channel(c, ch)));
        }
    }
    return 0;
}

// the filtered stream -> the zlib stream.  stats[10]: [0] internal inconsistencies (must be 0), [1] matches at the fixed
// distances, [2] matches from the hash table, [3..5] blocks stored / fixed / dynamic, [6] the CRC-32 of the stream as the
// device combines it, [7] tokens, [8] matches of length 3, [9] of length 258.
int png_emu_deflate(const uint8_t* stream, uint32_t n, uint32_t bpp, uint32_t pitch, int level, uint8_t* out, size_t cap, size_t* out_len,
                    uint32_t* stats) {
    std::memset(stats, 0, 10 * sizeof(uint32_t));
    if (n == 0) return 1;
    const uint32_t n_chunks = (n + kPngChunk - 1u) / kPngChunk;
    std::vector<Chunk> chunks(n_chunks);
    size_t total = 2;
    for (uint32_t c = 0; c < n_chunks; ++c) { code_chunk(stream, n, c, n_chunks, bpp, pitch, level == 0, &chunks[c], stats); total += chunks[c].bytes.size(); stats[7] += static_cast<uint32_t>(chunks[c].tokens.size()); }
    total += 4;
    *out_len = total;
    if (total > cap) return 2;
    const uint32_t hdr = png_zlib_header(level);
    out[0] = static_cast<uint8_t>(hdr >> 8); out[1] = static_cast<uint8_t>(hdr);
    size_t at = 2;
    uint32_t adler = 1, crc = png_crc_shift(png_crc32(out, 2), total - 2u);
    for (uint32_t c = 0; c < n_chunks; ++c) {
        std::memcpy(out + at, chunks[c].bytes.data(), chunks[c].bytes.size());
        at += chunks[c].bytes.size();
        crc ^= png_crc_shift(chunks[c].crc, total - at);
        adler = png_adler_combine(adler, chunks[c].adler, std::min(kPngChunk, n - c * kPngChunk));
    }
    png_be32(out + at, adler);
    crc ^= png_crc32(out + at, 4);
    stats[6] = crc;
    return 0;
}

// a whole file around a zlib stream, the way the last kernel frames it
int png_emu_file(const uint8_t* zstream, uint32_t zlen, uint32_t w, uint32_t h, uint32_t color_type, uint8_t* out) {
    png_write_head(out, w, h, color_type);
    uint8_t* c = out + kPngHeadBytes;
    std::memcpy(c + 8, zstream, zlen);
    c += png_close_chunk(c, kPngIDAT, zlen);
    c += png_close_chunk(c, kPngIEND, 0);
    return static_cast<int>(c - out);
}

uint32_t png_emu_crc32(const uint8_t* p, uint32_t n) { return png_crc32(p, n); }
uint32_t png_emu_crc_combine(uint32_t a, uint32_t b, uint64_t len_b) { return png_crc_combine(a, b, len_b); }
uint32_t png_emu_adler32(const uint8_t* p, uint32_t n) { return png_adler32(p, n); }
uint32_t png_emu_adler_combine(uint32_t a, uint32_t b, uint64_t len_b) { return png_adler_combine(a, b, len_b); }
void png_emu_symbols(uint32_t len, uint32_t dist, uint32_t* out6) {
    png_length_symbol(len, out6, out6 + 1, out6 + 2);
    png_dist_symbol(dist, out6 + 3, out6 + 4, out6 + 5);
}

}  // extern "C"
