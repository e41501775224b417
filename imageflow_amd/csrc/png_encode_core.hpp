// png_encode_core.hpp -- the arithmetic of the device PNG coder (csrc/png_encode.hip), written so that it compiles for the
// gfx950 kernels AND for a plain host compiler: tests/png_emulate.cpp runs the same filter choice, the same round-based
// parse, the same code construction and the same bit placement lane by lane on the CPU, and zlib must inflate what comes
// out -- test infrastructure; the product has one path, the kernels.
//
// What is coded: EncoderPreset::Libpng (imageflow_types/src/lib.rs:751-755, codecs/libpng_encoder.rs:43-72,134-160,
// c_components/lib/codec_png_wrapper.c:349-430): 8-bit RGB / RGBA, non-interlaced, libpng's default adaptive row filters,
// one zlib stream.  The deflate blocks are this coder's own (a parallel parse cannot equal zlib's serial one byte for
// byte); every rule with a bit in it -- RFC 1950 / 1951 and the PNG specification -- lives here.
#pragma once
#include <cstdint>

#ifndef IFHIP_HD
#if defined(__HIPCC__)
#define IFHIP_HD __host__ __device__ __forceinline__
#else
#define IFHIP_HD inline
#endif
#endif

namespace ifhip {

constexpr uint32_t kPngChunk = 32768;        // filtered bytes per deflate block (one workgroup's piece)
constexpr uint32_t kPngWindow = 32768;       // RFC 1951: distances reach 32 KiB back
constexpr uint32_t kPngRound = 1024;         // positions a workgroup parses per round: 64 per wave, 16 waves
constexpr uint32_t kPngMinMatch = 3, kPngMaxMatch = 258;
constexpr uint32_t kPngTooFar = 4096;        // a 3-byte match further back than this costs more than its literals (zlib's TOO_FAR)
// Shortest match taken at distance 1 (kPngMinMatch), at the other fixed distances, and from the hash table.  Filtered image
// data is noisy: short matches at arbitrary distances cost more than their literals under the chunk's own code (zlib's
// Z_FILTERED strategy, which libpng selects, drops matches of 5 bytes or fewer for the same reason).  DESIGN 4.9 has the sizes.
constexpr uint32_t kPngMinNear = 4, kPngMinHashed = 6;
constexpr uint32_t kPngHashBits = 13;
constexpr uint32_t kPngLL = 286, kPngD = 30, kPngCL = 19, kPngSyms = kPngLL + kPngD;
constexpr uint32_t kPngPrefixWords = 144;    // block header: 3 + 14 + 19*3 + 316*(7+7) bits at most = 4498 bits
constexpr uint32_t kPngFraming = 8 + 25 + 16 + 13 + 44 + 12 + 12;   // signature, IHDR, gAMA, sRGB, cHRM, IDAT's 12 bytes, IEND
constexpr uint32_t kPngFileOverflow = 1;

// ---- filters (PNG specification 9.2; libpng's default choice for 8-bit truecolour) ---------------------------------------
IFHIP_HD uint32_t png_paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = static_cast<int>(a) + static_cast<int>(b) - static_cast<int>(c);
    int pa = p - static_cast<int>(a), pb = p - static_cast<int>(b), pc = p - static_cast<int>(c);
    pa = pa < 0 ? -pa : pa; pb = pb < 0 ? -pb : pb; pc = pc < 0 ? -pc : pc;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
// x: the byte, a: bpp to the left, b: above, c: above left (0 outside the image)
IFHIP_HD uint32_t png_filter_byte(uint32_t f, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t pred = f == 0u ? 0u : f == 1u ? a : f == 2u ? b : f == 3u ? (a + b) >> 1 : png_paeth(a, b, c);
    return (x - pred) & 255u;
}
IFHIP_HD uint32_t png_filter_cost(uint32_t v) { return v < 128u ? v : 256u - v; }
IFHIP_HD uint32_t png_choose_filter(const uint32_t sums[5]) {     // the smallest sum; a tie goes to the lowest number
    uint32_t best = 0, least = sums[0];
    for (uint32_t f = 1; f < 5u; ++f) if (sums[f] < least) { least = sums[f]; best = f; }
    return best;
}
// channel `ch` of the file's pixel (R, G, B, A) from a BGRA dword
IFHIP_HD uint32_t png_channel(uint32_t bgra, uint32_t ch) { return (bgra >> (ch == 3u ? 24u : 16u - 8u * ch)) & 255u; }

// ---- deflate symbols (RFC 1951 3.2.5) --------------------------------------------------------------------------------------
IFHIP_HD uint32_t png_log2(uint32_t v) { return 31u - static_cast<uint32_t>(__builtin_clz(v)); }
IFHIP_HD void png_length_symbol(uint32_t len, uint32_t* sym, uint32_t* ebits, uint32_t* eval) {
    const uint32_t l = len - 3u;
    if (len == 258u) { *sym = 285u; *ebits = 0; *eval = 0; return; }
    if (l < 8u) { *sym = 257u + l; *ebits = 0; *eval = 0; return; }
    const uint32_t e = png_log2(l) - 2u;
    *sym = 261u + 4u * e + ((l >> e) & 3u); *ebits = e; *eval = l & ((1u << e) - 1u);
}
IFHIP_HD void png_dist_symbol(uint32_t dist, uint32_t* sym, uint32_t* ebits, uint32_t* eval) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { *sym = d; *ebits = 0; *eval = 0; return; }
    const uint32_t e = png_log2(d) - 1u;
    *sym = 2u * (e + 1u) + ((d >> e) & 1u); *ebits = e; *eval = d & ((1u << e) - 1u);
}
IFHIP_HD uint32_t png_ll_extra_bits(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
IFHIP_HD uint32_t png_d_extra_bits(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }
IFHIP_HD uint32_t png_fixed_ll_length(uint32_t sym) { return sym < 144u ? 8u : sym < 256u ? 9u : sym < 280u ? 7u : 8u; }

// ---- the parse: tokens ---------------------------------------------------------------------------------------------------------
// A token is a literal (the byte) or a match (length << 16 | distance).  The stream lies in a dword buffer (little endian).
IFHIP_HD uint32_t png_load4(const uint32_t* w, uint32_t p) {          // four bytes at byte position p (reads one dword further)
    const uint64_t v = static_cast<uint64_t>(w[p >> 2]) | (static_cast<uint64_t>(w[(p >> 2) + 1u]) << 32);
    return static_cast<uint32_t>(v >> ((p & 3u) * 8u));
}
IFHIP_HD uint32_t png_hash3(uint32_t v) { return ((v & 0xFFFFFFu) * 0x9E3779B1u) >> (32u - kPngHashBits); }
IFHIP_HD uint32_t png_match_length(const uint32_t* w, uint32_t p, uint32_t q, uint32_t cap) {
    uint32_t n = 0;
    while (n < cap) {
        const uint32_t x = png_load4(w, p + n) ^ png_load4(w, q + n);
        if (x) { n += static_cast<uint32_t>(__builtin_ctz(x)) >> 3; break; }
        n += 4u;
    }
    return n < cap ? n : cap;
}
// The best match of position lp (a byte index of the buffer; everything below lp is history): the distances PNG data
// favours -- 1, bpp, the row pitch and its two neighbours -- and the hash table's candidate (position + 1 as the table
// stood BEFORE the round, 0 = none).  The longest wins, the earlier candidate on a tie.  Returns the length (0: literal).
IFHIP_HD uint32_t png_best_match(const uint32_t* w, uint32_t lp, uint32_t cap, uint32_t bpp, uint32_t pitch, uint32_t hash_cand,
                                 uint32_t* dist_out) {
    uint32_t best = 0, bd = 0;
    if (cap >= kPngMinMatch) {
        for (uint32_t k = 0; k < 6u; ++k) {
            uint32_t dist = k == 0u ? 1u : k == 1u ? bpp : k == 2u ? pitch - bpp : k == 3u ? pitch : k == 4u ? pitch + bpp
                                                                                   : (hash_cand && hash_cand - 1u < lp ? lp - (hash_cand - 1u) : 0u);
            if (dist == 0u || dist > lp || dist > kPngWindow || best >= cap) continue;
            const uint32_t len = png_match_length(w, lp, lp - dist, cap);
            if (len > best && len >= (k == 0u ? kPngMinMatch : k < 5u ? kPngMinNear : kPngMinHashed)) { best = len; bd = dist; }
        }
    }
    if (best < kPngMinMatch || (best == kPngMinMatch && bd > kPngTooFar)) best = 0;
    *dist_out = bd;
    return best;
}

// ---- code construction -----------------------------------------------------------------------------------------------------------
// Workspace of one chunk's code construction (LDS on the device): nothing here is indexed from registers.
struct PngCodeWork {
    uint32_t cnt[kPngSyms + 4];      // in: literal/length counts [0, 286), distance counts [286, 316)
    uint32_t tab[kPngSyms + 4];      // out: bit-reversed code | length << 16 per symbol, of the block type chosen
    uint8_t len[kPngSyms + 4 + 20];  // code lengths: literal/length, distance, then the code-length alphabet at 320
    uint16_t sorted[288];
    uint32_t wt[576];
    uint16_t parent[576];
    uint32_t nc[36];                 // codes per length, then the next code per length
    uint16_t rle[kPngSyms + 4];      // header symbols: symbol | extra value << 8
    uint32_t nrle, hlit, hdist, hclen;
    uint32_t clcnt[20], cltab[20];
    uint32_t prefix[kPngPrefixWords];    // the block's first bits: BFINAL, BTYPE and the dynamic header
    uint32_t prefix_bits;
};
constexpr uint32_t kPngLenCL = kPngSyms + 4;   // where the code-length alphabet's lengths start in PngCodeWork::len

// rank of every used symbol in increasing (count, symbol) order -- the part of the sort one lane of `nlanes` does
IFHIP_HD void png_rank_sort_lane(const uint32_t* cnt, uint32_t n, uint32_t lane, uint32_t nlanes, uint16_t* sorted) {
    for (uint32_t s = lane; s < n; s += nlanes) {
        const uint32_t cs = cnt[s];
        if (!cs) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < n; ++t) { const uint32_t c = cnt[t]; r += (c && (c < cs || (c == cs && t < s))) ? 1u : 0u; }
        sorted[r] = static_cast<uint16_t>(s);
    }
}
// Code lengths of at most max_bits from counts (`sorted` filled by png_rank_sort_lane): Huffman's algorithm with two
// queues, then the depth histogram is moved under the limit the way zlib's gen_bitlen / miniz do (a code of the longest
// length below the limit is split, one of the limit is taken away, until the Kraft sum is 1 again) and the lengths are
// handed out again, longest to the rarest.  Fewer than two used symbols: the used one (else `lone`) gets one bit, and when
// `complete` a second symbol gets the other one-bit code.  Returns the number of used symbols.
IFHIP_HD uint32_t png_build_lengths(PngCodeWork& W, const uint32_t* cnt, uint32_t n, uint32_t max_bits, uint8_t* len, uint32_t lone, bool complete) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; ++s) { len[s] = 0; m += cnt[s] ? 1u : 0u; }
    if (m < 2u) {
        const uint32_t used = m ? W.sorted[0] : lone;
        len[used] = 1;
        if (complete) len[used == 0u ? 1u : 0u] = 1;
        return m;
    }
    for (uint32_t i = 0; i < m; ++i) W.wt[i] = cnt[W.sorted[i]];
    uint32_t li = 0, ii = m, next = m;
    while (next < 2u * m - 1u) {
        uint32_t sum = 0;
        for (int k = 0; k < 2; ++k) {
            uint32_t pick;
            if (li < m && (ii >= next || W.wt[li] <= W.wt[ii])) pick = li++; else pick = ii++;
            sum += W.wt[pick];
            W.parent[pick] = static_cast<uint16_t>(next);
        }
        W.wt[next++] = sum;
    }
    const uint32_t root = 2u * m - 2u;
    W.wt[root] = 0;
    for (uint32_t i = root; i-- > 0u;) W.wt[i] = W.wt[W.parent[i]] + 1u;        // depths (a parent has the higher index)
    for (uint32_t b = 0; b <= max_bits; ++b) W.nc[b] = 0;
    for (uint32_t i = 0; i < m; ++i) W.nc[W.wt[i] < max_bits ? W.wt[i] : max_bits] += 1u;
    uint32_t total = 0;
    for (uint32_t b = max_bits; b > 0u; --b) total += W.nc[b] << (max_bits - b);
    while (total != (1u << max_bits)) {
        W.nc[max_bits] -= 1u;
        for (uint32_t b = max_bits - 1u; b > 0u; --b) if (W.nc[b]) { W.nc[b] -= 1u; W.nc[b + 1u] += 2u; break; }
        total -= 1u;
    }
    uint32_t j = 0;
    for (uint32_t b = max_bits; b > 0u; --b) for (uint32_t k = 0; k < W.nc[b]; ++k) len[W.sorted[j++]] = static_cast<uint8_t>(b);
    return m;
}
IFHIP_HD uint32_t png_reverse_bits(uint32_t v, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1u - i);
    return r;
}
// canonical codes (RFC 1951 3.2.2), stored bit-reversed: a Huffman code enters the stream most significant bit first, and
// the writer packs everything from the low bit
IFHIP_HD void png_assign_codes(PngCodeWork& W, const uint8_t* len, uint32_t n, uint32_t* tab) {
    for (uint32_t b = 0; b < 18u; ++b) W.nc[b] = 0;
    for (uint32_t s = 0; s < n; ++s) W.nc[len[s]] += 1u;
    uint32_t code = 0;
    W.nc[0] = 0;
    for (uint32_t b = 1; b <= 15u; ++b) { code = (code + W.nc[b - 1u]) << 1; W.nc[18u + b] = code; }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = len[s];
        tab[s] = l ? (png_reverse_bits(W.nc[18u + l]++, l) | (l << 16)) : 0u;
    }
}
// `nbits` (at most 32) bits of v at bit position *pos of a zeroed dword stream, low bit first; one writer
IFHIP_HD void png_put(uint32_t* words, uint32_t* pos, uint32_t v, uint32_t nbits) {
    const uint64_t x = static_cast<uint64_t>(v) << (*pos & 31u);
    words[*pos >> 5] |= static_cast<uint32_t>(x);
    if (x >> 32) words[(*pos >> 5) + 1u] |= static_cast<uint32_t>(x >> 32);
    *pos += nbits;
}
IFHIP_HD uint32_t png_cl_order(uint32_t i) {       // RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 8u - ((i - 3u) >> 1) : 8u + ((i - 4u) >> 1);
}
IFHIP_HD void png_rle_emit(PngCodeWork& W, uint32_t sym, uint32_t extra) {
    W.rle[W.nrle++] = static_cast<uint16_t>(sym | (extra << 8));
    W.clcnt[sym] += 1u;
}
// The plan of one chunk's block, by one lane, from the counts and the dynamic lengths in W.len (png_build_lengths for the
// two alphabets): the dynamic header, the exact size of the block as dynamic, fixed and stored, the cheapest of the three,
// its code tables and its first bits.  A block that is not the stream's last is followed by an empty stored block, which
// closes it to a byte boundary (what a zlib sync flush writes: 3 bits, padding, 00 00 FF FF); a stored block starts on
// one and needs none.  Returns the chunk's bytes in the stream; *type_out: BTYPE.
IFHIP_HD uint32_t png_plan_block(PngCodeWork& W, uint32_t n_bytes, bool last, bool stored_only, uint32_t* type_out) {
    uint32_t hlit = kPngLL, hdist = kPngD;
    while (hlit > 257u && W.len[hlit - 1u] == 0) --hlit;
    while (hdist > 1u && W.len[kPngLL + hdist - 1u] == 0) --hdist;
    W.hlit = hlit; W.hdist = hdist; W.nrle = 0;
    for (uint32_t i = 0; i < 20u; ++i) W.clcnt[i] = 0;
    const uint32_t total = hlit + hdist;
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = W.len[i < hlit ? i : kPngLL + (i - hlit)];
        uint32_t run = 1;
        while (i + run < total) {
            const uint32_t k = i + run;
            if (W.len[k < hlit ? k : kPngLL + (k - hlit)] != v) break;
            ++run;
        }
        i += run;
        if (v == 0u) {
            while (run >= 11u) { const uint32_t t = run < 138u ? run : 138u; png_rle_emit(W, 18u, t - 11u); run -= t; }
            if (run >= 3u) { png_rle_emit(W, 17u, run - 3u); run = 0; }
        } else {
            png_rle_emit(W, v, 0); --run;
            while (run >= 3u) { const uint32_t t = run < 6u ? run : 6u; png_rle_emit(W, 16u, t - 3u); run -= t; }
        }
        while (run > 0u) { png_rle_emit(W, v, 0); --run; }
    }
    png_rank_sort_lane(W.clcnt, kPngCL, 0, 1, W.sorted);
    png_build_lengths(W, W.clcnt, kPngCL, 7, W.len + kPngLenCL, 0, true);
    uint32_t hclen = kPngCL;
    while (hclen > 4u && W.len[kPngLenCL + png_cl_order(hclen - 1u)] == 0) --hclen;
    W.hclen = hclen;
    uint64_t dyn = 14u + 3u * hclen, fix = 0;
    for (uint32_t i = 0; i < W.nrle; ++i) {
        const uint32_t s = W.rle[i] & 255u;
        dyn += W.len[kPngLenCL + s] + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
    }
    for (uint32_t s = 0; s < kPngLL; ++s) { dyn += static_cast<uint64_t>(W.cnt[s]) * (W.len[s] + png_ll_extra_bits(s)); fix += static_cast<uint64_t>(W.cnt[s]) * (png_fixed_ll_length(s) + png_ll_extra_bits(s)); }
    for (uint32_t s = 0; s < kPngD; ++s) { dyn += static_cast<uint64_t>(W.cnt[kPngLL + s]) * (W.len[kPngLL + s] + png_d_extra_bits(s)); fix += static_cast<uint64_t>(W.cnt[kPngLL + s]) * (5u + png_d_extra_bits(s)); }
    const uint64_t bits = 3u + (fix <= dyn ? fix : dyn);
    const uint64_t coded = last ? (bits + 7u) >> 3 : ((bits + 3u + 7u) >> 3) + 4u;
    const uint32_t type = stored_only || n_bytes + 5u <= coded ? 0u : fix <= dyn ? 1u : 2u;
    *type_out = type;
    for (uint32_t i = 0; i < kPngPrefixWords; ++i) W.prefix[i] = 0;
    W.prefix_bits = 0;
    if (type == 0u) return n_bytes + 5u;
    png_put(W.prefix, &W.prefix_bits, last ? 1u : 0u, 1);
    png_put(W.prefix, &W.prefix_bits, type, 2);
    if (type == 1u) {                                   // RFC 1951 3.2.6 (its alphabet has 288 symbols: the codes are written out)
        for (uint32_t s = 0; s < kPngLL; ++s) {
            const uint32_t l = png_fixed_ll_length(s), code = s < 144u ? 0x30u + s : s < 256u ? 0x190u + (s - 144u) : s < 280u ? s - 256u : 0xC0u + (s - 280u);
            W.tab[s] = png_reverse_bits(code, l) | (l << 16);
        }
        for (uint32_t s = 0; s < kPngD; ++s) W.tab[kPngLL + s] = png_reverse_bits(s, 5) | (5u << 16);
        return static_cast<uint32_t>(coded);
    } else {
        png_assign_codes(W, W.len + kPngLenCL, kPngCL, W.cltab);
        png_put(W.prefix, &W.prefix_bits, hlit - 257u, 5);
        png_put(W.prefix, &W.prefix_bits, hdist - 1u, 5);
        png_put(W.prefix, &W.prefix_bits, hclen - 4u, 4);
        for (uint32_t i = 0; i < hclen; ++i) png_put(W.prefix, &W.prefix_bits, W.len[kPngLenCL + png_cl_order(i)], 3);
        for (uint32_t i = 0; i < W.nrle; ++i) {
            const uint32_t s = W.rle[i] & 255u, e = W.rle[i] >> 8, t = W.cltab[s];
            png_put(W.prefix, &W.prefix_bits, t & 0xFFFFu, t >> 16);
            if (s >= 16u) png_put(W.prefix, &W.prefix_bits, e, s == 16u ? 2u : s == 17u ? 3u : 7u);
        }
    }
    png_assign_codes(W, W.len, kPngLL, W.tab);
    png_assign_codes(W, W.len + kPngLL, kPngD, W.tab + kPngLL);
    return static_cast<uint32_t>(coded);
}
// the bits of one token under the block's tables: value (low bit first) and count, at most 48
IFHIP_HD uint32_t png_token_bits(const uint32_t* tab, uint32_t tok, uint64_t* value) {
    const uint32_t len = tok >> 16;
    if (len == 0u) { const uint32_t t = tab[tok & 255u]; *value = t & 0xFFFFu; return t >> 16; }
    uint32_t sym, eb, ev;
    png_length_symbol(len, &sym, &eb, &ev);
    uint32_t t = tab[sym];
    uint64_t v = t & 0xFFFFu;
    uint32_t n = t >> 16;
    v |= static_cast<uint64_t>(ev) << n; n += eb;
    png_dist_symbol(tok & 0xFFFFu, &sym, &eb, &ev);
    t = tab[kPngLL + sym];
    v |= static_cast<uint64_t>(t & 0xFFFFu) << n; n += t >> 16;
    v |= static_cast<uint64_t>(ev) << n; n += eb;
    *value = v;
    return n;
}

// up to 48 bits of v ORed into a zeroed dword stream at bit position pos; or_word: how a word shared between lanes is ORed
template <typename Or>
IFHIP_HD void png_or_bits(uint32_t* words, uint32_t pos, uint64_t v, Or or_word) {
    const uint32_t w = pos >> 5, s = pos & 31u;
    const uint32_t w0 = static_cast<uint32_t>(v << s);
    const uint64_t rest = s ? v >> (32u - s) : v >> 32;
    if (w0) or_word(words + w, w0);
    if (static_cast<uint32_t>(rest)) or_word(words + w + 1u, static_cast<uint32_t>(rest));
    if (rest >> 32) or_word(words + w + 2u, static_cast<uint32_t>(rest >> 32));
}

// ---- checksums ----------------------------------------------------------------------------------------------------------------------
IFHIP_HD uint32_t png_crc_step(uint32_t crc, uint32_t byte) {         // the register, not the conditioned value
    crc ^= byte;
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    return crc;
}
IFHIP_HD uint32_t png_crc32(const uint8_t* p, uint32_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) c = png_crc_step(c, p[i]);
    return ~c;
}
// a * b modulo the CRC polynomial, both in the reflected representation (bit 31 is x^0)
IFHIP_HD uint32_t png_gf2_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return p;
}
// crc * x^(8 * len) modulo the polynomial, by square and multiply
IFHIP_HD uint32_t png_crc_shift(uint32_t crc, uint64_t len) {
    uint32_t p = 0x80000000u, b = 0x00800000u;                        // x^0, x^8
    for (; len; len >>= 1) {
        if (len & 1u) p = png_gf2_mul(b, p);
        b = png_gf2_mul(b, b);
    }
    return png_gf2_mul(p, crc);
}
// crc(A || B) from crc(A), crc(B) and len(B); the conditioning of the two cancels, so pieces combine by XOR of shifts
IFHIP_HD uint32_t png_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return png_crc_shift(crc_a, len_b) ^ crc_b; }

constexpr uint32_t kAdlerBase = 65521;
IFHIP_HD uint32_t png_adler32(const uint8_t* p, uint32_t n) {         // n <= 5552 (no reduction inside)
    uint32_t a = 1, b = 0;
    for (uint32_t i = 0; i < n; ++i) { a += p[i]; b += a; }
    return (a % kAdlerBase) | ((b % kAdlerBase) << 16);
}
IFHIP_HD uint32_t png_adler_combine(uint32_t ad1, uint32_t ad2, uint64_t len2) {
    const uint32_t rem = static_cast<uint32_t>(len2 % kAdlerBase);
    uint32_t s1 = ad1 & 0xFFFFu, s2 = (rem * s1) % kAdlerBase;
    s1 += (ad2 & 0xFFFFu) + kAdlerBase - 1u;
    s2 += (ad1 >> 16) + (ad2 >> 16) + kAdlerBase - rem;
    if (s1 >= kAdlerBase) s1 -= kAdlerBase;
    if (s1 >= kAdlerBase) s1 -= kAdlerBase;
    if (s2 >= (kAdlerBase << 1)) s2 -= (kAdlerBase << 1);
    if (s2 >= kAdlerBase) s2 -= kAdlerBase;
    return s1 | (s2 << 16);
}

// ---- the file's fixed parts ----------------------------------------------------------------------------------------------------------
IFHIP_HD uint32_t png_stream_pitch(uint32_t w, uint32_t bpp) { return 1u + w * bpp; }
IFHIP_HD uint32_t png_zlib_header(int level) {                        // CMF 0x78 (deflate, 32 KiB window), FLG as zlib sets it
    const uint32_t l = level < 0 || level > 9 ? 6u : static_cast<uint32_t>(level);
    const uint32_t flags = l < 2u ? 0u : l < 6u ? 1u : l == 6u ? 2u : 3u;
    uint32_t h = (0x78u << 8) | (flags << 6);
    h += 31u - h % 31u;
    return h;
}

IFHIP_HD void png_be32(uint8_t* p, uint32_t v) { p[0] = static_cast<uint8_t>(v >> 24); p[1] = static_cast<uint8_t>(v >> 16); p[2] = static_cast<uint8_t>(v >> 8); p[3] = static_cast<uint8_t>(v); }
// a chunk whose type (a big-endian FourCC) and data_len bytes of data are in place behind the 4 bytes of its length:
// writes the length in front and the CRC behind; returns the chunk's size
IFHIP_HD uint32_t png_close_chunk(uint8_t* chunk, uint32_t fourcc, uint32_t data_len) {
    png_be32(chunk, data_len);
    png_be32(chunk + 4, fourcc);
    png_be32(chunk + 8u + data_len, png_crc32(chunk + 4, 4u + data_len));
    return 12u + data_len;
}
constexpr uint32_t kPngHeadBytes = 8 + 25 + 16 + 13 + 44;
constexpr uint32_t kPngIDAT = 0x49444154u, kPngIEND = 0x49454E44u;
// signature, IHDR and what png_set_sRGB_gAMA_and_cHRM(.., PNG_sRGB_INTENT_PERCEPTUAL) adds in front of the first IDAT
// (codec_png_wrapper.c:402-415): gAMA 45455, sRGB 0, cHRM with the specification's sRGB primaries.  One lane.
IFHIP_HD void png_write_head(uint8_t* o, uint32_t w, uint32_t h, uint32_t color_type) {
    o[0] = 0x89; o[1] = 'P'; o[2] = 'N'; o[3] = 'G'; o[4] = 13; o[5] = 10; o[6] = 26; o[7] = 10;
    uint8_t* c = o + 8;
    png_be32(c + 8, w); png_be32(c + 12, h);
    c[16] = 8; c[17] = static_cast<uint8_t>(color_type); c[18] = 0; c[19] = 0; c[20] = 0;
    c += png_close_chunk(c, 0x49484452u, 13);                       // IHDR
    png_be32(c + 8, 45455u);
    c += png_close_chunk(c, 0x67414D41u, 4);                        // gAMA
    c[8] = 0;
    c += png_close_chunk(c, 0x73524742u, 1);                        // sRGB
    png_be32(c + 8, 31270u); png_be32(c + 12, 32900u); png_be32(c + 16, 64000u); png_be32(c + 20, 33000u);
    png_be32(c + 24, 30000u); png_be32(c + 28, 60000u); png_be32(c + 32, 15000u); png_be32(c + 36, 6000u);
    png_close_chunk(c, 0x6348524Du, 32);                            // cHRM
}

}  // namespace ifhip
