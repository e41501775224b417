// png_encode_core.hpp -- the arithmetic of the device PNG coder (csrc/png_encode.hip), written so that it compiles for the
// gfx950 kernels AND for a plain host compiler: tests/png_emulate.cpp runs the same filter choice, the same round-based
// parse, the same code construction and the same bit placement lane by lane on the CPU, and zlib must inflate what comes
// out -- test infrastructure; the product has one path, the kernels.
//
// What is coded: EncoderPreset::Libpng (imageflow_types/src/lib.rs:751-755, codecs/libpng_encoder.rs:43-72,134-160,
// c_components/lib/codec_png_wrapper.c:349-430): 8-bit RGB / RGBA, non-interlaced, libpng's default adaptive row filters,
// one zlib stream.  The deflate blocks are this coder's own (a parallel parse cannot equal zlib's serial one byte for
// byte); every rule with a bit in it -- RFC 1950 / 1951, the PNG specification -- lives here or, shared, in prefix_code_core.hpp.
#pragma once
#include <cstdint>

#include "prefix_code_core.hpp"

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
constexpr uint32_t kPngLL = 286, kPngD = 30, kPngSyms = kPngLL + kPngD;
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
IFHIP_HD void png_length_symbol(uint32_t len, uint32_t* sym, uint32_t* ebits, uint32_t* eval) {
    const uint32_t l = len - 3u;
    if (len == 258u) { *sym = 285u; *ebits = 0; *eval = 0; return; }
    if (l < 8u) { *sym = 257u + l; *ebits = 0; *eval = 0; return; }
    const uint32_t e = floor_log2(l) - 2u;
    *sym = 261u + 4u * e + ((l >> e) & 3u); *ebits = e; *eval = l & ((1u << e) - 1u);
}
IFHIP_HD void png_dist_symbol(uint32_t dist, uint32_t* sym, uint32_t* ebits, uint32_t* eval) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { *sym = d; *ebits = 0; *eval = 0; return; }
    const uint32_t e = floor_log2(d) - 1u;
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
// Workspace of one chunk's block (LDS on the device): the block's own state on top of the construction of its codes.
struct PngCodeWork : CodeWork {
    uint32_t cnt[kPngSyms + 4];      // in: literal/length counts [0, 286), distance counts [286, 316)
    uint32_t tab[kPngSyms + 4];      // out: bit-reversed code | length << 16 per symbol, of the block type chosen
    uint8_t len[kPngSyms + 4];       // the dynamic code lengths: literal/length, then distance
    uint32_t prefix[kPngPrefixWords];    // the block's first bits: BFINAL, BTYPE and the dynamic header
    uint32_t prefix_bits;
};
IFHIP_HD uint32_t png_cl_order(uint32_t i) {       // RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 8u - ((i - 3u) >> 1) : 8u + ((i - 4u) >> 1);
}
// The plan of one chunk's block, by one lane, from the counts and the dynamic lengths in W.len (code_build_lengths for the
// two alphabets): the dynamic header, the exact size of the block as dynamic, fixed and stored, the cheapest of the three,
// its code tables and its first bits.  A block that is not the stream's last is followed by an empty stored block, which
// closes it to a byte boundary (what a zlib sync flush writes: 3 bits, padding, 00 00 FF FF); a stored block starts on
// one and needs none.  Returns the chunk's bytes in the stream; *type_out: BTYPE.
IFHIP_HD uint32_t png_plan_block(PngCodeWork& W, uint32_t n_bytes, bool last, bool stored_only, uint32_t* type_out) {
    uint32_t hlit = kPngLL, hdist = kPngD;
    while (hlit > 257u && W.len[hlit - 1u] == 0) --hlit;
    while (hdist > 1u && W.len[kPngLL + hdist - 1u] == 0) --hdist;
    // one sequence of lengths: the hlit literal/length ones, then the hdist distance ones; behind HLIT, HDIST and HCLEN (14 bits)
    uint64_t fix = 0, dyn = 14u + code_plan_header(W, hlit + hdist, [&](uint32_t i) -> uint32_t { return W.len[i < hlit ? i : kPngLL + (i - hlit)]; }, png_cl_order);
    for (uint32_t s = 0; s < kPngLL; ++s) { dyn += static_cast<uint64_t>(W.cnt[s]) * (W.len[s] + png_ll_extra_bits(s)); fix += static_cast<uint64_t>(W.cnt[s]) * (png_fixed_ll_length(s) + png_ll_extra_bits(s)); }
    for (uint32_t s = 0; s < kPngD; ++s) { dyn += static_cast<uint64_t>(W.cnt[kPngLL + s]) * (W.len[kPngLL + s] + png_d_extra_bits(s)); fix += static_cast<uint64_t>(W.cnt[kPngLL + s]) * (5u + png_d_extra_bits(s)); }
    const uint64_t bits = 3u + (fix <= dyn ? fix : dyn);
    const uint64_t coded = last ? (bits + 7u) >> 3 : ((bits + 3u + 7u) >> 3) + 4u;
    const uint32_t type = stored_only || n_bytes + 5u <= coded ? 0u : fix <= dyn ? 1u : 2u;
    *type_out = type;
    for (uint32_t i = 0; i < kPngPrefixWords; ++i) W.prefix[i] = 0;
    W.prefix_bits = 0;
    if (type == 0u) return n_bytes + 5u;
    put_bits(W.prefix, &W.prefix_bits, last ? 1u : 0u, 1);
    put_bits(W.prefix, &W.prefix_bits, type, 2);
    if (type == 1u) {                                   // RFC 1951 3.2.6 (its alphabet has 288 symbols: the codes are written out)
        for (uint32_t s = 0; s < kPngLL; ++s) {
            const uint32_t l = png_fixed_ll_length(s), code = s < 144u ? 0x30u + s : s < 256u ? 0x190u + (s - 144u) : s < 280u ? s - 256u : 0xC0u + (s - 280u);
            W.tab[s] = reverse_bits(code, l) | (l << 16);
        }
        for (uint32_t s = 0; s < kPngD; ++s) W.tab[kPngLL + s] = reverse_bits(s, 5) | (5u << 16);
        return static_cast<uint32_t>(coded);
    }
    put_bits(W.prefix, &W.prefix_bits, hlit - 257u, 5);
    put_bits(W.prefix, &W.prefix_bits, hdist - 1u, 5);
    put_bits(W.prefix, &W.prefix_bits, W.hclen - 4u, 4);
    code_write_cl_lengths(W, W.prefix, &W.prefix_bits, png_cl_order);
    code_write_rle(W, W.prefix, &W.prefix_bits);
    code_assign_codes(W, W.len, kPngLL, W.tab);
    code_assign_codes(W, W.len + kPngLL, kPngD, W.tab + kPngLL);
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
