// prefix_code_core.hpp -- what the device coders that write prefix codes share (deflate: png_encode_core.hpp; VP8L, which
// took its codes from deflate: webp_encode_core.hpp), for the gfx950 kernels AND for a plain host compiler (the CPU
// emulations of the tests): length-limited Huffman lengths, canonical codes, the run-length coded header of a code's lengths
// (RFC 1951 3.2.7), bit placement.  The formats keep their alphabets, the order of the code-length code, the bits around the header.
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

// the largest alphabet (deflate: 286, VP8L: 280), the most lengths in one header (286 + 30), the code-length alphabet (0..15, 16 / 17 / 18)
constexpr uint32_t kCodeMaxSyms = 288, kCodeMaxLengths = 320, kCodeCL = 19;
IFHIP_HD uint32_t floor_log2(uint32_t v) { return 31u - static_cast<uint32_t>(__builtin_clz(v)); }

// Workspace of one code's construction and of its header (LDS on the device): nothing here is indexed from registers.
struct CodeWork {
    uint32_t wt[2 * kCodeMaxSyms];
    uint32_t nc[36];                 // codes per length, then the next code per length
    uint32_t clcnt[20], cltab[20];   // the code-length code: counts, then bit-reversed code | length << 16
    uint32_t nrle, hclen;            // header symbols in rle; lengths of the code-length code that are sent
    uint16_t sorted[kCodeMaxSyms];
    uint16_t parent[2 * kCodeMaxSyms];
    uint16_t rle[kCodeMaxLengths];   // header symbols: symbol | extra value << 8
    uint8_t cllen[20];               // the lengths of the code-length code
};

// rank of every used symbol in increasing (count, symbol) order -- the part of the sort one lane of `nlanes` does
IFHIP_HD void code_rank_sort_lane(const uint32_t* cnt, uint32_t n, uint32_t lane, uint32_t nlanes, uint16_t* sorted) {
    for (uint32_t s = lane; s < n; s += nlanes) {
        const uint32_t cs = cnt[s];
        if (!cs) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < n; ++t) { const uint32_t c = cnt[t]; r += (c && (c < cs || (c == cs && t < s))) ? 1u : 0u; }
        sorted[r] = static_cast<uint16_t>(s);
    }
}
// Code lengths of at most max_bits from counts (`sorted` filled by code_rank_sort_lane): Huffman's algorithm with two
// queues, then the depth histogram is moved under the limit the way zlib's gen_bitlen / miniz do (a code of the longest
// length below the limit is split, one of the limit is taken away, until the Kraft sum is 1 again) and the lengths are
// handed out again, longest to the rarest.  Fewer than two used symbols: the used one (else `lone`) gets one bit, and when
// `complete` a second symbol gets the other one-bit code.  Returns the number of used symbols.
IFHIP_HD uint32_t code_build_lengths(CodeWork& W, const uint32_t* cnt, uint32_t n, uint32_t max_bits, uint8_t* len, uint32_t lone, bool complete) {
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
IFHIP_HD uint32_t reverse_bits(uint32_t v, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1u - i);
    return r;
}
// canonical codes (RFC 1951 3.2.2), stored bit-reversed: a Huffman code enters the stream most significant bit first, and
// the writer packs everything from the low bit
IFHIP_HD void code_assign_codes(CodeWork& W, const uint8_t* len, uint32_t n, uint32_t* tab) {
    for (uint32_t b = 0; b < 18u; ++b) W.nc[b] = 0;
    for (uint32_t s = 0; s < n; ++s) W.nc[len[s]] += 1u;
    uint32_t code = 0;
    W.nc[0] = 0;
    for (uint32_t b = 1; b <= 15u; ++b) { code = (code + W.nc[b - 1u]) << 1; W.nc[18u + b] = code; }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = len[s];
        tab[s] = l ? (reverse_bits(W.nc[18u + l]++, l) | (l << 16)) : 0u;
    }
}

// ---- bit placement ---------------------------------------------------------------------------------------------------------------
// `nbits` (at most 32) bits of v at bit position *pos of a zeroed dword stream, low bit first; one writer
IFHIP_HD void put_bits(uint32_t* words, uint32_t* pos, uint32_t v, uint32_t nbits) {
    const uint64_t x = static_cast<uint64_t>(v) << (*pos & 31u);
    words[*pos >> 5] |= static_cast<uint32_t>(x);
    if (x >> 32) words[(*pos >> 5) + 1u] |= static_cast<uint32_t>(x >> 32);
    *pos += nbits;
}
// up to 64 bits of v ORed into a zeroed dword stream at bit position pos (32 bits wide where the stream is a workgroup's
// window, 64 where it is a file); or_word: how a word shared between writers is ORed
template <typename Pos, typename Or>
IFHIP_HD void or_bits(uint32_t* words, Pos pos, uint64_t v, Or or_word) {
    uint32_t* w = words + (pos >> 5);
    const uint32_t s = static_cast<uint32_t>(pos) & 31u;
    const uint32_t w0 = static_cast<uint32_t>(v << s);
    const uint64_t rest = s ? v >> (32u - s) : v >> 32;
    if (w0) or_word(w, w0);
    if (static_cast<uint32_t>(rest)) or_word(w + 1, static_cast<uint32_t>(rest));
    if (rest >> 32) or_word(w + 2, static_cast<uint32_t>(rest >> 32));
}

// ---- the header of a code's lengths (RFC 1951 3.2.7) -----------------------------------------------------------------------------
IFHIP_HD void code_rle_emit(CodeWork& W, uint32_t sym, uint32_t extra) {
    W.rle[W.nrle++] = static_cast<uint16_t>(sym | (extra << 8));
    W.clcnt[sym] += 1u;
}
IFHIP_HD uint32_t code_rle_extra_bits(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }
// The plan of the header of the n (at most kCodeMaxLengths) lengths length_at(0 .. n - 1), by one lane: run-length symbols
// (16: the previous length 3-6 times, used only behind that length itself; 17: 3-10 zeros; 18: 11-138 zeros) in W.rle,
// the code of the code lengths (complete, at most 7 bits) in W.cllen, and in W.hclen how many of its lengths are sent in
// the format's order cl_order(0 .. 18): at least 4, none behind the last that is not zero.  Returns the bits of the two
// parts the writers below write: W.hclen fields of 3 bits, and the symbols with their extra bits.
template <typename LengthAt, typename Order>
IFHIP_HD uint32_t code_plan_header(CodeWork& W, uint32_t n, LengthAt length_at, Order cl_order) {
    W.nrle = 0;
    for (uint32_t i = 0; i < 20u; ++i) W.clcnt[i] = 0;
    for (uint32_t i = 0; i < n;) {
        const uint32_t v = length_at(i);
        uint32_t run = 1;
        while (i + run < n && length_at(i + run) == v) ++run;
        i += run;
        if (v == 0u) {
            while (run >= 11u) { const uint32_t t = run < 138u ? run : 138u; code_rle_emit(W, 18u, t - 11u); run -= t; }
            if (run >= 3u) { code_rle_emit(W, 17u, run - 3u); run = 0; }
        } else {
            code_rle_emit(W, v, 0); --run;
            while (run >= 3u) { const uint32_t t = run < 6u ? run : 6u; code_rle_emit(W, 16u, t - 3u); run -= t; }
        }
        while (run > 0u) { code_rle_emit(W, v, 0); --run; }
    }
    code_rank_sort_lane(W.clcnt, kCodeCL, 0, 1, W.sorted);
    code_build_lengths(W, W.clcnt, kCodeCL, 7, W.cllen, 0, true);
    uint32_t hclen = kCodeCL;
    while (hclen > 4u && W.cllen[cl_order(hclen - 1u)] == 0) --hclen;
    W.hclen = hclen;
    uint32_t bits = 3u * hclen;
    for (uint32_t i = 0; i < W.nrle; ++i) { const uint32_t s = W.rle[i] & 255u; bits += W.cllen[s] + code_rle_extra_bits(s); }
    return bits;
}
// the first part of a planned header: the lengths of the code-length code (whose codes are assigned here)
template <typename Order>
IFHIP_HD void code_write_cl_lengths(CodeWork& W, uint32_t* words, uint32_t* pos, Order cl_order) {
    code_assign_codes(W, W.cllen, kCodeCL, W.cltab);
    for (uint32_t i = 0; i < W.hclen; ++i) put_bits(words, pos, W.cllen[cl_order(i)], 3);
}
// the second part: the run-length symbols under that code, with their extra bits
IFHIP_HD void code_write_rle(const CodeWork& W, uint32_t* words, uint32_t* pos) {
    for (uint32_t i = 0; i < W.nrle; ++i) {
        const uint32_t s = W.rle[i] & 255u, e = W.rle[i] >> 8, t = W.cltab[s];
        put_bits(words, pos, t & 0xFFFFu, t >> 16);
        if (s >= 16u) put_bits(words, pos, e, code_rle_extra_bits(s));
    }
}
// Four of these under the names they had in png_encode_core.hpp and webp_encode_core.hpp: sources written against those headers
// (the CPU emulations in the preceding revision's tests/) still compile.  Forwarders only; nothing in this tree calls them.
template <typename... A> IFHIP_HD void png_rank_sort_lane(A... a) { code_rank_sort_lane(a...); }
template <typename... A> IFHIP_HD uint32_t png_build_lengths(CodeWork& W, A... a) { return code_build_lengths(W, a...); }
template <typename Or> IFHIP_HD void png_or_bits(uint32_t* words, uint32_t pos, uint64_t v, Or or_word) { or_bits(words, pos, v, or_word); }
template <typename Or> IFHIP_HD void webp_or_bits(uint32_t* words, uint64_t pos, uint64_t v, Or or_word) { or_bits(words, pos, v, or_word); }

}  // namespace ifhip
