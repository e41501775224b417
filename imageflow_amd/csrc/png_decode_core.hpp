// png_decode_core.hpp -- the arithmetic of the device PNG decoder (csrc/png_decode.hip), written so that it compiles for the
// gfx950 kernels AND for a plain host compiler: tests/png_decode_emulate.cpp runs the same inflate (bit reader, code
// tables, token loop, window copies, flushes, Adler-32) and the same un-filter schedule lane by lane on the CPU, and
// zlib.decompress is the yardstick -- test infrastructure; the product has one path, the kernels.  csrc/png_read.cpp uses
// the same inflate on the host for the one thing that is not pixel data: a compressed iCCP profile.
//
// What is decoded: what libpng hands the reference after its transforms (c_components/lib/codec_png_wrapper.c:131-212,
// 215-246,266-292; imageflow_core/src/codecs/libpng_decoder.rs:36-104,297-299,340-383): all 15 legal (colour type, bit
// depth) pairs, interlaced or not, normalised to 8-bit BGRA.  Every rule with a bit in it -- RFC 1950 / 1951, zlib's
// inflate_table refusals, the PNG specification's filters, Adam7 and sample scaling -- lives here.
//
// How the inflate is written: standard deflate is serial per stream, so almost everything below is wave-UNIFORM code that
// every lane of the one wave runs identically (on the CPU: once).  The parts that are wave-wide go through an executor X:
//   X.lanes(f)   f(lane) for lanes 0..63, with a barrier in front and behind (CPU: a loop)
//   X.one(f)     f() on one lane, no barrier: LDS / memory writes of uniform code
//   X.sync()     a barrier (CPU: nothing)
// Wave-wide are the table fill, the staging of input, the copies (matches and stored blocks), the flush of the window to
// memory and the checksum's partial sums.
#pragma once
#include <cstdint>

#include "png_encode_core.hpp"

namespace ifhip {

enum : uint32_t {
    kPngDecOk = 0,
    kPngDecTruncated = 1,        // the stream ends inside a block, a header or the checksum
    kPngDecBlockType = 2,        // BTYPE 3
    kPngDecStoredLength = 3,     // LEN != ~NLEN
    kPngDecCodeLengths = 4,      // over-subscribed or incomplete set, a repeat with nothing to repeat or past the end, no end-of-block code
    kPngDecBadCode = 5,          // bits that are no code of the block's set, literal/length symbols 286/287, distance symbols 30/31
    kPngDecDistance = 6,         // a distance that reaches before the stream's start
    kPngDecZlibHeader = 7,       // CM != 8, window > 32 KiB, FCHECK, a preset dictionary
    kPngDecAdler = 8,            // Adler-32 mismatch
    kPngDecTooLittle = 9,        // the stream ended before the image was complete (libpng: "Not enough image data")
    kPngDecFilter = 10,          // a row's filter type above 4 (libpng: "bad adaptive filter value")
};

constexpr uint32_t kInfRing = 32768;         // the window (RFC 1951: distances reach 32 KiB back), an LDS ring
constexpr uint32_t kInfIn = 4096;            // staged input bytes held in LDS at a time
constexpr uint32_t kInfFlush = 8192;         // the window's new bytes go to memory whenever this many have gathered
constexpr uint32_t kInfFastBits = 10;        // codes up to this length decode by one table look-up
constexpr uint32_t kInfLanes = 64;

typedef uint32_t PngQuad __attribute__((vector_size(16)));       // 16 bytes moved as one value: a full-width load / store per lane

struct PngHuff {
    uint16_t fast[1u << kInfFastBits];   // symbol << 4 | length for every kInfFastBits-bit peek a code of that length starts; 0: longer, or none
    uint16_t count[16], first[16], offs[16], next[16];   // per length: codes, first canonical code, index of its first symbol; scratch
    uint16_t symbol[288];                // the used symbols in canonical order
};

struct PngInflateLds {
    PngQuad ring[kInfRing / 16u];
    PngQuad in[kInfIn / 16u + 1u];       // (one quad to spare: png_load4 reads a dword further)
    PngHuff ll, d;                       // d doubles as the code-length code while a dynamic header is read
    uint8_t lens[320];                   // code lengths: literal/length, then distance
    uint8_t cl_lens[20];
    uint8_t stage[260];                  // a match whose source and destination slots meet on the ring (dist + len > 32768)
    uint32_t part[kInfLanes][2];
    uint32_t bad;
};

struct PngInflateResult { uint32_t status, produced; };

// ---- symbols -> values (RFC 1951 3.2.5), the inverse of png_length_symbol / png_dist_symbol -----------------------------------
IFHIP_HD uint32_t png_length_base(uint32_t sym, uint32_t* ebits) {       // sym in [257, 285]
    if (sym < 265u) { *ebits = 0; return sym - 254u; }
    if (sym == 285u) { *ebits = 0; return 258u; }
    const uint32_t e = (sym - 261u) >> 2;
    *ebits = e;
    return 3u + ((4u + ((sym - 261u) & 3u)) << e);
}
IFHIP_HD uint32_t png_dist_base(uint32_t sym, uint32_t* ebits) {         // sym in [0, 29]
    if (sym < 4u) { *ebits = 0; return sym + 1u; }
    const uint32_t e = (sym >> 1) - 1u;
    *ebits = e;
    return 1u + ((2u + (sym & 1u)) << e);
}

// ---- code tables ------------------------------------------------------------------------------------------------------------------
// zlib's inflate_table rules: an over-subscribed set is refused; an incomplete one is refused unless it is a literal/length
// or distance set whose only code has one bit (so a single-code distance set passes); a distance set with no code at all
// passes too (a block of literals) -- every look-up in it is then an invalid code.  codes_type: the code-length code,
// where nothing incomplete passes.  Returns true when the set is refused.
template <typename X>
IFHIP_HD bool png_build_huff(X& x, PngHuff& H, const uint8_t* lens, uint32_t n, bool codes_type, uint32_t* bad_word) {
    x.sync();
    x.one([&] {
        for (uint32_t l = 0; l < 16u; ++l) H.count[l] = 0;
        for (uint32_t s = 0; s < n; ++s) H.count[lens[s]] += 1u;
        uint32_t max = 15;
        while (max > 0u && H.count[max] == 0) --max;
        int left = 1;
        bool bad = false;
        for (uint32_t l = 1; l < 16u; ++l) { left <<= 1; left -= static_cast<int>(H.count[l]); if (left < 0) { bad = true; break; } }
        if (max == 0u) bad = codes_type;
        else if (!bad && left > 0 && (codes_type || max != 1u)) bad = true;
        uint32_t code = 0, at = 0;
        H.count[0] = 0;
        for (uint32_t l = 1; l < 16u; ++l) {
            H.first[l] = static_cast<uint16_t>(code); H.offs[l] = H.next[l] = static_cast<uint16_t>(at);
            code = (code + H.count[l]) << 1; at += H.count[l];
        }
        if (!bad) for (uint32_t s = 0; s < n; ++s) { const uint32_t l = lens[s]; if (l) H.symbol[H.next[l]++] = static_cast<uint16_t>(s); }
        H.next[0] = static_cast<uint16_t>(bad ? 0u : at);                  // the number of used symbols
        *bad_word = bad ? 1u : 0u;
    });
    x.lanes([&](uint32_t lane) { for (uint32_t i = lane; i < (1u << kInfFastBits); i += kInfLanes) H.fast[i] = 0; });
    if (*bad_word) return true;
    x.lanes([&](uint32_t lane) {
        const uint32_t used = H.next[0];
        for (uint32_t i = lane; i < used; i += kInfLanes) {
            const uint32_t s = H.symbol[i], l = lens[s];
            if (l > kInfFastBits) continue;
            const uint32_t rev = reverse_bits(H.first[l] + (i - H.offs[l]), l);
            for (uint32_t k = rev; k < (1u << kInfFastBits); k += 1u << l) H.fast[k] = static_cast<uint16_t>(s << 4 | l);
        }
    });
    return false;
}
// One symbol from the low bits of `bits` (at least 15 valid or zero-filled): the symbol and its length in *len, or -1
IFHIP_HD int png_decode_symbol(const PngHuff& H, uint32_t bits, uint32_t* len) {
    const uint32_t e = H.fast[bits & ((1u << kInfFastBits) - 1u)];
    if (e) { *len = e & 15u; return static_cast<int>(e >> 4); }
    uint32_t code = 0, first = 0, index = 0;                               // the canonical walk, a bit at a time
    for (uint32_t l = 1; l < 16u; ++l) {
        code |= (bits >> (l - 1u)) & 1u;
        const uint32_t cnt = H.count[l];
        if (code < first + cnt) { *len = l; return H.symbol[index + (code - first)]; }
        index += cnt; first = (first + cnt) << 1; code <<= 1;
    }
    *len = 0;
    return -1;
}

// ---- the bit reader: bounded by the staged length -----------------------------------------------------------------------------------
// src: 16-byte aligned, readable in whole quads up to `len` rounded up to 16 (the host pads with zeros); nothing beyond is
// touched: quads past the end enter the LDS window as zeros, and using a bit that the stream does not have is kPngDecTruncated.
struct PngBits {
    const uint8_t* src;
    uint32_t len, base, pos, cnt;        // base: stream offset of the LDS window; pos: the next byte to enter buf; cnt: valid bits in buf
    uint64_t buf;
};
template <typename X>
IFHIP_HD void png_bits_window(X& x, PngInflateLds& S, PngBits& b, bool force) {
    if (!force && b.pos + 32u <= b.base + kInfIn) return;
    b.base = b.pos & ~15u;
    const uint32_t padded = (b.len + 15u) & ~15u, base = b.base;
    const PngQuad* src = reinterpret_cast<const PngQuad*>(b.src);
    x.lanes([&](uint32_t lane) {
        for (uint32_t q = lane; q < kInfIn / 16u + 1u; q += kInfLanes) {
            const uint32_t off = base + q * 16u;
            PngQuad v = {0u, 0u, 0u, 0u};
            if (off < padded) v = src[off >> 4];
            S.in[q] = v;
        }
    });
}
IFHIP_HD void png_bits_need32(const PngInflateLds& S, PngBits& b) {       // at least 32 valid (or zero-filled) bits in buf
    if (b.cnt >= 32u) return;
    const uint32_t v = png_load4(reinterpret_cast<const uint32_t*>(S.in), b.pos - b.base);
    b.buf |= static_cast<uint64_t>(v) << b.cnt;
    b.cnt += 32u; b.pos += 4u;
}
IFHIP_HD uint32_t png_bits_take(PngBits& b, uint32_t n) {                 // n <= 32, after png_bits_need32
    const uint32_t v = static_cast<uint32_t>(b.buf) & (n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u);
    b.buf >>= n; b.cnt -= n;
    return v;
}
IFHIP_HD bool png_bits_overrun(const PngBits& b) { return static_cast<uint64_t>(b.pos) * 8u - b.cnt > static_cast<uint64_t>(b.len) * 8u; }

// ---- output: the LDS ring, its flush and the checksum -----------------------------------------------------------------------------
struct PngOut {
    uint8_t* dst;                        // 16-byte aligned, writable in whole quads up to cap rounded up to 16
    uint32_t cap, pos, flushed;          // cap: the expected inflated size -- nothing beyond it is produced
    uint32_t a, b;                       // Adler-32 of [0, flushed)
};
// [flushed, to) goes to memory in quads (to: a multiple of 16, or the end); the checksum takes the bytes below pos
template <typename X>
IFHIP_HD void png_out_flush(X& x, PngInflateLds& S, PngOut& o, uint32_t to) {
    PngQuad* dst = reinterpret_cast<PngQuad*>(o.dst);
    const uint8_t* ring = reinterpret_cast<const uint8_t*>(S.ring);
    while (o.flushed < to) {
        const uint32_t from = o.flushed, quads = (to - from + 15u) >> 4, nq = quads < kInfLanes ? quads : kInfLanes;
        const uint32_t n = (o.pos - from) < nq * 16u ? (o.pos - from) : nq * 16u;       // bytes of this piece that count
        x.lanes([&](uint32_t lane) {
            uint32_t s1 = 0, s2 = 0;
            if (lane < nq) {
                const uint32_t at = from + lane * 16u;
                dst[at >> 4] = S.ring[(at & (kInfRing - 1u)) >> 4];
                for (uint32_t k = 0; k < 16u; ++k) {
                    const uint32_t i = lane * 16u + k, v = i < n ? ring[(at + k) & (kInfRing - 1u)] : 0u;
                    s1 += v; s2 += (n - i) * v;
                }
            }
            S.part[lane][0] = s1; S.part[lane][1] = s2;
        });
        uint32_t s1 = 0, s2 = 0;
        for (uint32_t l = 0; l < kInfLanes; ++l) { s1 += S.part[l][0]; s2 += S.part[l][1]; }
        o.b = (o.b + n * o.a + s2 % kAdlerBase) % kAdlerBase;              // n <= 1024: s2 < 2^28, n * a < 2^26
        o.a = (o.a + s1) % kAdlerBase;
        o.flushed = from + nq * 16u;
    }
}
template <typename X>
IFHIP_HD void png_out_maybe_flush(X& x, PngInflateLds& S, PngOut& o) {
    if (o.pos - o.flushed >= kInfFlush) png_out_flush(x, S, o, o.pos & ~15u);
}

// ---- inflate: one zlib stream by one wave ----------------------------------------------------------------------------------------------
// Produces at most `cap` bytes (the image's expected size).  A stream that holds more is cut there and is fine (libpng only
// warns "Too much image data", and never reaches the checksum); one that ends with less is kPngDecTooLittle; one that ends
// with exactly cap bytes has its Adler-32 checked.
template <typename X>
IFHIP_HD PngInflateResult png_inflate(X& x, PngInflateLds& S, const uint8_t* src, uint32_t len, uint8_t* dst, uint32_t cap) {
    PngBits b = {src, len, 0u, 0u, 0u, 0u};
    PngOut o = {dst, cap, 0u, 0u, 1u, 0u};
    uint8_t* ring = reinterpret_cast<uint8_t*>(S.ring);
    uint32_t status = kPngDecOk;
    bool cut = false;
    png_bits_window(x, S, b, true);
    png_bits_need32(S, b);
    {
        const uint32_t cmf = png_bits_take(b, 8), flg = png_bits_take(b, 8);
        if (png_bits_overrun(b)) status = kPngDecTruncated;
        else if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) status = kPngDecZlibHeader;
    }
    bool last = false;
    while (status == kPngDecOk && !last && !cut) {
        png_bits_window(x, S, b, false);
        png_bits_need32(S, b);
        last = png_bits_take(b, 1) != 0u;
        const uint32_t type = png_bits_take(b, 2);
        if (png_bits_overrun(b)) { status = kPngDecTruncated; break; }
        if (type == 3u) { status = kPngDecBlockType; break; }
        if (type == 0u) {
            png_bits_take(b, b.cnt & 7u);
            png_bits_need32(S, b);
            const uint32_t ln = png_bits_take(b, 16), nln = png_bits_take(b, 16);
            if (png_bits_overrun(b)) { status = kPngDecTruncated; break; }
            if ((ln ^ nln) != 0xFFFFu) { status = kPngDecStoredLength; break; }
            uint32_t p = b.pos - (b.cnt >> 3);                             // the stored bytes start here
            if (static_cast<uint64_t>(p) + ln > len) { status = kPngDecTruncated; break; }
            uint32_t left = ln;
            while (left > 0u && !cut) {
                uint32_t n = left < 4096u ? left : 4096u;
                if (n > o.cap - o.pos) { n = o.cap - o.pos; cut = true; }
                const uint32_t at = o.pos, from = p;
                x.lanes([&](uint32_t lane) { for (uint32_t j = lane; j < n; j += kInfLanes) ring[(at + j) & (kInfRing - 1u)] = src[from + j]; });
                o.pos += n; p += n; left -= n;
                png_out_maybe_flush(x, S, o);
            }
            b.pos = p; b.cnt = 0; b.buf = 0;
            png_bits_window(x, S, b, true);
            continue;
        }
        if (type == 1u) {                                                  // RFC 1951 3.2.6 (288 and 32 symbols: 286/287 and 30/31 are refused when met)
            x.sync();
            x.lanes([&](uint32_t lane) { for (uint32_t s = lane; s < 320u; s += kInfLanes) S.lens[s] = static_cast<uint8_t>(s < 288u ? png_fixed_ll_length(s) : 5u); });
            png_build_huff(x, S.ll, S.lens, 288u, false, &S.bad);
            png_build_huff(x, S.d, S.lens + 288u, 32u, false, &S.bad);
        } else {
            const uint32_t hlit = png_bits_take(b, 5) + 257u, hdist = png_bits_take(b, 5) + 1u, hclen = png_bits_take(b, 4) + 4u;
            if (hlit > 286u || hdist > 30u) { status = kPngDecCodeLengths; break; }       // zlib: "too many length or distance symbols"
            x.sync();
            x.one([&] { for (uint32_t i = 0; i < 19u; ++i) S.cl_lens[i] = 0; });
            for (uint32_t i = 0; i < hclen; ++i) {
                png_bits_need32(S, b);
                const uint32_t v = png_bits_take(b, 3);
                x.one([&] { S.cl_lens[png_cl_order(i)] = static_cast<uint8_t>(v); });
            }
            if (png_bits_overrun(b)) { status = kPngDecTruncated; break; }
            if (png_build_huff(x, S.d, S.cl_lens, 19u, true, &S.bad)) { status = kPngDecCodeLengths; break; }
            const uint32_t total = hlit + hdist;
            uint32_t i = 0, prev = 0;
            while (i < total && status == kPngDecOk) {
                png_bits_window(x, S, b, false);
                png_bits_need32(S, b);
                uint32_t l;
                const int sym = png_decode_symbol(S.d, static_cast<uint32_t>(b.buf), &l);
                if (sym < 0) { status = png_bits_overrun(b) ? kPngDecTruncated : kPngDecBadCode; break; }
                png_bits_take(b, l);
                uint32_t rep = 1, val = static_cast<uint32_t>(sym);
                if (sym == 16) { if (i == 0u) { status = kPngDecCodeLengths; break; } val = prev; rep = 3u + png_bits_take(b, 2); }
                else if (sym == 17) { val = 0; rep = 3u + png_bits_take(b, 3); }
                else if (sym == 18) { val = 0; rep = 11u + png_bits_take(b, 7); }
                if (png_bits_overrun(b)) { status = kPngDecTruncated; break; }
                if (i + rep > total) { status = kPngDecCodeLengths; break; }
                const uint32_t at = i;
                x.one([&] { for (uint32_t k = 0; k < rep; ++k) { const uint32_t s = at + k; S.lens[s < hlit ? s : 288u + (s - hlit)] = static_cast<uint8_t>(val); } });
                i += rep; prev = val;
            }
            if (status != kPngDecOk) break;
            x.sync();
            if (S.lens[256] == 0) { status = kPngDecCodeLengths; break; }   // zlib: "invalid code -- missing end-of-block"
            if (png_build_huff(x, S.ll, S.lens, hlit, false, &S.bad)) { status = kPngDecCodeLengths; break; }
            if (png_build_huff(x, S.d, S.lens + 288u, hdist, false, &S.bad)) { status = kPngDecCodeLengths; break; }
        }
        // the token loop
        for (;;) {
            png_bits_window(x, S, b, false);
            png_bits_need32(S, b);
            uint32_t l, eb;
            const int sym = png_decode_symbol(S.ll, static_cast<uint32_t>(b.buf), &l);
            if (sym < 0 || sym > 285) { status = png_bits_overrun(b) ? kPngDecTruncated : kPngDecBadCode; break; }
            png_bits_take(b, l);
            if (png_bits_overrun(b)) { status = kPngDecTruncated; break; }
            if (sym == 256) break;
            if (sym < 256) {
                if (o.pos >= o.cap) { cut = true; break; }
                const uint32_t at = o.pos;
                x.one([&] { ring[at & (kInfRing - 1u)] = static_cast<uint8_t>(sym); });
                o.pos += 1u;
            } else {
                uint32_t n = png_length_base(static_cast<uint32_t>(sym), &eb);
                n += png_bits_take(b, eb);
                png_bits_need32(S, b);
                const int ds = png_decode_symbol(S.d, static_cast<uint32_t>(b.buf), &l);
                if (ds < 0 || ds > 29) { status = png_bits_overrun(b) ? kPngDecTruncated : kPngDecBadCode; break; }
                png_bits_take(b, l);
                uint32_t dist = png_dist_base(static_cast<uint32_t>(ds), &eb);
                dist += png_bits_take(b, eb);
                if (png_bits_overrun(b)) { status = kPngDecTruncated; break; }
                if (dist > o.pos) { status = kPngDecDistance; break; }
                if (o.pos >= o.cap) { cut = true; break; }
                if (n > o.cap - o.pos) { n = o.cap - o.pos; cut = true; }
                // Every byte of the match is a byte from before it: with dist >= n one step, else the dist bytes as a
                // repeating pattern.  On the 32 KiB ring the slot byte j is read from is the slot byte j + (32768 - dist) of
                // the SAME match is written to.  With dist + n <= 32768 no such byte exists: nothing read is written, and the
                // lanes need no order among themselves.  A longer reach (dist in (32768 - 258, 32768): libdeflate, zopfli
                // and 7-zip write such matches, zlib never does) goes through a staging row -- all bytes are read, a
                // barrier, all are written -- so that this copy too is independent of the order the lanes run in.
                const uint32_t at = o.pos, whole = dist >= n ? 1u : 0u;
                if (dist + n <= kInfRing) {
                    x.lanes([&](uint32_t lane) {
                        for (uint32_t j = lane; j < n; j += kInfLanes)
                            ring[(at + j) & (kInfRing - 1u)] = ring[(at - dist + (whole ? j : j % dist)) & (kInfRing - 1u)];
                    });
                } else {                                                     // (dist > 32768 - 258 >= n: one step)
                    x.lanes([&](uint32_t lane) { for (uint32_t j = lane; j < n; j += kInfLanes) S.stage[j] = ring[(at - dist + j) & (kInfRing - 1u)]; });
                    x.lanes([&](uint32_t lane) { for (uint32_t j = lane; j < n; j += kInfLanes) ring[(at + j) & (kInfRing - 1u)] = S.stage[j]; });
                }
                o.pos += n;
                if (cut) break;
            }
            if (o.pos - o.flushed >= kInfFlush) png_out_flush(x, S, o, o.pos & ~15u);
        }
    }
    x.sync();
    png_out_flush(x, S, o, o.pos);
    if (status == kPngDecOk && !cut) {
        if (o.pos < o.cap) status = kPngDecTooLittle;
        else {
            png_bits_window(x, S, b, false);
            png_bits_take(b, b.cnt & 7u);
            png_bits_need32(S, b);
            const uint32_t v = png_bits_take(b, 32);
            const uint32_t want = (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
            if (png_bits_overrun(b)) status = kPngDecTruncated;
            else if (want != ((o.b << 16) | o.a)) status = kPngDecAdler;
        }
    }
    return PngInflateResult{status, o.pos};
}

// ---- geometry (PNG specification 7.2, 8.2, 9.2) -------------------------------------------------------------------------------------
IFHIP_HD uint32_t png_channels(uint32_t color_type) { return color_type == 2u ? 3u : color_type == 4u ? 2u : color_type == 6u ? 4u : 1u; }
IFHIP_HD bool png_legal_type(uint32_t ct, uint32_t depth) {
    if (ct == 0u) return depth == 1u || depth == 2u || depth == 4u || depth == 8u || depth == 16u;
    if (ct == 3u) return depth == 1u || depth == 2u || depth == 4u || depth == 8u;
    return (ct == 2u || ct == 4u || ct == 6u) && (depth == 8u || depth == 16u);
}
// bytes per complete pixel, rounded up to one: what the filters call "the corresponding byte of the pixel to the left"
IFHIP_HD uint32_t png_filter_bpp(uint32_t ct, uint32_t depth) { const uint32_t b = png_channels(ct) * depth / 8u; return b ? b : 1u; }
IFHIP_HD uint64_t png_row_bytes(uint32_t w, uint32_t ct, uint32_t depth) { return (static_cast<uint64_t>(w) * png_channels(ct) * depth + 7u) / 8u; }
// Adam7 pass p (0..6): first column / row and the steps, a nibble per pass
IFHIP_HD uint32_t png_pass_x0(uint32_t p) { return (0x0102040u >> (4u * p)) & 15u; }
IFHIP_HD uint32_t png_pass_y0(uint32_t p) { return (0x1020400u >> (4u * p)) & 15u; }
IFHIP_HD uint32_t png_pass_dx(uint32_t p) { return (0x1224488u >> (4u * p)) & 15u; }
IFHIP_HD uint32_t png_pass_dy(uint32_t p) { return (0x2244888u >> (4u * p)) & 15u; }
IFHIP_HD uint32_t png_pass_width(uint32_t w, uint32_t p) { const uint32_t x0 = png_pass_x0(p), dx = png_pass_dx(p); return w > x0 ? (w - x0 + dx - 1u) / dx : 0u; }
IFHIP_HD uint32_t png_pass_height(uint32_t h, uint32_t p) { const uint32_t y0 = png_pass_y0(p), dy = png_pass_dy(p); return h > y0 ? (h - y0 + dy - 1u) / dy : 0u; }
// the pass pixel (x, y) of an interlaced image belongs to
IFHIP_HD uint32_t png_pass_of(uint32_t x, uint32_t y) {
    if ((y & 7u) == 0u && (x & 7u) == 0u) return 0u;
    if ((y & 7u) == 0u && (x & 7u) == 4u) return 1u;
    if ((y & 7u) == 4u && (x & 3u) == 0u) return 2u;
    if ((y & 3u) == 0u && (x & 3u) == 2u) return 3u;
    if ((y & 3u) == 2u && (x & 1u) == 0u) return 4u;
    if ((y & 1u) == 0u) return 5u;
    return 6u;
}
// the filtered bytes of one (sub-)image: a filter byte and the row, per row; an empty pass has none
IFHIP_HD uint64_t png_image_bytes(uint32_t w, uint32_t h, uint32_t ct, uint32_t depth) { return w && h ? (1u + png_row_bytes(w, ct, depth)) * h : 0u; }
IFHIP_HD uint64_t png_inflated_size(uint32_t w, uint32_t h, uint32_t ct, uint32_t depth, uint32_t interlace) {
    if (!interlace) return png_image_bytes(w, h, ct, depth);
    uint64_t n = 0;
    for (uint32_t p = 0; p < 7u; ++p) n += png_image_bytes(png_pass_width(w, p), png_pass_height(h, p), ct, depth);
    return n;
}

// ---- un-filter (PNG specification 9.2), on pixels: bpp bytes in the low end of a 64-bit word ---------------------------------------
// x: the filtered pixel, a: the un-filtered one to the left, b: above, c: above left (0 outside the image); f: 0..4
IFHIP_HD uint64_t png_unfilter_pixel(uint32_t f, uint64_t x, uint64_t a, uint64_t b, uint64_t c, uint32_t bpp) {
    uint64_t r = 0;
    for (uint32_t k = 0; k < 8u; ++k) {
        if (k >= bpp) break;
        const uint32_t s = 8u * k, xa = static_cast<uint32_t>(a >> s) & 255u, xb = static_cast<uint32_t>(b >> s) & 255u, xc = static_cast<uint32_t>(c >> s) & 255u;
        const uint32_t pred = f == 0u ? 0u : f == 1u ? xa : f == 2u ? xb : f == 3u ? (xa + xb) >> 1 : png_paeth(xa, xb, xc);
        r |= static_cast<uint64_t>((static_cast<uint32_t>(x >> s) + pred) & 255u) << s;
    }
    return r;
}
IFHIP_HD uint64_t png_load_pixel(const uint8_t* p, uint32_t bpp) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < 8u; ++k) { if (k >= bpp) break; v |= static_cast<uint64_t>(p[k]) << (8u * k); }
    return v;
}
IFHIP_HD void png_store_pixel(uint8_t* p, uint64_t v, uint32_t bpp) {
    for (uint32_t k = 0; k < 8u; ++k) { if (k >= bpp) break; p[k] = static_cast<uint8_t>(v >> (8u * k)); }
}

// ---- samples -> BGRA: libpng's transforms in the order the reference sets them (codec_png_wrapper.c:131-212) --------------------------
// expand (palette -> RGB, gray 1/2/4 -> 8 by bit replication, tRNS -> alpha with the key compared at the FILE's depth), filler
// 0xFF, strip 16 -> 8 by the high byte, gray -> RGB, BGR.
struct PngExpand {
    uint32_t color_type, depth, has_trns;
    uint32_t key[3];                     // the tRNS key of gray (key[0]) / RGB files, at the file's depth
};
IFHIP_HD uint32_t png_sample(const uint8_t* row, uint32_t idx, uint32_t depth) {
    if (depth == 8u) return row[idx];
    if (depth == 16u) return static_cast<uint32_t>(row[2u * idx]) << 8 | row[2u * idx + 1u];
    const uint32_t bit = idx * depth;
    return (row[bit >> 3] >> (8u - depth - (bit & 7u))) & ((1u << depth) - 1u);
}
IFHIP_HD uint32_t png_sample_to8(uint32_t v, uint32_t depth) { return depth == 16u ? v >> 8 : depth == 8u ? v : depth == 4u ? v * 17u : depth == 2u ? v * 85u : v * 255u; }
// pixel x of an un-filtered row as a BGRA dword (B in the low byte); palette: 256 BGRA entries with tRNS applied
IFHIP_HD uint32_t png_expand_pixel(const PngExpand& e, const uint32_t* palette, const uint8_t* row, uint32_t x) {
    const uint32_t d = e.depth;
    if (e.color_type == 3u) return palette[png_sample(row, x, d)];
    if (e.color_type == 0u || e.color_type == 4u) {
        const bool ga = e.color_type == 4u;
        const uint32_t g = png_sample(row, ga ? 2u * x : x, d), g8 = png_sample_to8(g, d);
        const uint32_t a = ga ? png_sample_to8(png_sample(row, 2u * x + 1u, d), d) : (e.has_trns && g == e.key[0]) ? 0u : 255u;
        return g8 | g8 << 8 | g8 << 16 | a << 24;
    }
    const uint32_t n = e.color_type == 6u ? 4u : 3u;
    const uint32_t r = png_sample(row, n * x, d), g = png_sample(row, n * x + 1u, d), b = png_sample(row, n * x + 2u, d);
    const uint32_t a = n == 4u ? png_sample_to8(png_sample(row, n * x + 3u, d), d) : (e.has_trns && r == e.key[0] && g == e.key[1] && b == e.key[2]) ? 0u : 255u;
    return png_sample_to8(b, d) | png_sample_to8(g, d) << 8 | png_sample_to8(r, d) << 16 | a << 24;
}

}  // namespace ifhip
