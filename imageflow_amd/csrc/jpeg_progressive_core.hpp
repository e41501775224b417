// jpeg_progressive_core.hpp -- the entropy decoder of progressive (SOF2) Huffman JPEG files, stated once for the gfx950 kernels
// (csrc/jpeg_progressive_decode.hip) and for the CPU (tests/jpeg_progressive_emulate.cpp), in the manner of gif_decode_core.hpp:
// the records a batch is laid out in, the Huffman table every lookup reads, the four block decoders of libjpeg's jdphuff.c
// (decode_mcu_DC_first, _AC_first, _DC_refine, _AC_refine) exactly as csrc/jpeg_read.cpp states them -- the `<< Al` through
// uint32_t and the int16 casts included -- and the walk of one *stream* (the bits of one restart interval of one scan) by one
// wave.  No HIP in here beyond the two function attributes: the wave is a template parameter.
//
// The wave.  A stream is a serial chain -- a symbol's length says where the next one starts -- and a lone lane pays a full memory
// round trip per symbol (jpeg_entropy.hip, walk_wave: ~400 cycles).  So the 64 lanes look up, at once, the symbol that WOULD
// start d bits behind the current position, d = 0..63 (`ProgWalk::window`), and the chain symbol -> skip -> next symbol is then
// resolved by wave-uniform code that reads lane `pos` of that window (readlane on the device, an array index on the CPU).
// Wave is the policy: Var<T> a value per lane, lanes(f) runs f(lane) on every lane, ballot(f) the 64-bit mask of f(lane),
// sync() the barrier between a write to the workgroup's scratch and its reading by other lanes, raise() the file's status word.
// Everything that steers control flow is wave-uniform.
//
// What bounds each access.  Stream words are read through the stage only, and the stage is filled by ProgWalk::restage, which
// compares every word index with the block's total (`n_words`) and reads 0 beyond it; a stage index is at most 6 words behind
// the window's first word and the window is re-staged kProgStageAhead words before the stage's end.  A stream ends by its MCU
// count; a symbol that ends behind the stream's last bit raises kProgOutOfBits before anything of it is stored.  Every block
// address comes from prog_block, which compares the block's column with the plane's width and its index with the plane's size
// (blocks_w x blocks_h, which the entry point has compared with the bytes the CALLER gave).  A pending end-of-band run is cut
// at the stream's block count.  Table reads: the first level by 9 bits of the window, the search by (code + valoff) & 255.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define IFHIP_PROG_HD __host__ __device__ inline
#else
#define IFHIP_PROG_HD inline
#endif

namespace ifhip {

enum : uint32_t { kProgDcFirst = 0, kProgDcRefine = 1, kProgAcFirst = 2, kProgAcRefine = 3 };
// the status word of a file: 0 = decoded.  (IFHIP_JPEG_PROG_* in include/imageflow_hip_jpeg_progressive.h are these.)
enum : uint32_t { kProgNoSuchCode = 1, kProgPastSe = 2, kProgRefineSize = 4, kProgOutOfBits = 8, kProgBounds = 16 };

constexpr uint32_t kProgLutBits = 9, kProgLutEntries = 1u << kProgLutBits;
constexpr uint32_t kProgWave = 64;
constexpr uint32_t kProgStageWords = 1024;      // the stream's window in the workgroup's scratch: 4 KB, 32768 bits
constexpr uint32_t kProgStageAhead = 8;         // words behind the window's first that one window's work may read (6, see above)
constexpr uint32_t kProgMaxBlocksInMcu = 6;     // chroma is 1x1 (jpeg_markers.hpp chroma_is_1x1): 2x2 + 1 + 1

// A Huffman table: the first level answers codes of up to 9 bits with one read -- (symbol << 8) | length, 0: longer -- and
// jdhuff.c's maxcode / valoff search the rest (lengths 10..16; seven compares, no dependent loads).
struct ProgTable {
    uint32_t lut[kProgLutEntries];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t vals[256];
};
constexpr uint32_t kProgInvalid = 0xFFu;        // length field of "no such code"

struct ProgFileRec {
    uint64_t coef[3];                           // the caller's planes
    uint64_t plane_blocks[3];                   // blocks_w x blocks_h of each (the caller's plane holds at least that: prog_layout_batch)
    uint32_t bw[3];                             // plane width in blocks
    uint32_t ncomp;
};
struct ProgScanRec {
    uint32_t file, kind, ns;
    uint32_t Ss, Se, Al;
    uint32_t raster_w;                          // MCUs (interleaved) or blocks (one component: jdinput.c per_scan_setup) in a row
    uint32_t bpm;                               // blocks per MCU
    uint32_t tab[3];                            // table of scan component s, an index into the batch's tables
    uint8_t comp[4], nh[4], nv[4];              // per scan component: frame component, blocks of an MCU across and down
    uint8_t kslot[8], kdx[8], kdy[8];           // block k of an MCU: scan component and place inside the MCU
};
// The bits of one restart interval of one scan, FF00 un-stuffed, from a 32-bit boundary of the batch's words: start state
// (predictors 0, end-of-band run 0), first MCU, MCU count.  A later change that cuts the Ah = 0 streams into self-synchronising
// sub-sequences adds records that point INTO a stream (word0 / n_bits stay what they are); nothing here assumes one wave a stream.
struct ProgStreamRec {
    uint32_t scan;
    uint32_t n_bits;
    uint64_t word0;
    uint32_t first_mcu, n_mcu;
};
struct ProgArgs {
    const ProgFileRec* files;
    const ProgScanRec* scans;
    const ProgStreamRec* streams;
    const ProgTable* tables;
    const uint32_t* words;
    uint64_t n_words;
    uint32_t* status;
    uint32_t n_files;
};

// zigzag position -> natural (row-major) position (a function-local table: the same statement compiles for host and device)
IFHIP_PROG_HD uint32_t prog_natural(uint32_t k) {
    constexpr uint8_t t[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                               15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63u];
}

// jdhuff.c jpeg_make_d_derived_tbl from a DHT's counts and values.  false: not a prefix code (libjpeg: JERR_BAD_HUFF_TABLE).
inline bool prog_build_table(const uint8_t bits[17], const uint8_t vals[256], ProgTable* t) {
    std::memset(t, 0, sizeof *t);
    std::memcpy(t->vals, vals, 256);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t->valoff[l] = k - code;
        if (code + bits[l] > (1 << l)) return false;
        for (int i = 0; i < bits[l]; ++i, ++k, ++code)
            if (l <= static_cast<int>(kProgLutBits)) {
                const uint32_t first = static_cast<uint32_t>(code) << (kProgLutBits - l);
                for (uint32_t f = 0; f < (1u << (kProgLutBits - l)); ++f) t->lut[first + f] = (static_cast<uint32_t>(vals[k & 255]) << 8) | static_cast<uint32_t>(l);
            }
        t->maxcode[l] = bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    if (k > 256) return false;
    t->maxcode[0] = -1; t->maxcode[17] = 0x7fffffff;
    t->valoff[0] = t->valoff[17] = 0;
    return true;
}

// The symbol whose code starts at the top of `win`: (symbol << 8) | code length, length kProgInvalid where no code does.
IFHIP_PROG_HD uint32_t prog_lookup(const ProgTable* t, uint32_t win) {
    uint32_t e = t->lut[win >> (32u - kProgLutBits)];
    if (e & 255u) return e;
    e = kProgInvalid;
    for (uint32_t l = 16u; l > kProgLutBits; --l) {                      // the FIRST length whose code is in range: the last hit of a downward loop
        const int32_t code = static_cast<int32_t>(win >> (32u - l));
        if (code <= t->maxcode[l]) e = (static_cast<uint32_t>(t->vals[(code + t->valoff[l]) & 255]) << 8) | l;
    }
    return e;
}

// jdhuff.c HUFF_EXTEND of the s bits r, s in 1..15
IFHIP_PROG_HD int32_t prog_extend(uint32_t r, uint32_t s) { return r < (1u << (s - 1u)) ? static_cast<int32_t>(r) - static_cast<int32_t>((1u << s) - 1u) : static_cast<int32_t>(r); }
// the n bits (1..15) that follow the first `len` (<= 16) of a window
IFHIP_PROG_HD uint32_t prog_bits_behind(uint32_t win, uint32_t len, uint32_t n) { return (win << len) >> (32u - n); }
// decode_mcu_DC_first / _AC_first: the value a coefficient is stored as
IFHIP_PROG_HD int16_t prog_shifted(int32_t v, uint32_t Al) { return static_cast<int16_t>(static_cast<uint32_t>(v) << Al); }
// decode_mcu_AC_refine: one correction bit for a coefficient that is already nonzero
IFHIP_PROG_HD int16_t prog_correct(int16_t c, uint32_t bit, uint32_t Al) {
    const int32_t p1 = 1 << Al, m1 = -(1 << Al);
    if (bit && (c & p1) == 0) return static_cast<int16_t>(c >= 0 ? c + p1 : c + m1);
    return c;
}
IFHIP_PROG_HD uint64_t prog_range(uint32_t a, uint32_t b) {             // bits a..b, a <= b + 1, b <= 63
    if (a > b) return 0ull;
    const uint64_t hi = b >= 63u ? ~0ull : ((1ull << (b + 1u)) - 1ull);
    return hi & ~((1ull << a) - 1ull);
}
IFHIP_PROG_HD uint32_t prog_popc(uint64_t m) { return static_cast<uint32_t>(__builtin_popcountll(m)); }
IFHIP_PROG_HD uint32_t prog_ctz(uint64_t m) { return static_cast<uint32_t>(__builtin_ctzll(m)); }            // m != 0

// Block k of MCU m of a scan.  false: outside the component's plane (never, for the records the front
// end writes: a stream's MCUs lie inside the scan's raster and the raster inside the plane).
IFHIP_PROG_HD bool prog_block(const ProgFileRec& f, const ProgScanRec& sc, uint32_t m, uint32_t k, int16_t** out) {
    const uint32_t slot = sc.kslot[k], ci = sc.comp[slot];
    const uint32_t my = m / sc.raster_w, mx = m - my * sc.raster_w;
    const uint32_t bx = mx * sc.nh[slot] + sc.kdx[k], by = my * sc.nv[slot] + sc.kdy[k];
    const uint64_t idx = static_cast<uint64_t>(by) * f.bw[ci] + bx;
    if (bx >= f.bw[ci] || idx >= f.plane_blocks[ci]) return false;
    *out = reinterpret_cast<int16_t*>(f.coef[ci]) + idx * 64u;
    return true;
}

// ---- one stream, one wave ---------------------------------------------------------------------------------------------------------
template <class W>
struct ProgWalk {
    W& w;
    const ProgArgs& a;
    const ProgStreamRec st;                      // (a copy: stores to the planes do not make the compiler read it again)
    uint32_t* stage;                             // kProgStageWords of the workgroup's scratch
    uint32_t base = 0;                           // stream word held by stage[0]
    bool staged = false;
    uint32_t p = 0;                              // the window's bit position in the stream
    typename W::template Var<uint32_t> e, win;   // lane d: the symbol that would start at p + d, and the 32 bits from there
    typename W::template Var<uint32_t> nat;      // lane z: the natural position of zigzag coefficient z (read by lane: no memory on a symbol's chain)

    IFHIP_PROG_HD ProgWalk(W& w_, const ProgArgs& a_, const ProgStreamRec& st_, uint32_t* stage_) : w(w_), a(a_), st(st_), stage(stage_) {
        w.lanes([&](uint32_t lane) { nat[lane] = prog_natural(lane); });
    }

    IFHIP_PROG_HD void restage() {
        w.sync();                                                        // (the lanes have read what the stage held)
        base = p >> 5;
        w.lanes([&](uint32_t lane) {
            for (uint32_t t = lane; t < kProgStageWords; t += kProgWave) {
                const uint64_t gi = st.word0 + base + t;                 // bound: the block's words, zeros behind them
                stage[t] = gi < a.n_words ? a.words[gi] : 0u;
            }
        });
        w.sync();
        staged = true;
    }
    // move the window to p + pos (the bits up to there are consumed) and look the 64 symbols up again
    IFHIP_PROG_HD void window(const ProgTable* tab, uint32_t pos) {
        p += pos;
        if (!staged || (p >> 5) + kProgStageAhead > base + kProgStageWords) restage();
        w.lanes([&](uint32_t d) {
            const uint32_t q = p + d, i = (q >> 5) - base, sh = q & 31u;   // i + 1 <= (p >> 5) + 3 - base < kProgStageWords - 4
            const uint32_t hi = stage[i], lo = stage[i + 1u];
            uint32_t v = sh ? (hi << sh) | (lo >> (32u - sh)) : hi;
            // zeros behind the stream's last bit (the words there are a neighbour's): what a stream raises depends on it alone
            const uint32_t left = q < st.n_bits ? st.n_bits - q : 0u;
            v = left >= 32u ? v : (left ? v & ~(0xFFFFFFFFu >> left) : 0u);
            win[d] = v;
            e[d] = prog_lookup(tab, v);
        });
    }
    // bit q of the stream, p <= q < p + 160 (five words behind the window's first: inside the stage by window()'s margin)
    IFHIP_PROG_HD uint32_t bit(uint32_t q) const { return (stage[(q >> 5) - base] >> (31u - (q & 31u))) & 1u; }
};

// decode_mcu_DC_first over the stream's MCUs.  -> status flags
template <class W>
IFHIP_PROG_HD uint32_t prog_walk_dc_first(ProgWalk<W>& k, const ProgFileRec& f, const ProgScanRec& sc, const ProgTable* tabs) {
    W& w = k.w;
    const uint64_t total = static_cast<uint64_t>(k.st.n_mcu) * sc.bpm;
    uint32_t pred[3] = {0u, 0u, 0u};                                     // (unsigned: the sum wraps as the host's does in practice, without UB)
    uint32_t kin = 0, m = k.st.first_mcu;
    for (uint64_t j = 0; j < total;) {
        const uint32_t slot = sc.kslot[kin];
        k.window(tabs + slot, 0u);
        uint32_t pos = 0;
        for (;;) {
            const uint32_t es = k.e.read(pos), ws = k.win.read(pos);
            const uint32_t len = es & 255u, sym = es >> 8;
            if (len == kProgInvalid || sym > 15u) return kProgNoSuchCode;
            const int32_t diff = sym ? prog_extend(prog_bits_behind(ws, len, sym), sym) : 0;
            pos += len + sym;
            if (k.p + pos > k.st.n_bits) return kProgOutOfBits;
            const uint32_t ci = sc.comp[slot];
            pred[ci] += static_cast<uint32_t>(diff);
            int16_t* blk;
            if (!prog_block(f, sc, m, kin, &blk)) return kProgBounds;
            const int16_t v = prog_shifted(static_cast<int32_t>(pred[ci]), sc.Al);
            w.lanes([&](uint32_t lane) { if (lane == 0u) blk[0] = v; });
            ++j;
            if (++kin == sc.bpm) { kin = 0; ++m; }
            if (j >= total || sc.kslot[kin] != slot || pos >= kProgWave) break;
        }
        k.p += pos;
    }
    return 0u;
}

// decode_mcu_DC_refine: closed form -- block j of the stream owns bit j -- one lane per block
template <class W>
IFHIP_PROG_HD uint32_t prog_walk_dc_refine(ProgWalk<W>& k, const ProgFileRec& f, const ProgScanRec& sc) {
    W& w = k.w;
    const uint64_t total = static_cast<uint64_t>(k.st.n_mcu) * sc.bpm;
    if (total > k.st.n_bits) return kProgOutOfBits;
    typename W::template Var<uint32_t> bad;
    w.lanes([&](uint32_t lane) { bad[lane] = 0u; });
    for (uint64_t j0 = 0; j0 < total; j0 += kProgWave)
        w.lanes([&](uint32_t lane) {
            const uint64_t j = j0 + lane;
            if (j >= total) return;
            const uint64_t gi = k.st.word0 + (j >> 5);                   // bound: j < n_bits, and the block's words all the same
            const uint32_t word = gi < k.a.n_words ? k.a.words[gi] : 0u;
            if (!((word >> (31u - (static_cast<uint32_t>(j) & 31u))) & 1u)) return;
            const uint32_t m = k.st.first_mcu + static_cast<uint32_t>(j / sc.bpm), kin = static_cast<uint32_t>(j % sc.bpm);
            int16_t* blk;
            if (!prog_block(f, sc, m, kin, &blk)) { bad[lane] = 1u; return; }
            blk[0] = static_cast<int16_t>(blk[0] | (1 << sc.Al));
        });
    return w.ballot([&](uint32_t lane) { return bad[lane] != 0u; }) ? kProgBounds : 0u;
}

// decode_mcu_AC_first: one component, the band Ss..Se; the chain runs on across blocks (one table), an end-of-band run
// skips its blocks without a look at them
template <class W>
IFHIP_PROG_HD uint32_t prog_walk_ac_first(ProgWalk<W>& k, const ProgFileRec& f, const ProgScanRec& sc, const ProgTable* tab) {
    W& w = k.w;
    const uint32_t total = k.st.n_mcu, Ss = sc.Ss, Se = sc.Se;
    uint32_t j = 0, z = Ss, pos = 0;
    int16_t* blk = nullptr;
    while (j < total) {
        k.window(tab, pos);
        pos = 0;
        while (j < total && pos < kProgWave) {
            const uint32_t es = k.e.read(pos), ws = k.win.read(pos);
            const uint32_t len = es & 255u, sym = es >> 8;
            if (len == kProgInvalid) return kProgNoSuchCode;
            const uint32_t r = sym >> 4, sz = sym & 15u;
            uint32_t skip_blocks = 0;
            if (sz) {
                z += r;
                if (z > Se) return kProgPastSe;
                pos += len + sz;
                if (k.p + pos > k.st.n_bits) return kProgOutOfBits;
                if (!blk && !prog_block(f, sc, k.st.first_mcu + j, 0u, &blk)) return kProgBounds;
                const int16_t v = prog_shifted(prog_extend(prog_bits_behind(ws, len, sz), sz), sc.Al);
                const uint32_t nat = k.nat.read(z);
                int16_t* const dst = blk;
                w.lanes([&](uint32_t lane) { if (lane == 0u) dst[nat] = v; });
                if (++z > Se) skip_blocks = 1u;
            } else if (r == 15u) {
                z += 16u;
                if (z > Se) return kProgPastSe;                          // (a ZRL stands in front of a coefficient)
                pos += len;
                if (k.p + pos > k.st.n_bits) return kProgOutOfBits;
            } else {
                const uint32_t run = (1u << r) + (r ? prog_bits_behind(ws, len, r) : 0u);
                pos += len + r;
                if (k.p + pos > k.st.n_bits) return kProgOutOfBits;
                skip_blocks = run;                                       // this block and run - 1 behind it
            }
            if (skip_blocks) {
                j = skip_blocks > total - j ? total : j + skip_blocks;   // the run is cut at the stream's end
                z = Ss;
                blk = nullptr;
            }
        }
    }
    return 0u;
}

// decode_mcu_AC_refine.  Lane z owns zigzag coefficient z of the block (128 bytes of the plane, complete since the launch of
// the level before); a ballot gives the nonzero history of the band; a symbol's run is "the (r+1)-th zero at or behind z" and
// its correction bits "the nonzero ones in front of that", both bit counts on the mask; every lane takes its own correction
// bit; the lanes whose value changed store it, once.
template <class W>
IFHIP_PROG_HD uint32_t prog_walk_ac_refine(ProgWalk<W>& k, const ProgFileRec& f, const ProgScanRec& sc, const ProgTable* tab) {
    W& w = k.w;
    const uint32_t total = k.st.n_mcu, Ss = sc.Ss, Se = sc.Se, Al = sc.Al;
    const int16_t p1 = static_cast<int16_t>(1 << Al), m1 = static_cast<int16_t>(-(1 << Al));
    typename W::template Var<int16_t> c, c0;
    uint32_t eobrun = 0, pos = 0;
    k.window(tab, 0u);
    for (uint32_t j = 0; j < total; ++j) {
        int16_t* blk;
        if (!prog_block(f, sc, k.st.first_mcu + j, 0u, &blk)) return kProgBounds;
        w.lanes([&](uint32_t lane) {
            c0[lane] = (lane >= Ss && lane <= Se) ? blk[k.nat[lane]] : static_cast<int16_t>(0);
            c[lane] = c0[lane];
        });
        const uint64_t nz = w.ballot([&](uint32_t lane) { return c0[lane] != 0; });
        uint32_t z = Ss;
        uint32_t status = 0;
        // corrections for the nonzero coefficients of `cm`, their bits from stream position q on, in zigzag order
        auto correct = [&](uint64_t cm, uint32_t q) {
            w.lanes([&](uint32_t lane) {
                if ((cm >> lane) & 1ull) c[lane] = prog_correct(c[lane], k.bit(q + prog_popc(cm & ((1ull << lane) - 1ull))), Al);
            });
        };
        if (eobrun == 0u) {
            while (z <= Se) {
                if (pos >= kProgWave) { k.window(tab, pos); pos = 0; }
                const uint32_t es = k.e.read(pos), ws = k.win.read(pos);
                const uint32_t len = es & 255u, sym = es >> 8;
                if (len == kProgInvalid) { status = kProgNoSuchCode; break; }
                const uint32_t r = sym >> 4, sz = sym & 15u;
                if (sz > 1u) { status = kProgRefineSize; break; }
                if (!sz && r != 15u) {                                   // EOBr: the rest of the block is the end-of-band logic below
                    eobrun = (1u << r) + (r ? prog_bits_behind(ws, len, r) : 0u);
                    pos += len + r;
                    break;
                }
                const uint32_t hdr = len + sz;                           // the code and, for a new coefficient, its sign
                // the (r+1)-th zero of the band at or behind z
                const uint64_t zeros = ~nz & prog_range(z, Se);
                const uint64_t hit = w.ballot([&](uint32_t lane) { return ((zeros >> lane) & 1ull) != 0ull && prog_popc(zeros & ((1ull << lane) - 1ull)) == r; });
                if (!hit) { status = kProgPastSe; break; }               // (neither a coefficient nor a ZRL may run out of the band)
                const uint32_t t = prog_ctz(hit);
                const uint64_t cm = nz & prog_range(z, t) ;
                const uint32_t ncorr = prog_popc(cm);
                if (k.p + pos + hdr + ncorr > k.st.n_bits) { status = kProgOutOfBits; break; }
                correct(cm, k.p + pos + hdr);
                if (sz) {
                    const int16_t v = ((ws << len) >> 31) ? p1 : m1;
                    w.lanes([&](uint32_t lane) { if (lane == t) c[lane] = v; });
                }
                pos += hdr + ncorr;
                z = t + 1u;
            }
            if (status) return status;
            if (k.p + pos > k.st.n_bits) return kProgOutOfBits;
        }
        if (eobrun > 0u) {
            if (pos >= kProgWave) { k.window(tab, pos); pos = 0; }       // (the stage follows: the corrections are read from it)
            const uint64_t cm = nz & prog_range(z, Se);
            const uint32_t ncorr = prog_popc(cm);
            if (k.p + pos + ncorr > k.st.n_bits) return kProgOutOfBits;
            correct(cm, k.p + pos);
            pos += ncorr;
            --eobrun;
        }
        w.lanes([&](uint32_t lane) { if (c[lane] != c0[lane]) blk[k.nat[lane]] = c[lane]; });
    }
    return 0u;
}

// One workgroup (= one wave) of a level's launch: stream `si`.  scratch: the workgroup's, kProgScratchBytes.
constexpr uint32_t kProgScratchBytes = 3u * static_cast<uint32_t>(sizeof(ProgTable)) + kProgStageWords * 4u;
template <class W>
IFHIP_PROG_HD void prog_stream_workgroup(W& w, const ProgArgs& a, uint32_t si, uint8_t* scratch) {
    const ProgStreamRec& st = a.streams[si];
    const ProgScanRec& sc = a.scans[st.scan];
    const ProgFileRec& f = a.files[sc.file];
    // (a damaged file's later streams run all the same: what they do depends on the file alone -- streams of one level write
    // disjoint coefficients whatever their bits say -- so the status word is the same on every run, and in the CPU form)
    ProgTable* tabs = reinterpret_cast<ProgTable*>(scratch);
    uint32_t* stage = reinterpret_cast<uint32_t*>(scratch + 3u * sizeof(ProgTable));
    if (sc.kind != kProgDcRefine) {
        const uint32_t nt = sc.kind == kProgDcFirst ? sc.ns : 1u;
        w.lanes([&](uint32_t lane) {
            for (uint32_t t = 0; t < nt; ++t) {
                const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tables + sc.tab[t]);
                uint32_t* dst = reinterpret_cast<uint32_t*>(tabs + t);
                for (uint32_t i = lane; i < sizeof(ProgTable) / 4u; i += kProgWave) dst[i] = src[i];
            }
        });
        w.sync();
    }
    ProgWalk<W> k(w, a, st, stage);
    uint32_t status;
    switch (sc.kind) {
        case kProgDcFirst: status = prog_walk_dc_first(k, f, sc, tabs); break;
        case kProgDcRefine: status = prog_walk_dc_refine(k, f, sc); break;
        case kProgAcFirst: status = prog_walk_ac_first(k, f, sc, tabs); break;
        default: status = prog_walk_ac_refine(k, f, sc, tabs); break;
    }
    if (status) w.raise(a.status + sc.file, status);
}

// The clear: thread `t` of `n_threads` over plane (file, comp); the first thread of a file's first plane zeroes its status word.
IFHIP_PROG_HD void prog_clear_thread(const ProgArgs& a, uint32_t file, uint32_t comp, uint64_t t, uint64_t n_threads) {
    const ProgFileRec& f = a.files[file];
    if (comp == 0u && t == 0u) a.status[file] = 0u;
    if (comp >= f.ncomp) return;
    uint64_t* dst = reinterpret_cast<uint64_t*>(f.coef[comp]);           // (planes are 8-byte aligned: the entry point's check)
    const uint64_t n = f.plane_blocks[comp] * 16u;                       // bound: the plane as the caller sized it
    for (uint64_t i = t; i < n; i += n_threads) dst[i] = 0ull;
}

// ---- the CPU form of the wave and of every launch ----------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
struct ProgCpuWave {
    template <typename T> struct Var {
        T v[kProgWave];
        T& operator[](uint32_t lane) { return v[lane]; }
        T read(uint32_t lane) const { return v[lane]; }
    };
    template <typename F> void lanes(F f) { for (uint32_t lane = 0; lane < kProgWave; ++lane) f(lane); }
    template <typename F> uint64_t ballot(F f) { uint64_t m = 0; for (uint32_t lane = 0; lane < kProgWave; ++lane) if (f(lane)) m |= 1ull << lane; return m; }
    void sync() {}
    void raise(uint32_t* word, uint32_t flags) { *word |= flags; }
};
// level_first[l] .. level_first[l + 1]: the streams of level l.  clear_grid_x x 256 threads clear a plane, as the device does.
inline void jpeg_progressive_decode_batch_cpu(const ProgArgs& a, const uint32_t* level_first, uint32_t n_levels, uint32_t clear_grid_x) {
    for (uint32_t y = 0; y < a.n_files * 3u; ++y)
        for (uint64_t t = 0; t < static_cast<uint64_t>(clear_grid_x) * 256u; ++t) prog_clear_thread(a, y / 3u, y % 3u, t, static_cast<uint64_t>(clear_grid_x) * 256u);
    for (uint32_t l = 0; l < n_levels; ++l)
        for (uint32_t si = level_first[l]; si < level_first[l + 1u]; ++si) {
            alignas(16) uint8_t scratch[kProgScratchBytes];
            std::memset(scratch, 0xA5, sizeof scratch);                  // LDS is not cleared on the device either
            ProgCpuWave w;
            prog_stream_workgroup(w, a, si, scratch);
        }
}
#endif

}  // namespace ifhip
