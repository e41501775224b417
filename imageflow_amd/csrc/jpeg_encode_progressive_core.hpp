// jpeg_encode_progressive_core.hpp -- the arithmetic of the device entropy coder for the libjpeg_turbo preset's two options
// (optimize_huffman_coding, progressive), restating csrc/jpeg_write.cpp (Progressive, run_scan, gen_optimal_table and the
// marker order of jpeg_write -- byte-identical to libjpeg-turbo's jcphuff.c / jchuff.c) in lane-sized pieces that compile
// for the gfx950 kernels (csrc/jpeg_encode_progressive.hip) AND for a plain host compiler: tests/enc_progressive_emulate.cpp
// runs the same routines pass by pass on the CPU.
//
// An image is a list of scans (ProgPlan): one interleaved sequential scan for IFHIP_JPEG_OPTIMIZE_HUFFMAN alone, the 10 (6 for
// gray) scans of jpeg_simple_progression for IFHIP_JPEG_PROGRESSIVE.  Every (scan, block) pair is an ITEM; the passes:
//   A  classify   per item: its own symbols ("head") into the scan's histograms; does it end in an end-of-band ("tail"), and
//                 with how many correction bits (AC refinement)
//   R  runs       per maximal sequence of tails with no head between: cut greedily at 0x7FFF blocks / more than 937 buffered
//                 correction bits; the EOBn symbol is charged to the run's first block (eob[item] = run length) and counted
//   T  tables     jpeg_gen_optimal_table per (image, scan, table)
//   C  count      bits per item with the tables -> prefix sums per scan
//   W  write      every item's bits (head, EOBn field when a run starts here, the tail's correction bits) are contiguous
//   then the 0xFF count / stuffing passes, every scan a stream of its own that starts on a chunk boundary of the word stream.
#pragma once
#include <cstdint>

#include "jpeg_encode_core.hpp"

namespace ifhip {

constexpr uint32_t kProgMaxScans = 10, kProgMaxSlots = 10;
constexpr uint32_t kProgSeq = 0, kProgDcFirst = 1, kProgDcRefine = 2, kProgAcFirst = 3, kProgAcRefine = 4;
constexpr uint32_t kProgNoSlot = 0xFFu;
constexpr uint32_t kProgRunChunk = 2048;            // blocks per wave of the run pass (a run is walked by the wave whose chunk it starts in)
constexpr uint32_t kProgDhtPitch = 288;             // a DHT segment: marker, length, class | id, 16 counts, up to 256 values = 277 bytes
constexpr uint32_t kProgMaxDht = 277, kProgMaxSos = 14, kProgMaxHeader0 = 2 + 18 + 2 * 69 + 19;
constexpr uint32_t kProgEobLimit = 0x7FFF;          // jcphuff.c: the longest end-of-band run
constexpr uint32_t kProgCorrLimit = 1000 - 64 + 1;  // the host writer's `be.size() > 1000 - 64 + 1`: flush when MORE bits than this wait

struct ProgScan {
    uint32_t kind, comp, Ss, Se, Ah, Al;
    uint32_t nblocks, wb, pitch;    // items of the scan; AC scans: the component's own width in blocks and its plane's pitch
    float rcp_wb;
    uint32_t wg0, item0, chunk0;    // first workgroup of the block passes, first item, first chunk of the run pass (AC scans)
    uint32_t slot[4];               // table slots dc0, ac0, dc1, ac1 (kProgNoSlot: not used by this scan)
    uint32_t ndht, dht[4];          // the slots whose DHT segments precede the scan, in jcmarker.c's order
    uint32_t sos_len;
    uint8_t sos[16];
};
struct ProgPlan {
    uint32_t nscans, nslots, n_wg, n_items, n_chunks, progressive;
    uint32_t header0_len, sof_marker_at;            // SOI .. SOF: the baseline header's first bytes, with the SOF marker patched to SOF2
    uint8_t slot_id[kProgMaxSlots];                 // class << 4 | table id
    ProgScan scan[kProgMaxScans];
};

// the most bits one block can take in a scan (codes of at most 16 bits; an EOBn field of 16 + 14 bits charged to it)
IFHIP_HD uint32_t prog_worst_bits(const ProgScan& s) {
    const uint32_t band = s.Se - s.Ss + 1u;
    switch (s.kind) {
    case kProgSeq: return kEncMaxBitsPerBlock;
    case kProgDcFirst: return 16u + 11u;
    case kProgDcRefine: return 1u;
    case kProgAcFirst: return band * (16u + 10u) + 30u;
    default: return band * 17u + 4u * 16u + 30u + 63u;   // new coefficients (code + sign), ZRLs, EOBn, correction bits
    }
}

// Host: the scans of an image.  flags: 1 optimise, 2 progressive (which implies 1).
inline void prog_make_plan(const EncGeom& g, uint32_t width, uint32_t height, int flags, ProgPlan* p) {
    *p = ProgPlan{};
    const bool progressive = (flags & 2) != 0;
    p->progressive = progressive ? 1u : 0u;
    const uint32_t nc = g.ncomp, ntab = nc == 3u ? 2u : 1u;
    p->sof_marker_at = 2u + 18u + 69u * ntab + 1u;
    p->header0_len = 2u + 18u + 69u * ntab + 2u + 2u + 6u + 3u * nc;
    struct S { int ncomp, comp, Ss, Se, Ah, Al; };
    static const S color[10] = {{3, 0, 0, 0, 0, 1}, {1, 0, 1, 5, 0, 2}, {1, 2, 1, 63, 0, 1}, {1, 1, 1, 63, 0, 1}, {1, 0, 6, 63, 0, 2},
                                {1, 0, 1, 63, 2, 1}, {3, 0, 0, 0, 1, 0}, {1, 2, 1, 63, 1, 0}, {1, 1, 1, 63, 1, 0}, {1, 0, 1, 63, 1, 0}};
    static const S gray[6] = {{1, 0, 0, 0, 0, 1}, {1, 0, 1, 5, 0, 2}, {1, 0, 6, 63, 0, 2}, {1, 0, 1, 63, 2, 1}, {1, 0, 0, 0, 1, 0}, {1, 0, 1, 63, 1, 0}};
    const S seq{static_cast<int>(nc), 0, 0, 63, 0, 0};
    const S* script = progressive ? (nc == 3u ? color : gray) : &seq;
    p->nscans = progressive ? (nc == 3u ? 10u : 6u) : 1u;
    uint32_t hmax = 1, vmax = 1;
    for (uint32_t c = 0; c < nc; ++c) { hmax = g.H[c] > hmax ? g.H[c] : hmax; vmax = g.V[c] > vmax ? g.V[c] : vmax; }
    for (uint32_t j = 0; j < p->nscans; ++j) {
        const S& s = script[j];
        ProgScan& d = p->scan[j];
        d.comp = static_cast<uint32_t>(s.comp); d.Ss = static_cast<uint32_t>(s.Ss); d.Se = static_cast<uint32_t>(s.Se);
        d.Ah = static_cast<uint32_t>(s.Ah); d.Al = static_cast<uint32_t>(s.Al);
        const bool dc_scan = s.Ss == 0, ac_scan = s.Se > 0;
        d.kind = dc_scan && ac_scan ? kProgSeq : dc_scan ? (s.Ah ? kProgDcRefine : kProgDcFirst) : (s.Ah ? kProgAcRefine : kProgAcFirst);
        for (int i = 0; i < 4; ++i) d.slot[i] = kProgNoSlot;
        if (dc_scan) {                              // MCU order (a single component's MCU is one block: jcmaster.c)
            d.nblocks = g.nblocks; d.wb = g.mcus_w; d.pitch = g.pitch[0];
        } else {                                    // the component's own size in blocks, not the MCU-padded plane
            const uint32_t c = d.comp;
            d.wb = (width * g.H[c] + hmax * 8u - 1u) / (hmax * 8u);
            d.nblocks = d.wb * ((height * g.V[c] + vmax * 8u - 1u) / (vmax * 8u));
            d.pitch = g.pitch[c];
        }
        d.rcp_wb = 1.0f / static_cast<float>(d.wb);
        d.wg0 = p->n_wg; d.item0 = p->n_items; d.chunk0 = p->n_chunks;
        p->n_wg += (d.nblocks + kEncBlocksPerWg - 1u) / kEncBlocksPerWg;
        p->n_items += d.nblocks;
        if (!dc_scan) p->n_chunks += (d.nblocks + kProgRunChunk - 1u) / kProgRunChunk;
        // jcmarker.c write_scan_header: the tables of the scan's components in component order, DC then AC, each once
        const bool needs_dc = dc_scan && s.Ah == 0, needs_ac = ac_scan;
        uint8_t* b = d.sos;
        *b++ = 0xFF; *b++ = 0xDA; *b++ = 0; *b++ = static_cast<uint8_t>(6 + 2 * s.ncomp); *b++ = static_cast<uint8_t>(s.ncomp);
        for (int i = 0; i < s.ncomp; ++i) {
            const uint32_t c = s.ncomp > 1 ? static_cast<uint32_t>(i) : d.comp, t = c ? 1u : 0u;
            if (needs_dc && d.slot[2u * t] == kProgNoSlot) { p->slot_id[p->nslots] = static_cast<uint8_t>(t); d.dht[d.ndht++] = d.slot[2u * t] = p->nslots++; }
            if (needs_ac && d.slot[2u * t + 1u] == kProgNoSlot) { p->slot_id[p->nslots] = static_cast<uint8_t>(0x10u | t); d.dht[d.ndht++] = d.slot[2u * t + 1u] = p->nslots++; }
            // jcmarker.c emit_sos: a progressive scan names only the table it uses
            const uint32_t td = progressive ? (needs_dc ? t : 0u) : t, ta = progressive ? (ac_scan ? t : 0u) : t;
            *b++ = static_cast<uint8_t>(c + 1u); *b++ = static_cast<uint8_t>((td << 4) | ta);
        }
        *b++ = static_cast<uint8_t>(s.Ss); *b++ = static_cast<uint8_t>(s.Se); *b++ = static_cast<uint8_t>((s.Ah << 4) | s.Al);
        d.sos_len = static_cast<uint32_t>(b - d.sos);
    }
}

// The unstuffed entropy-coded bytes of an image at worst, summed over its scans (every scan padded to a byte).
inline uint64_t prog_worst_stream_bytes(const ProgPlan& p) {
    uint64_t sum = 0;
    for (uint32_t j = 0; j < p.nscans; ++j) sum += (static_cast<uint64_t>(p.scan[j].nblocks) * prog_worst_bits(p.scan[j]) + 7u) / 8u;
    return sum;
}
// everything of a file that is not entropy-coded data, at most
inline uint64_t prog_segment_bytes(const ProgPlan& p) {
    return kProgMaxHeader0 + static_cast<uint64_t>(p.nscans) * kProgMaxSos + static_cast<uint64_t>(p.nslots) * kProgMaxDht + 2u;
}

// Where an item's block lies (offset in blocks inside the component's plane) and the block that predicts its DC value.
IFHIP_HD EncBlockRef prog_locate(const EncGeom& g, const ProgScan& sc, uint32_t s) {
    if (sc.kind <= kProgDcRefine) return enc_locate(g, s);
    const uint32_t by = enc_div(s, sc.wb, sc.rcp_wb), bx = s - by * sc.wb;
    return EncBlockRef{sc.comp, by * sc.pitch + bx, 0xFFFFFFFFu};
}

// ---- the block routines -------------------------------------------------------------------------------------------------
// |low half| >> al, |high half| >> al of a dword of two coefficients (-32768 counts as 32768 and is refused by the range check)
IFHIP_HD uint32_t prog_pair_abs_shift(uint32_t w, uint32_t al) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t n, a;
    asm("v_pk_sub_i16 %0, %1, %2" : "=v"(n) : "v"(0u), "v"(w));
    asm("v_pk_max_i16 %0, %1, %2" : "=v"(a) : "v"(n), "v"(w));
    asm("v_pk_lshrrev_b16 %0, %1, %2" : "=v"(a) : "v"(al * 0x00010001u), "v"(a));
    return a;
#else
    const int32_t lo = static_cast<int16_t>(w & 0xffffu), hi = static_cast<int16_t>(w >> 16);
    const uint32_t a = static_cast<uint32_t>(lo < 0 ? -lo : lo) >> al, b = static_cast<uint32_t>(hi < 0 ? -hi : hi) >> al;
    return a | b << 16;
#endif
}
// Masks of the zigzag positions (position k at bit 63 - k) whose magnitude after the point transform is not zero / is one.
// No branch per coefficient: the flag pairs of the 32 staged dwords are shifted into two registers (jpeg_encode_core.hpp).
template <class Coef>
IFHIP_HD void prog_masks(const Coef& coef, uint32_t al, uint64_t* nonzero, uint64_t* one) {
    uint32_t hn = 0, ln = 0, hg = 0, lg = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t a = prog_pair_abs_shift(coef.pair(j), al);
        hn = (hn << 1) | enc_pair_flags(a);
        hg = (hg << 1) | enc_pair_flags((a >> 1) & 0x7fff7fffu);
    }
#pragma unroll
    for (int j = 16; j < 32; ++j) {
        const uint32_t a = prog_pair_abs_shift(coef.pair(j), al);
        ln = (ln << 1) | enc_pair_flags(a);
        lg = (lg << 1) | enc_pair_flags((a >> 1) & 0x7fff7fffu);
    }
    hn = (hn << 16) | (hn >> 16); ln = (ln << 16) | (ln >> 16);
    hg = (hg << 16) | (hg >> 16); lg = (lg << 16) | (lg >> 16);
    *nonzero = static_cast<uint64_t>(hn) << 32 | ln;
    *one = *nonzero & ~(static_cast<uint64_t>(hg) << 32 | lg);
}
IFHIP_HD uint64_t prog_band(uint32_t Ss, uint32_t Se) { return (~0ull >> Ss) & (~0ull << (63u - Se)); }

// what a block routine reports: bit 0 head (it put a symbol of its own), bit 1 tail (it ends in an end-of-band), bits 2..7
// the tail's correction bits, bit 8 a coefficient out of range
constexpr uint32_t kProgHead = 1, kProgTail = 2, kProgBad = 256;
IFHIP_HD uint32_t prog_ncorr(uint32_t f) { return (f >> 2) & 63u; }

// Outputs: sym(symbol, extra bits, n extra) and raw(bits, n), n <= 32.
template <class Sink>
struct ProgCoded {                  // against a table of 256 `code | length << 16`
    Sink& s;
    const uint32_t* tab;
    IFHIP_HD void sym(uint32_t symbol, uint32_t extra, uint32_t n) {
        const uint32_t cs = tab[symbol];
        s.put(((cs & 0xffffu) << n) | extra, (cs >> 16) + n);
    }
    IFHIP_HD void raw(uint32_t v, uint32_t n) { s.put(v, n); }
};
template <class Add>
struct ProgCounted {                // statistics: Add::one(&histogram[symbol])
    uint32_t* hist;
    IFHIP_HD void sym(uint32_t symbol, uint32_t, uint32_t) { Add::add(hist + symbol, 1u); }
    IFHIP_HD void raw(uint32_t, uint32_t) {}
};
// enc_block's statistics: run against the identity table (entry i = i, length 0), a field is `symbol << n | extra` of length n
template <class Add>
struct EncStatSink {
    uint32_t* dc;
    uint32_t* ac;
    bool first = true;
    IFHIP_HD void put(uint32_t code, uint32_t len) { Add::add((first ? dc : ac) + (code >> len), 1u); first = false; }
    IFHIP_HD void put_times(uint32_t code, uint32_t len, uint32_t times) { if (times) Add::add(ac + (code >> len), times); }
};

template <class Out>
IFHIP_HD void prog_raw_bits(Out& out, uint64_t bits, uint32_t n) {      // n <= 63 bits, the first one highest
    if (n > 32u) { out.raw(static_cast<uint32_t>(bits >> 32), n - 32u); out.raw(static_cast<uint32_t>(bits), 32u); }
    else if (n) out.raw(static_cast<uint32_t>(bits), n);
}
// the EOBn symbol of a run that starts at this block (eobrun = 0: none does)
template <class Out>
IFHIP_HD void prog_put_eobrun(Out& out, uint32_t eobrun) {
    if (eobrun) {
        const uint32_t nb = 31u - static_cast<uint32_t>(__builtin_clz(eobrun));
        out.sym(nb << 4, eobrun & ((1u << nb) - 1u), nb);
    }
}

// jcphuff.c encode_mcu_DC_first: the category of (coef >> Al) - predecessor and its bits
template <class Out>
IFHIP_HD uint32_t prog_dc_first(int32_t coef0, int32_t pred_coef, uint32_t al, Out& out) {
    const int32_t diff = (coef0 >> al) - (pred_coef >> al);
    const uint32_t t = static_cast<uint32_t>(diff < 0 ? -diff : diff), t2 = static_cast<uint32_t>(diff < 0 ? diff - 1 : diff);
    uint32_t nb = enc_nbits(t), bad = 0;
    if (nb > 11u) { bad = kProgBad; nb = 11u; }
    out.sym(nb, t2 & ((1u << nb) - 1u), nb);
    return bad | kProgHead;
}

// jcphuff.c encode_mcu_AC_first
template <class Coef, class Out>
IFHIP_HD uint32_t prog_ac_first(const Coef& coef, uint32_t Ss, uint32_t Se, uint32_t al, uint32_t eobrun, Out& out) {
    uint64_t nz, one;
    prog_masks(coef, al, &nz, &one);
    uint64_t m = nz & prog_band(Ss, Se);
    uint32_t flags = m ? kProgHead : 0u, prev = Ss - 1u, widest = 0;
    while (m) {
        const uint32_t k = static_cast<uint32_t>(__builtin_clzll(m));
        m &= ~(0x8000000000000000ull >> k);
        const uint32_t run = k - prev - 1u;
        prev = k;
        for (uint32_t z = run >> 4; z; --z) out.sym(0xF0u, 0u, 0u);
        const int32_t v = coef(static_cast<int>(k));
        const uint32_t a = static_cast<uint32_t>(v < 0 ? -v : v) >> al;
        uint32_t nb = enc_nbits(a);
        widest = nb > widest ? nb : widest;
        nb = nb > 10u ? 10u : nb;
        out.sym(((run & 15u) << 4) + nb, (v < 0 ? ~a : a) & ((1u << nb) - 1u), nb);
    }
    if (widest > 10u) flags |= kProgBad;
    if (prev != Se) { flags |= kProgTail; prog_put_eobrun(out, eobrun); }
    return flags;
}

// jcphuff.c encode_mcu_AC_refine
template <class Coef, class Out>
IFHIP_HD uint32_t prog_ac_refine(const Coef& coef, uint32_t Ss, uint32_t Se, uint32_t al, uint32_t eobrun, Out& out) {
    uint64_t nz, one;
    prog_masks(coef, al, &nz, &one);
    const uint64_t band = prog_band(Ss, Se);
    uint64_t m = nz & band;
    one &= band;
    const uint32_t eob = one ? 63u - static_cast<uint32_t>(__builtin_ctzll(one)) : 0u;     // the last newly nonzero coefficient
    uint32_t flags = 0, r = 0, prev = Ss - 1u, nbr = 0;
    uint64_t br = 0;                                // correction bits since the last symbol
    while (m) {
        const uint32_t k = static_cast<uint32_t>(__builtin_clzll(m));
        m &= ~(0x8000000000000000ull >> k);
        r += k - prev - 1u;
        prev = k;
        while (r > 15u && k <= eob) {               // (a symbol of the block: the pending run ends in front of it)
            out.sym(0xF0u, 0u, 0u);
            r -= 16u;
            prog_raw_bits(out, br, nbr);
            br = 0; nbr = 0;
            flags |= kProgHead;
        }
        const int32_t v = coef(static_cast<int>(k));
        if (!((one >> (63u - k)) & 1u)) {           // already nonzero: one correction bit
            br = (br << 1) | ((static_cast<uint32_t>(v < 0 ? -v : v) >> al) & 1u);
            ++nbr;
            continue;
        }
        out.sym((r << 4) + 1u, v < 0 ? 0u : 1u, 1u);
        prog_raw_bits(out, br, nbr);
        br = 0; nbr = 0; r = 0;
        flags |= kProgHead;
    }
    r += Se - prev;
    if (r > 0u || nbr > 0u) {
        flags |= kProgTail | nbr << 2;
        prog_put_eobrun(out, eobrun);
        prog_raw_bits(out, br, nbr);
    }
    return flags;
}

// ---- end-of-band runs ---------------------------------------------------------------------------------------------------
// A wave walks a scan's blocks 64 at a time.  W (the wave: registers and ballots on the device, arrays in the emulation):
//   load(base, n)        the flags of items base .. base + n - 1, one per lane
//   heads() / tails()    64-bit masks of the loaded lanes
//   prev_tail()          the tail flag of item base - 1 (false at the scan's start)
//   incl_bits(lane)      the inclusive prefix sum over lanes of the tails' correction bit counts
//   crossing(...)        the lanes at which prog_run_crosses holds
//   emit(start, len, by_bits)   a run of `len` blocks whose first block is item `start` (by_bits: 0 cut at 0x7FFF, 1 cut by
//                               the correction bits, 2 ended by a head or the scan's end)
struct ProgRunState { uint32_t len = 0, bits = 0, start = 0; };
IFHIP_HD uint64_t prog_below(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }
// lane's own test: a tail in [q, h) at which the run reaches 0x7FFF blocks or more than 937 buffered bits.  pt / pb: the
// lane's inclusive prefixes of tails and bits; ptq / pbq: the same in front of lane q; len0 / bits0: the run so far.
IFHIP_HD bool prog_run_crosses(uint32_t lane, uint32_t q, uint32_t h, bool tail, uint32_t pt, uint32_t pb, uint32_t ptq, uint32_t pbq,
                               uint32_t len0, uint32_t bits0) {
    return lane >= q && lane < h && tail && (len0 + pt - ptq == kProgEobLimit || bits0 + pb - pbq > kProgCorrLimit);
}
template <class W>
IFHIP_HD void prog_run_step(W& w, ProgRunState& st, uint32_t base, uint32_t q, uint32_t end) {
    const uint64_t H = w.heads(), T = w.tails();
    while (q < end) {
        const uint64_t hm = H & ~prog_below(q) & prog_below(end);
        const uint32_t h = hm ? static_cast<uint32_t>(__builtin_ctzll(hm)) : end;
        if (h > q) {                                // tails without a head between
            const uint32_t ptq = static_cast<uint32_t>(__builtin_popcountll(T & prog_below(q))), pbq = q ? w.incl_bits(q - 1u) : 0u;
            const uint64_t cm = w.crossing(q, h, st.len, st.bits, ptq, pbq);
            const uint32_t x = cm ? static_cast<uint32_t>(__builtin_ctzll(cm)) : h - 1u;
            const uint64_t seg = T & ~prog_below(q) & prog_below(x + 1u);
            if (seg) {
                if (st.len == 0u) st.start = base + static_cast<uint32_t>(__builtin_ctzll(seg));
                st.len += static_cast<uint32_t>(__builtin_popcountll(seg));
                st.bits += w.incl_bits(x) - pbq;
            }
            if (cm) {                               // the cut: greedy, the moment the bound is reached
                w.emit(st.start, st.len, st.len == kProgEobLimit ? 0u : 1u);
                st.len = 0; st.bits = 0;
            }
            q = x + 1u;
            continue;
        }
        // a head at lane q: the pending run is written in front of its first symbol; its own tail starts the next run
        if (st.len) w.emit(st.start, st.len, 2u);
        st.len = 0; st.bits = 0;
        if ((T >> q) & 1u) { st.start = base + q; st.len = 1u; st.bits = w.incl_bits(q) - (q ? w.incl_bits(q - 1u) : 0u); }
        ++q;
    }
}
// The runs that START in items [c0, c1) of a scan of n items: a maximal run (tails with no head between) belongs to the
// chunk of its first block and is walked to its end, beyond c1 if need be -- the cut is not associative, so a run is never
// split among waves; a flat frame is one run, walked by one wave in steps of 64.
template <class W>
IFHIP_HD void prog_run_chunk(W& w, uint32_t c0, uint32_t c1, uint32_t n) {
    ProgRunState st;
    bool skipping = c0 != 0u;                       // until the first run that starts in the chunk
    for (uint32_t base = c0; base < n; base += 64u) {
        const uint32_t nv = n - base < 64u ? n - base : 64u;
        w.load(base, nv);
        const uint64_t H = w.heads(), T = w.tails(), valid = prog_below(nv);
        const uint64_t prev_t = (T << 1) | (w.prev_tail() ? 1ull : 0ull);
        const uint32_t lo = c1 > base ? c1 - base : 0u;
        uint32_t q = 0, end = nv;
        // at or behind c1: a head ends the run, a block behind a block without a tail starts one of the next chunk's
        const uint64_t X = (H | ~prev_t) & valid & ~prog_below(lo);
        if (X) end = static_cast<uint32_t>(__builtin_ctzll(X));
        if (skipping) {
            const uint64_t S = T & (H | ~prev_t) & valid & prog_below(lo);
            if (!S) { if (base + 64u >= c1) return; continue; }
            q = static_cast<uint32_t>(__builtin_ctzll(S));
            skipping = false;
        }
        prog_run_step(w, st, base, q, end);
        if (end < nv) break;
    }
    if (st.len) w.emit(st.start, st.len, 2u);
}

// ---- jpeg_gen_optimal_table ---------------------------------------------------------------------------------------------
// The two minimum searches of a merge step are lane-parallel: the least frequency, ties to the LARGER symbol (jchuff.c
// scans upwards with <=), as one 64-bit key; a lane looks at entries lane, lane + 64, ... of the 257.
IFHIP_HD uint64_t huff_key(uint32_t freq, uint32_t i) { return freq ? (static_cast<uint64_t>(freq) << 9) | (511u - i) : ~0ull; }
IFHIP_HD uint32_t huff_key_index(uint64_t key) { return 511u - static_cast<uint32_t>(key & 511u); }
IFHIP_HD uint64_t huff_lane_key(const uint32_t* freq, uint32_t lane, uint32_t exclude) {
    uint64_t best = ~0ull;
    for (uint32_t i = lane; i < 257u; i += 64u) {
        const uint64_t k = i == exclude ? ~0ull : huff_key(freq[i], i);
        best = k < best ? k : best;
    }
    return best;
}
IFHIP_HD void huff_init(const uint32_t* counts, uint32_t lane, uint32_t* freq, uint32_t* codesize, int32_t* others) {
    for (uint32_t i = lane; i < 257u; i += 64u) { freq[i] = i < 256u ? counts[i] : 1u; codesize[i] = 0u; others[i] = -1; }
}
IFHIP_HD void huff_merge(uint32_t c1, uint32_t c2, uint32_t* freq, uint32_t* codesize, int32_t* others) {
    freq[c1] += freq[c2];
    freq[c2] = 0;
    codesize[c1]++;
    while (others[c1] >= 0) { c1 = static_cast<uint32_t>(others[c1]); codesize[c1]++; }
    others[c1] = static_cast<int32_t>(c2);
    codesize[c2]++;
    while (others[c2] >= 0) { c2 = static_cast<uint32_t>(others[c2]); codesize[c2]++; }
}
// Annex K.2 (adjust_bits): the counts per length, limited to 16, the pseudo-symbol's code point taken from the longest
IFHIP_HD void huff_limit(const uint32_t* codesize, uint32_t* bits /* [33] */) {
    for (int i = 0; i <= 32; ++i) bits[i] = 0;
    for (int i = 0; i <= 256; ++i) if (codesize[i]) bits[codesize[i] > 32u ? 32u : codesize[i]]++;
    int i;
    for (i = 32; i > 16; --i)
        while (bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && bits[j] == 0) --j;
            bits[i] -= 2; bits[i - 1]++; bits[j + 1] += 2; bits[j]--;
        }
    while (i > 0 && bits[i] == 0) --i;
    if (i > 0) bits[i]--;
}
// a symbol's place in the DHT's value list: ordered by code length as merged (before the limit), then by symbol
IFHIP_HD uint32_t huff_rank(const uint32_t* codesize, uint32_t j) {
    uint32_t r = 0;
    const uint32_t mine = codesize[j];
    for (uint32_t i = 0; i < 256u; ++i) {
        const uint32_t c = codesize[i];
        r += (c != 0u && (c < mine || (c == mine && i < j))) ? 1u : 0u;
    }
    return r;
}
// The DHT segment and the encode table (jpeg_make_c_derived_tbl) from the counts per length and the ordered values;
// returns the segment's length.  `codes` must be zero.
IFHIP_HD uint32_t huff_emit(const uint32_t* bits, const uint8_t* vals, uint32_t id, uint8_t* dht, uint32_t* codes) {
    uint32_t nvals = 0;
    for (int l = 1; l <= 16; ++l) nvals += bits[l];
    const uint32_t len = 2u + 1u + 16u + nvals;
    dht[0] = 0xFF; dht[1] = 0xC4; dht[2] = static_cast<uint8_t>(len >> 8); dht[3] = static_cast<uint8_t>(len); dht[4] = static_cast<uint8_t>(id);
    uint32_t code = 0, k = 0;
    for (uint32_t l = 1; l <= 16u; ++l) {
        dht[4u + l] = static_cast<uint8_t>(bits[l]);
        for (uint32_t i = 0; i < bits[l]; ++i, ++k, ++code) { dht[21u + k] = vals[k]; codes[vals[k]] = code | (l << 16); }
        code <<= 1;
    }
    return len + 2u;
}

}  // namespace ifhip
