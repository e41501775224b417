// jpeg_entropy.hip -- baseline (sequential Huffman) JPEG entropy decoding on gfx950.
//
// Replaces the serial jpeg_read_coefficients / decode_mcu loop that MzDec::read_frame drives on the host
// (codecs/mozjpeg_decoder.rs:346-362 -> mozjpeg jdhuff.c) and that caps the JPEG path at ~50 MP/s per core: the scan's
// bit stream is decoded by thousands of lanes at once and lands as the quantised coefficient planes the pixel stage
// (jpeg_kernels.hip) consumes, so a compressed file is the only thing that crosses PCIe.
//
// Host: jpeg_parse.cpp reads the markers (SOF0/SOF1, DHT, DQT, DRI, SOS), un-stuffs the scan and splits it at restart markers
// into *segments* (independent bit streams with a known start state).  The rest of the host half is plain C++ that a host
// compiler builds alone: jpeg_entropy_tables.hpp / .cpp (the entry formats both sides read, the decode tables of a file),
// jpeg_entropy_plan.hpp / .cpp (what is prepared of a file, the layout of a batch's table block) and jpeg_scan_report.cpp (the
// host diagnostic).  This file keeps the kernels, the device side of the two handles, the uploads and the launches.
// Device: the self-synchronising parallel decode (Klein & Wiseman; Weissenberger & Schmidt, ICPP 2018):
//   * the stream is cut into sub-sequences of 1024 bits, one lane each;
//   * round 0 decodes every sub-sequence speculatively from state (block 0 of the MCU, coefficient 0); because Huffman
//     codes re-synchronise, most lanes end in the true state; then, inside the workgroup, every lane whose predecessor's
//     exit state moved decodes again from it, until nothing moves (first lanes of a segment are exact, so the fixpoint is
//     the serial decode); workgroups warm up on the sub-sequences in front of their range, so nothing crosses them;
//   * the count pass walks every sub-sequence from its final entry state: blocks started and DC sums per component (and
//     it checks the fixpoint: only if a sub-sequence was decoded from another state than its predecessor's exit does the
//     host run further rounds);
//   * the write pass scans those counts (every lane's output block and DC predictors), decodes once more and stores
//     coefficients (natural order) straight into the planes.
// Integer / table work, bound by dependent bit-serial decoding per lane and L1/L2 latency, not by HBM (no MFMA).
// Coefficient-exact against oracle/jpeg_oracle.c jo_jpeg_read_coefficients (itself pinned to libjpeg-turbo).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hip_entry.hpp"
#include "jpeg_entropy_plan.hpp"

namespace ifhip {

struct EntropyArgs {
    EntropyGeom g;
    const uint32_t* words;                           // un-stuffed scan data, big-endian words, segments 1024-bit aligned
    const Segment* segs;
    const uint32_t* sub_seg;                         // segment of every sub-sequence
    const uint32_t* wg_order;                        // synchronisation launch: workgroup blockIdx.x works on this block of kOwnSubs sub-sequences
    const FastTabs* ftabs;                           // [image]
    const FastTabs* ptabs;                           // [image] the same tables with pair entries, for the synchronisation rounds
    const FastTabs* ctabs;                           // [image] pair entries in the AC tables only, for the count pass (it reads the DC symbols)
    const SearchTab* stabs;                          // [image][comp][dc, ac]: the serial search, for sub-tables that did not fit
    uint32_t n_sub, n_seg;
    uint32_t uniform_tables;                         // every image carries the same Huffman tables (e.g. the standard ones)
    uint32_t* exit_p[2];                             // exit bit position, double buffered by round parity
    uint32_t* exit_cz[2];                            // exit (block-in-MCU << 8) | zigzag index
    uint32_t* start_p;                               // start state the lane last decoded from
    uint32_t* start_cz;
    int4* cnt;                                       // per sub-sequence {blocks started, DC sum comp 0, 1, 2}
    int4* tail;                                      // per chunk of kChunkSubs sub-sequences: sum of cnt over the part that belongs to the
                                                     // segment of the chunk's last sub-sequence (what a segment carries into the next chunk)
    uint32_t* changed;                               // [16] lanes whose exit state moved in round r, at [r & 15]
    uint32_t* errors;                                // [16] bit 0 invalid code, 2 run past 63, 3 short segment
    uint32_t* unsettled;                             // [17] sub-sequences the count pass found decoded from another state than their predecessor's exit
    int16_t* coef[3];                                // [image][bh][bw][64]
    uint32_t round;
    uint32_t inner_rounds;                           // fixpoint iterations inside a workgroup per launch (kInnerRounds; tests lower it)
};

__constant__ uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                                    15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- per-workgroup staging and the bit reader ---------------------------------------------------------------------
// A workgroup owns kWg consecutive sub-sequences of contiguous stream, copied into LDS with coalesced loads.  The copy
// is COLUMN-MAJOR with pitch 33 (word j of sub-sequence t at t * 33 + j: lanes walking their own sub-sequences at the
// same depth hit 32 different banks); bit positions are relative to the workgroup's first bit.
constexpr uint32_t kMarginSubs = 3;                  // > the longest possible block (64 symbols x 31 bits) + lookahead
constexpr uint32_t kColPitch = kSubWords + 1u;

template <uint32_t kWg, uint32_t kColsT>
__device__ __forceinline__ void stage_stream_columns(const EntropyArgs& a, uint32_t* lds_words, uint32_t first_sub) {
    const uint32_t word0 = first_sub * kSubWords;
    const uint32_t total = (a.n_sub + 2u) * kSubWords;                 // the buffer carries 64 slack words
    constexpr uint32_t kPer = (kColsT * kSubWords + kWg - 1u) / kWg;
    uint32_t v[kPer];
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {                              // all loads in flight before the first LDS store
        const uint32_t w = word0 + threadIdx.x + i * kWg;
        v[i] = w < total ? a.words[w] : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
        const uint32_t r = threadIdx.x + i * kWg;
        if (r < kColsT * kSubWords) lds_words[r + r / kSubWords] = v[i];
    }
}
__device__ __forceinline__ uint32_t stream_word(const uint32_t* lds_words, uint32_t i) { return lds_words[i + i / kSubWords]; }

// The stream behind a bit position, in registers: the two words the 32-bit window straddles, the word after them
// (requested one refill early, so the only LDS read on a symbol's dependent chain is the table entry) and the number
// of unread bits left in the first word.  The window is one v_alignbit_b32; moving on is branch-free -- with 64 lanes
// some lane refills in every iteration anyway, and a branch costs more than the four selects.
struct Reader {
    uint32_t w0, w1, next;
    uint32_t left;                                   // unread bits of w0: 0..31 (0: the window is w1)
    uint32_t at;                                     // word index of `next`
    __device__ __forceinline__ void open(const uint32_t* lds_words, uint32_t p) {
        const uint32_t i1 = (p + 31u) >> 5;
        w0 = stream_word(lds_words, i1 ? i1 - 1u : 0u);
        w1 = stream_word(lds_words, i1);
        at = i1 + 1u;
        next = stream_word(lds_words, at);
        left = (0u - p) & 31u;
    }
    __device__ __forceinline__ uint32_t peek() const { return __builtin_amdgcn_alignbit(w0, w1, left); }
    __device__ __forceinline__ void skip(const uint32_t* lds_words, uint32_t n) {       // n <= 31
        const int32_t rest = static_cast<int32_t>(left) - static_cast<int32_t>(n);
        const bool over = rest < 0;
        w0 = over ? w1 : w0;
        w1 = over ? next : w1;
        at += over ? 1u : 0u;
        left = static_cast<uint32_t>(rest) & 31u;
        next = stream_word(lds_words, at);
    }
};

// ---- synchronisation and count passes: the lean walker ----------------------------------------------------------
// These passes need the decoder STATE only (bit position, block-in-MCU, zigzag index), not the coefficients.  A dense
// pass is bound by instruction issue, a re-decode iteration of the fixpoint by the dependent chain of one symbol; both
// shrink with the instruction count.  Per symbol: the window (1 instruction), the table entry (address + LDS read),
// the reader's refill and the end-of-block bookkeeping as selects -- no divergent branch but the long-code lookup.
// kCount: also count the blocks started and sum the DC differences per component (into the lane's LDS slots dcs[comp *
// kDcPitch]: a dynamic index into three registers costs eight selects).
template <bool kCount, uint32_t kDcPitch, int kPairs, typename Tabs>
__device__ __forceinline__ void walk(const EntropyGeom& g, const uint32_t* lds_words, const Tabs* T, const SearchTab* S, uint32_t end,
                                     uint32_t& p, uint32_t& c, uint32_t& z, int32_t& n, int32_t* dcs) {
    const auto* lut0 = &T->lut[0][0];
    uint32_t comp = (g.kcomp_packed >> (2u * c)) & 3u;
    const auto* tcur = lut0 + comp * (2u * kLutEntries) + (z ? kLutEntries : 0u);
    Reader rd;
    rd.open(lds_words, p);
    while (p < end) {
        const uint32_t bits = rd.peek();
        uint32_t e = tcur[bits >> (32u - kLutBits)];
        if ((e & 255u) == 0u) e = long_entry<kPairs>(T, S, static_cast<uint32_t>(tcur - lut0) / kLutEntries, e, bits);
        if constexpr (kPairs == 1) {                                 // this symbol and the next, if this one ends neither block nor walk
            const bool both = z + ((e >> 8) & 255u) < 64u && p + (e & 255u) < end;
            e = both ? e >> 16 : e;
        }
        if constexpr (kCount) if (z == 0u) {                                     // DC symbol: jdhuff.c HUFF_EXTEND of the sz bits behind the code
            const uint32_t len = (e >> 16) & 255u, sz = (e >> 24) & 15u;
            const uint32_t v = ((bits << len) >> 1) >> (31u - sz);
            const int32_t ext = static_cast<int32_t>(v) - ((static_cast<int32_t>(bits << len) < 0 || sz == 0u) ? 0 : static_cast<int32_t>((1u << sz) - 1u));
            ++n;
            __hip_atomic_fetch_add(dcs + comp * kDcPitch, ext, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // ds_add, nothing returns
        }
        if constexpr (kPairs == 2) {                                 // (the DC entries of these tables are plain: the count pass reads them)
            const bool both = z != 0u && z + ((e >> 8) & 255u) < 64u && p + (e & 255u) < end;
            e = both ? e >> 16 : e;
        }
        const uint32_t skip = e & 255u;
        p += skip;
        rd.skip(lds_words, skip);
        z += (e >> 8) & 255u;
        const bool done = z >= 64u;                                  // block complete: next block of the MCU
        z = done ? 0u : z;
        const uint32_t c1 = c + 1u == g.blocks_per_mcu ? 0u : c + 1u;
        c = done ? c1 : c;
        comp = (g.kcomp_packed >> (2u * c)) & 3u;
        tcur = lut0 + comp * (2u * kLutEntries) + (done ? 0u : kLutEntries);
    }
}

// The same walk by a whole WAVE for one sub-sequence: lane d looks up the symbol that would start d bits behind the
// current position (all 64 offsets at once: one LDS round trip), then the chain "symbol at 0 -> skip -> symbol at skip
// -> ..." is resolved with scalar instructions and readlane -- no memory access on the dependent chain -- until the block
// ends (the tables change), the 64 looked-up offsets are used up or the sub-sequence ends.  About one block per window.
// A lone lane needs ~400 cycles per symbol (a wave issues one instruction per 4 cycles and every symbol waits for its
// table entry); the late iterations of the fixpoint, where a few sub-sequences carry a correction forward one step per
// iteration, are nothing but such lone walks.  p, c, z and end are wave-uniform.
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }

template <typename Tabs>
__device__ __forceinline__ void walk_wave(const EntropyGeom& g, const uint32_t* lds_words, const Tabs* T, const SearchTab* S, uint32_t end_,
                                          uint32_t& p_, uint32_t& c_, uint32_t& z_) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t p = uniform(p_), c = uniform(c_), z = uniform(z_);     // scalar registers: the chain below is scalar code
    const uint32_t end = uniform(end_), bpm = uniform(g.blocks_per_mcu), kc = uniform(g.kcomp_packed);
    while (p < end) {
        const uint32_t slot_ac = ((kc >> (2u * c)) & 3u) * 2u + 1u;
        const uint32_t q = p + lane, w = q >> 5;
        const uint32_t bits = __builtin_amdgcn_alignbit(stream_word(lds_words, w), stream_word(lds_words, w + 1u), (0u - q) & 31u);
        // (alignbit by 0 returns its second word: q & 31 == 0 needs the first)
        const uint32_t win = (q & 31u) ? bits : stream_word(lds_words, w);
        const uint32_t slot = (lane == 0u && z == 0u) ? slot_ac - 1u : slot_ac;       // only the symbol at the current position can be a DC symbol
        uint32_t e = T->lut[slot][win >> (32u - kLutBits)];
        // The chain, in scalar registers: entry of the symbol at `pos`, advance pos and z, until the block ends (z >= 64),
        // the window is used up (pos >= lim) or an entry has no skip (a code longer than the lookup ON the chain, 2 % of
        // the symbols: the long codes of the window are resolved then, once, and the chain goes on).  Hand-written because
        // the loop is the critical path of the late iterations: ten instructions and one taken branch per symbol.
        const uint32_t lim = min(64u, end - p);
        uint32_t pos = 0u, es, tmp;
        for (;;) {
            asm volatile(
                "1:\n\t"
                "v_readlane_b32 %[es], %[e], %[pos]\n\t"
                "s_and_b32 %[tmp], %[es], 0xff\n\t"
                "s_cbranch_scc0 2f\n\t"
                "s_add_u32 %[pos], %[pos], %[tmp]\n\t"
                "s_bfe_u32 %[tmp], %[es], 0x80008\n\t"
                "s_add_u32 %[z], %[z], %[tmp]\n\t"
                "s_cmp_ge_u32 %[z], 64\n\t"
                "s_cbranch_scc1 2f\n\t"
                "s_cmp_lt_u32 %[pos], %[lim]\n\t"
                "s_cbranch_scc1 1b\n\t"
                "2:"
                : [pos] "+s"(pos), [z] "+s"(z), [es] "=&s"(es), [tmp] "=&s"(tmp)
                : [e] "v"(e), [lim] "s"(lim)
                : "scc");
            if ((es & 255u) != 0u) break;
            if ((e & 255u) == 0u) e = long_entry<1>(T, S, slot, e, win);         // (only bits 0-15 of an entry are used here)
        }
        if (z >= 64u) {                                              // block complete: the lanes behind looked up the old tables
            z = 0u;
            c = c + 1u == bpm ? 0u : c + 1u;
        }
        p += pos;
    }
    p_ = p; c_ = c; z_ = z;
}

template <typename F>
__device__ __forceinline__ void with_fast_tables(const EntropyArgs& a, const FastTabs* gtabs, const FastTabs* lds_tabs, uint32_t lds_image,
                                                 uint32_t image, F&& f) {
    const SearchTab* S = a.stabs + static_cast<size_t>(image) * 6u;
    if (image == lds_image || a.uniform_tables) f(reinterpret_cast<const __attribute__((address_space(3))) FastTabs*>(
                                  static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds_tabs))), S);
    else f(gtabs + image, S);
}
template <uint32_t kWg>
__device__ __forceinline__ void stage_fast_tables(const FastTabs* gtabs, FastTabs* lds_tabs, uint32_t image) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(gtabs + image);
    uint32_t* dst = reinterpret_cast<uint32_t*>(lds_tabs);
    for (uint32_t i = threadIdx.x; i < sizeof(FastTabs) / 4u; i += kWg) dst[i] = src[i];
}

// (kSyncLanes, kWarmLanes, kOwnSubs, kInnerRounds, kChunkSubs, kFlagWords: jpeg_entropy_tables.hpp, the host sizes a batch by them)
constexpr uint32_t kSyncCols = kSyncLanes + 1u;                    // a walk stops within 31 bits of its end and looks 3 words ahead
constexpr uint32_t kFastStageDwords = kSyncCols * kColPitch;

// One synchronisation launch.  Inside the workgroup the fixpoint iteration runs in LDS: in every iteration the
// sub-sequences whose entry state (= the predecessor's exit) moved are decoded again, until nothing moves or
// kInnerRounds is reached; the host only iterates for corrections that cross workgroup boundaries.
// After the first two iterations few sub-sequences need another decode, but they are scattered -- a wave with one busy
// lane costs as much as a full one -- so the iteration COMPACTS them: sub-sequence states live in LDS (one packed word:
// relative bit position | block-in-MCU << 21 | zigzag index << 25), the lanes that need a decode enter a work list
// through a ballot / prefix count, and lane k decodes the k-th entry.  An iteration then costs what its dense waves cost.
constexpr uint32_t kWaveWalkMax = 16;                          // at most this many pending sub-sequences: one wave per walk
constexpr uint32_t kNever = 0xffffffffu;                       // no decode yet (no real state packs to this)
static_assert((kSyncLanes + 2u) * kSubBits < (1u << 21), "packed state: 21 bits of relative position");

__device__ __forceinline__ uint32_t pack_state(uint32_t p_rel, uint32_t cz) { return p_rel | ((cz >> 8) << 21) | ((cz & 255u) << 25); }

__global__ void __launch_bounds__(kSyncLanes) entropy_round_kernel(const EntropyArgs a) {
    __shared__ uint32_t lds_words[kFastStageDwords];
    __shared__ FastTabs lds_tabs;
    __shared__ uint2 st[kSyncLanes];                                 // .x exit state, .y the entry state it was decoded from (written as a pair)
    __shared__ uint16_t endinfo[kSyncLanes], work[kSyncLanes];       // end - t * 1024 (| kChase); sub-sequences to decode this iteration
    __shared__ uint32_t wave_cnt[kSyncLanes / 64u];
    // Workgroups are dispatched in blockIdx order and the launch lasts until its slowest one is done.  Their times differ by
    // what the fixpoint needs -- typically 3 iterations on a smooth image and 8 on a noisy one, ~19 us each -- but the LONGEST
    // correction chains of a batch (24 - 50 iterations on BASELINE cfg4's batches) sit in the SMOOTH images: where every block
    // looks like its neighbour a decoder that is bit-synchronous but one block out of phase in the MCU stays out of phase,
    // while noise throws it out and lets it re-synchronise.  One such chain that starts in the last dispatch round sets the
    // launch's length (measured: 1 425 us with a 50-iteration workgroup dispatched at 506 us, where perfect packing is 575).  So
    // the blocks of the images with the SMALLEST scans are dispatched first: their rare long chains run beside everybody else
    // (the same two batches: 848 -> 724 and 1 425 -> 946 us per launch; largest-first made it 1 016 and 1 409;
    // profiles/r6_entropy_dispatch_order.txt).  The true state crosses such a region one sub-sequence per iteration while
    // everything behind the front is decoded again from entries that are still wrong, so these iterations are lane walks of many
    // sub-sequences, not lone wave walks: letting a lone chain's wave follow it link by link (measured, round 6) met 3 of 50.
    const uint32_t own_sub = a.wg_order[blockIdx.x] * kOwnSubs, first_sub = own_sub - kWarmLanes;     // (wraps for block 0: those lanes are off)
    const uint32_t t = threadIdx.x, s = first_sub + t, lane = t & 63u, wave = t >> 6;
    if (a.round == 0u && blockIdx.x == 0u && t < kFlagWords) a.changed[t] = 0u;     // the flags of this decode (later launches set them)
    const uint32_t t0 = a.round == 0u ? 0u : kWarmLanes;             // first lane at work
    const bool on = s < a.n_sub && t >= t0;
    const uint32_t cur = a.round & 1u, prv = cur ^ 1u;
    const uint32_t bit0 = first_sub * kSubBits;
    const Segment sg = a.segs[a.sub_seg[on ? s : own_sub]];
    const bool first = on && s == sg.first_sub;
    // state carried over from the previous launch (none in round 0)
    uint32_t st_ex = 0u, st_used = kNever;
    if (on && a.round > 0u) {
        st_ex = pack_state(a.exit_p[prv][s] - bit0, a.exit_cz[prv][s]);
        st_used = a.start_p[s] == kNever ? kNever : pack_state(a.start_p[s] - bit0, a.start_cz[s]);
    }
    const uint32_t old_ex = st_ex;
    // entry state of lane 0 of the workgroup comes from the previous workgroup's last launch; round 0 starts every
    // sub-sequence speculatively at its own first bit
    uint32_t fixed_entry = pack_state(t * kSubBits, 0u);
    const bool fixed = first || a.round == 0u || t == t0;
    if (on && !first && a.round > 0u && t == t0) fixed_entry = pack_state(a.exit_p[prv][s - 1u] - bit0, a.exit_cz[prv][s - 1u]);
    if (a.round > 0u) {
        const uint32_t entry = (fixed || !on) ? fixed_entry : pack_state(a.exit_p[prv][s - 1u] - bit0, a.exit_cz[prv][s - 1u]);
        if (!__syncthreads_or(on && entry != st_used ? 1 : 0)) {     // nothing moved in front of this workgroup
            if (on) { a.exit_p[cur][s] = a.exit_p[prv][s]; a.exit_cz[cur][s] = a.exit_cz[prv][s]; }
            return;
        }
    }
    const uint32_t wg_image = a.segs[a.sub_seg[own_sub]].image;
    stage_stream_columns<kSyncLanes, kSyncCols>(a, lds_words, first_sub);
    stage_fast_tables<kSyncLanes>(a.ptabs, &lds_tabs, wg_image);
    st[t] = make_uint2(st_ex, st_used);
    constexpr uint32_t kChase = 0x8000u;                             // the entry is the predecessor's exit (not a segment's first sub-sequence)
    endinfo[t] = static_cast<uint16_t>(on ? (min((s + 1u) * kSubBits, sg.bit_end) - s * kSubBits) | (first ? 0u : kChase) : 0u);
    __syncthreads();
    bool pending = false;
    for (uint32_t it = 0; it < a.inner_rounds; ++it) {
        // speculative first decode of round 0: from the sub-sequence's own first bit; afterwards from the predecessor's exit
        const uint32_t entry = (fixed && !(a.round == 0u && it > 0u && !first && t > 0u)) ? fixed_entry : st[t ? t - 1u : 0u].x;
        const bool need = on && entry != st[t].y;
        const uint64_t vote = __ballot(need);
        if (lane == 0u) wave_cnt[wave] = static_cast<uint32_t>(__popcll(vote));
        __syncthreads();
        uint32_t base = 0u, total = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kSyncLanes / 64u; ++w) { const uint32_t n = wave_cnt[w]; base += w < wave ? n : 0u; total += n; }
        pending = total != 0u;
        if (!pending) break;
        if (need) {
            st[t].y = entry;
            work[base + static_cast<uint32_t>(__popcll(vote & ((1ull << lane) - 1ull)))] = static_cast<uint16_t>(t);
        }
        __syncthreads();
        if (total <= kWaveWalkMax) {                                 // few sub-sequences: one wave each, see walk_wave
            // (Letting the wave FOLLOW a correction into the next sub-sequence instead of leaving it to the next iteration
            // was measured: 459 -> 576 us per launch -- a chain followed from an exit that is itself corrected later is
            // walked twice, and the other work of the wave waits.)
            for (uint32_t k = wave; k < total; k += kSyncLanes / 64u) {
                const uint32_t j = uniform(work[k]);
                const uint32_t e0 = uniform(st[j].y);
                uint32_t p = e0 & 0x1fffffu, c = (e0 >> 21) & 15u, z = e0 >> 25;
                const uint32_t end = j * kSubBits + (endinfo[j] & (kChase - 1u));
                const uint32_t image = a.uniform_tables ? wg_image : a.segs[a.sub_seg[first_sub + j]].image;
                with_fast_tables(a, a.ptabs, &lds_tabs, wg_image, image, [&](auto tabs, const SearchTab* S) { walk_wave(a.g, lds_words, tabs, S, end, p, c, z); });
                if (lane == 0u) st[j].x = p | (c << 21) | (z << 25);
            }
        } else if (t < total) {
            const uint32_t j = work[t];
            const uint32_t e0 = st[j].y;
            uint32_t p = e0 & 0x1fffffu, c = (e0 >> 21) & 15u, z = e0 >> 25;
            const uint32_t end = j * kSubBits + (endinfo[j] & (kChase - 1u));
            int32_t n = 0;
            const uint32_t image = a.uniform_tables ? wg_image : a.segs[a.sub_seg[first_sub + j]].image;
            with_fast_tables(a, a.ptabs, &lds_tabs, wg_image, image, [&](auto tabs, const SearchTab* S) { walk<false, 0u, 1>(a.g, lds_words, tabs, S, end, p, c, z, n, nullptr); });
            st[j].x = p | (c << 21) | (z << 25);
        }
        __syncthreads();
    }
    if (!on || t < kWarmLanes) return;
    const uint32_t fin = st[t].x, fu = st[t].y;
    a.exit_p[cur][s] = (fin & 0x1fffffu) + bit0;
    a.exit_cz[cur][s] = (((fin >> 21) & 15u) << 8) | (fin >> 25);
    a.start_p[s] = fu == kNever ? kNever : (fu & 0x1fffffu) + bit0;
    a.start_cz[s] = (((fu >> 21) & 15u) << 8) | (fu >> 25);
    // another launch is needed if this lane's exit moved (its successor may sit in the next workgroup) or the inner
    // iteration was cut short
    if (a.round > 0u && (fin != old_ex || pending)) atomicAdd(a.changed + (a.round & 15u), 1u);
}

// Count pass, once the exit states are final: every lane walks its sub-sequence from its true entry state and records
// {blocks started, DC difference sum per component}; the write pass turns them into every lane's first block and DC
// predictors (an exclusive scan over the sub-sequences of a segment).  To spare that scan a launch of its own, the
// count pass also leaves, per chunk of kChunkSubs sub-sequences, what a segment carries out of the chunk (`tail`): a
// write workgroup adds the tails of the chunks between its segment's start and itself (a 4K file: at most 26) and
// scans its own 512 counts.  The pass also CHECKS the fixpoint: a sub-sequence that was last decoded from another state
// than its predecessor's exit (a correction that crossed a workgroup boundary of round 0, or an iteration limit) is
// counted in `unsettled`, and the host runs further rounds before it trusts count and write pass.
__device__ __forceinline__ int4 add4(int4 a, int4 b) { return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ int4 sub4(int4 a, int4 b) { return make_int4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ int4 shfl_up4(int4 v, uint32_t d) {
    return make_int4(__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64), __shfl_up(v.z, d, 64), __shfl_up(v.w, d, 64));
}
__device__ __forceinline__ int4 shfl_down4(int4 v, uint32_t d) {
    return make_int4(__shfl_down(v.x, d, 64), __shfl_down(v.y, d, 64), __shfl_down(v.z, d, 64), __shfl_down(v.w, d, 64));
}
__device__ __forceinline__ int4 wave_sum4(int4 v) {                 // lane 0 gets the sum over the wave
#pragma unroll
    for (uint32_t d = 32u; d > 0u; d >>= 1) v = add4(v, shfl_down4(v, d));
    return v;
}
static_assert(kSyncLanes % kChunkSubs == 0u, "a count workgroup covers whole chunks");

__global__ void __launch_bounds__(kSyncLanes) entropy_count_kernel(const EntropyArgs a) {
    __shared__ uint32_t lds_words[kFastStageDwords];
    __shared__ FastTabs lds_tabs;
    __shared__ int32_t lds_dc[3u * kSyncLanes];
    __shared__ int32_t lds_tail[kSyncLanes / kChunkSubs][4];
    const uint32_t first_sub = blockIdx.x * kSyncLanes;
    const uint32_t s = first_sub + threadIdx.x;
    const uint32_t wg_image = a.segs[a.sub_seg[first_sub]].image;
    stage_stream_columns<kSyncLanes, kSyncCols>(a, lds_words, first_sub);
    constexpr int kCountPairs = 2;
    const FastTabs* gtabs = kCountPairs ? a.ctabs : a.ftabs;
    stage_fast_tables<kSyncLanes>(gtabs, &lds_tabs, wg_image);
    int32_t* dcs = lds_dc + threadIdx.x;                     // this lane's three sums, kSyncLanes apart (one bank per lane)
    dcs[0] = 0; dcs[kSyncLanes] = 0; dcs[2u * kSyncLanes] = 0;
    if (threadIdx.x < (kSyncLanes / kChunkSubs) * 4u) (&lds_tail[0][0])[threadIdx.x] = 0;
    __syncthreads();
    const bool on = s < a.n_sub;
    int4 mine = make_int4(0, 0, 0, 0);
    uint32_t my_seg = 0xffffffffu;
    if (on) {
        my_seg = a.sub_seg[s];
        const Segment sg = a.segs[my_seg];
        const uint32_t fin = a.round & 1u;
        const uint32_t bit0 = first_sub * kSubBits;
        uint32_t p = s * kSubBits - bit0, c = 0, z = 0;
        if (s != sg.first_sub) {
            const uint32_t ep = a.exit_p[fin][s - 1u], ecz = a.exit_cz[fin][s - 1u];
            if (a.start_p[s] != ep || a.start_cz[s] != ecz) atomicAdd(a.unsettled, 1u);
            p = ep - bit0; c = ecz >> 8; z = ecz & 255u;
        }
        const uint32_t end = min((s + 1u) * kSubBits, sg.bit_end) - bit0;
        int32_t n = 0;
        with_fast_tables(a, gtabs, &lds_tabs, wg_image, sg.image, [&](auto tabs, const SearchTab* S) { walk<true, kSyncLanes, kCountPairs>(a.g, lds_words, tabs, S, end, p, c, z, n, dcs); });
        mine = make_int4(n, dcs[0], dcs[kSyncLanes], dcs[2u * kSyncLanes]);
        a.cnt[s] = mine;
    }
    // what the segment of each chunk's last sub-sequence carries out of the chunk
    const uint32_t half = threadIdx.x / kChunkSubs;
    const uint32_t chunk_first = first_sub + half * kChunkSubs;
    const bool chunk_on = chunk_first < a.n_sub;
    const uint32_t last_seg = chunk_on ? a.sub_seg[min(chunk_first + kChunkSubs, a.n_sub) - 1u] : 0xfffffffeu;
    const int4 part = wave_sum4(my_seg == last_seg ? mine : make_int4(0, 0, 0, 0));
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&lds_tail[half][0], part.x); atomicAdd(&lds_tail[half][1], part.y);
        atomicAdd(&lds_tail[half][2], part.z); atomicAdd(&lds_tail[half][3], part.w);
    }
    __syncthreads();
    if (threadIdx.x < kSyncLanes / kChunkSubs && first_sub + threadIdx.x * kChunkSubs < a.n_sub)
        a.tail[blockIdx.x * (kSyncLanes / kChunkSubs) + threadIdx.x] =
            make_int4(lds_tail[threadIdx.x][0], lds_tail[threadIdx.x][1], lds_tail[threadIdx.x][2], lds_tail[threadIdx.x][3]);
}

// Write pass.  A block belongs to the lane in whose sub-sequence it STARTS: that lane decodes it to the end (running
// past its sub-sequence if need be), assembles the 64 coefficients in a private LDS row (pitch 36 dwords: 16-byte
// aligned, eight consecutive lanes cover all banks) and stores the whole block with eight 16-byte stores -- every block
// is written exactly once, zeros included, so the planes need no clearing and no two lanes ever touch the same block.
// A lane that starts inside a block skips to its end without storing.  Same reader and table entries as the walker;
// workgroups of 512 sub-sequences (stream 66 KiB + rows 72 KiB + tables: one workgroup per CU).
// Storing a block is ~40 instructions that every lane of the wave pays for whenever ONE lane needs them, and with 64
// lanes a block ends somewhere in almost every symbol step; waiting for all lanes to finish their block (the loop
// structure a compiler makes of "decode a block, store it") leaves most lanes idle, blocks differ that much in length.
// So a lane that completed its block WAITS until kFlushLanes lanes of its wave wait (or nobody decodes any more) and
// they store together: the store path runs every third or fourth symbol step and a lane idles ~2 steps per block.
constexpr uint32_t kWriteLanes = kChunkSubs;
constexpr uint32_t kWriteCols = kWriteLanes + kMarginSubs;
constexpr uint32_t kBlkPitch = 36;                   // dwords per lane row (32 + 4: int16 slots 64..71 are padding)

constexpr uint32_t kFlushLanes = 16;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct BlockPlace { uint32_t hv, bw, bh, comp; };    // block k of an MCU: hs | vs << 8 | dx << 16 | dy << 24, plane dimensions in blocks

__global__ void __launch_bounds__(kWriteLanes) entropy_write_kernel(const EntropyArgs a) {
    __shared__ uint32_t lds_words[kWriteCols * kColPitch];
    __shared__ FastTabs lds_tabs;
    __shared__ __attribute__((aligned(16))) uint32_t lds_blk[kWriteLanes * kBlkPitch];
    __shared__ BlockPlace lds_place[kMaxBlocksInMcu];
    __shared__ int16_t* lds_plane[kMaxBlocksInMcu];  // coefficient plane of block k's component
    __shared__ uint8_t lds_zz[64];                   // zigzag -> natural order (a divergent index into __constant__ memory is a
    if (threadIdx.x < 64u) lds_zz[threadIdx.x] = kZigzag[threadIdx.x];      // vector-memory load per coefficient)
    if (threadIdx.x < a.g.blocks_per_mcu) {
        const uint32_t k = threadIdx.x, cm = a.g.kcomp[k];
        lds_place[k] = BlockPlace{a.g.hs[cm] | (a.g.vs[cm] << 8) | (static_cast<uint32_t>(a.g.kdx[k]) << 16) | (static_cast<uint32_t>(a.g.kdy[k]) << 24),
                                  a.g.bw[cm], a.g.bh[cm], cm};
        lds_plane[k] = a.coef[cm];
    }
    const uint32_t first_sub = blockIdx.x * kWriteLanes;
    const uint32_t s = first_sub + threadIdx.x;
    // This lane's first block and DC predictors: the exclusive scan of the counts over the sub-sequences of its segment
    // = (what the segment carried through the chunks in front of this workgroup) + (the scan inside the workgroup).
    int4 pre;
    {
        __shared__ int4 wave_tot[kWriteLanes / 64u], lead;
        int4* excl_at = reinterpret_cast<int4*>(lds_blk);            // (the rows are not in use yet)
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const bool on = s < a.n_sub;
        const Segment sg0 = a.segs[a.sub_seg[first_sub]], sgm = a.segs[a.sub_seg[on ? s : first_sub]];
        const int4 mine = on ? a.cnt[s] : make_int4(0, 0, 0, 0);
        int4 inc = mine;                                             // inclusive scan inside the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const int4 o = shfl_up4(inc, d);
            if (lane >= d) inc = add4(inc, o);
        }
        if (lane == 63u) wave_tot[wave] = inc;
        if (wave == 0u) {                                            // the leading segment's counts in front of this chunk
            int4 v = make_int4(0, 0, 0, 0);
            if (sg0.first_sub < first_sub)
                for (uint32_t i = sg0.first_sub / kChunkSubs + lane; i < blockIdx.x; i += 64u) v = add4(v, a.tail[i]);
            v = wave_sum4(v);
            if (lane == 0u) lead = v;
        }
        __syncthreads();
        int4 excl = sub4(inc, mine);
        for (uint32_t w = 0; w < wave; ++w) excl = add4(excl, wave_tot[w]);
        excl_at[threadIdx.x] = excl;
        __syncthreads();
        const bool from_before = sgm.first_sub < first_sub;          // the lane's segment began in front of this workgroup
        pre = sub4(excl, excl_at[from_before ? 0u : sgm.first_sub - first_sub]);
        if (from_before) pre = add4(pre, lead);
        __syncthreads();                                             // every lane has read: the rows may be cleared
    }
    int16_t* row = reinterpret_cast<int16_t*>(lds_blk + threadIdx.x * kBlkPitch);
    u32x4* row4 = reinterpret_cast<u32x4*>(lds_blk + threadIdx.x * kBlkPitch);
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) row4[i] = u32x4{0u, 0u, 0u, 0u};               // a row is cleared again when it is stored
    const uint32_t wg_image = a.segs[a.sub_seg[first_sub]].image;
    stage_stream_columns<kWriteLanes, kWriteCols>(a, lds_words, first_sub);
    stage_fast_tables<kWriteLanes>(a.ftabs, &lds_tabs, wg_image);
    __syncthreads();
    if (s >= a.n_sub) return;
    const Segment sg = a.segs[a.sub_seg[s]];
    const uint32_t fin = a.round & 1u;                       // parity of the last round run
    const uint32_t bit0 = first_sub * kSubBits;
    uint32_t p = s * kSubBits - bit0, c = 0u, z = 0u;
    if (s != sg.first_sub) { p = a.exit_p[fin][s - 1u] - bit0; const uint32_t cz = a.exit_cz[fin][s - 1u]; c = cz >> 8; z = cz & 255u; }
    const uint32_t end = min((s + 1u) * kSubBits, sg.bit_end) - bit0;
    uint32_t err = 0;
    int32_t dc0 = pre.y, dc1 = pre.z, dc2 = pre.w;
    uint32_t block = static_cast<uint32_t>(pre.x);           // the next block this lane starts
    const uint32_t B = a.g.blocks_per_mcu;
    uint32_t my, mx;                                         // MCU of that block (the block-in-MCU is the decoder's c)
    { const uint32_t m = sg.first_mcu + block / B; my = m / a.g.mcus_w; mx = m - my * a.g.mcus_w; }
    with_fast_tables(a, a.ftabs, &lds_tabs, wg_image, sg.image, [&](auto T, const SearchTab* S) {
        const auto* lut0 = &T->lut[0][0];
        uint32_t comp = (a.g.kcomp_packed >> (2u * c)) & 3u;
        const auto* tcur = lut0 + comp * (2u * kLutEntries) + (z ? kLutEntries : 0u);
        Reader rd;
        rd.open(lds_words, p);
        // one symbol: entry and the 32 bits it was decoded from; the reader moves on, z / tables are the caller's
        auto symbol = [&](uint32_t& bits) {
            bits = rd.peek();
            uint32_t e = tcur[bits >> (32u - kLutBits)];
            if ((e & 255u) == 0u) e = long_entry(T, S, static_cast<uint32_t>(tcur - lut0) / kLutEntries, e, bits);
            const uint32_t skip = e & 255u;
            p += skip;
            rd.skip(lds_words, skip);
            return e;
        };
        auto advance = [&](uint32_t e) {                     // -> true when the block is complete
            z += (e >> 8) & 255u;
            const bool done = z >= 64u;
            z = done ? 0u : z;
            const uint32_t c1 = c + 1u == B ? 0u : c + 1u;
            c = done ? c1 : c;
            comp = (a.g.kcomp_packed >> (2u * c)) & 3u;
            tcur = lut0 + comp * (2u * kLutEntries) + (done ? 0u : kLutEntries);
            return done;
        };
        uint32_t bits;
        while (z != 0u) advance(symbol(bits));               // tail of the predecessor's block
        bool run = p < end && block < sg.n_blocks;           // a block to decode (pad bits may follow the last block)
        bool waiting = false;                                // block complete, not stored yet
        uint32_t k = c;                                      // block-in-MCU of the block being decoded
        // The DC predictors are touched when a block is stored, not per symbol; a coefficient goes into the row one symbol late: its natural-order index is an LDS lookup, and the wave would
        // sit out that round trip; this way it overlaps the next symbol's table read.
        constexpr uint32_t kNoStore = 64u;                   // a slot in the row's padding: "nothing to store" without a branch
        // (the looked-up index is not even LOOKED AT in the step that requests it -- a select on it would wait for the read --
        // but at the next step's row store: `pend_raw` is that read's destination, `pend_ok` whether it counts)
        uint32_t pend_raw = kNoStore;
        bool pend_ok = false;
        int32_t pend_val = 0;
        for (;;) {
            if (run && !waiting) {
                const bool is_dc = z == 0u;
                bits = rd.peek();
                uint32_t e = tcur[bits >> (32u - kLutBits)];
                row[pend_ok ? pend_raw : kNoStore] = static_cast<int16_t>(pend_val);
                if ((e & 255u) == 0u) e = long_entry(T, S, static_cast<uint32_t>(tcur - lut0) / kLutEntries, e, bits);
                p += e & 255u;
                rd.skip(lds_words, e & 255u);
                const uint32_t len = (e >> 16) & 255u, sz = (e >> 24) & 15u;
                const uint32_t v = ((bits << len) >> 1) >> (31u - sz);           // sz bits behind the code (sz = 0 -> 0)
                const int32_t neg = static_cast<int32_t>((1u << sz) - 1u);
                pend_val = static_cast<int32_t>(v) - ((static_cast<int32_t>(bits << len) < 0 || sz == 0u) ? 0 : neg);   // jdhuff.c HUFF_EXTEND
                const uint32_t pos = z + ((e >> 8) & 255u) - 1u;                // zigzag index of an AC coefficient (DC: 0)
                const bool over = sz != 0u && pos > 63u;                         // a coefficient behind the block's end
                err |= ((e >> 21) & 1u) | (over ? 4u : 0u);                      // (length field 32: no such code)
                pend_raw = lds_zz[pos & 63u];
                pend_ok = is_dc || (sz != 0u && !over);                          // a DC entry holds the DIFFERENCE until the block is stored
                waiting = advance(e);
            }
            const uint32_t n_wait = static_cast<uint32_t>(__popcll(__ballot(waiting)));
            const bool decoding = __ballot(run && !waiting) != 0ull;
            if (n_wait < kFlushLanes && decoding) continue;
            if (n_wait == 0u) break;                         // nobody decodes, nothing to store
            if (waiting) {
                row[pend_ok ? pend_raw : kNoStore] = static_cast<int16_t>(pend_val);
                pend_ok = false;
                // every LDS read of the store (the row, where the block goes) is requested before the first is used
                const BlockPlace pl = lds_place[k];
                int16_t* plane = lds_plane[k];
                u32x4 r[8];
#pragma unroll
                for (uint32_t i = 0; i < 8u; ++i) r[i] = row4[i];
                {                                            // DC: difference -> value (jdhuff.c last_dc_val)
                    const int32_t diff = static_cast<int16_t>(r[0].x & 0xffffu);
                    dc0 += pl.comp == 0u ? diff : 0; dc1 += pl.comp == 1u ? diff : 0; dc2 += pl.comp == 2u ? diff : 0;
                    const int32_t dcv = pl.comp == 0u ? dc0 : (pl.comp == 1u ? dc1 : dc2);
                    r[0].x = (r[0].x & 0xffff0000u) | (static_cast<uint32_t>(dcv) & 0xffffu);
                }
                const uint32_t bx = mx * (pl.hv & 255u) + ((pl.hv >> 16) & 255u), by = my * ((pl.hv >> 8) & 255u) + (pl.hv >> 24);
                auto* dst = reinterpret_cast<__attribute__((address_space(1))) u32x4*>(reinterpret_cast<uintptr_t>(       // (global, not flat, stores)
                    plane + (static_cast<size_t>(sg.image * pl.bh + by) * pl.bw + bx) * 64u));
                // The store is bounded by POSITION as well as by the segment's block count: this launch is enqueued behind the count
                // pass before the host has seen whether the fixpoint settled, and on exit states that are not final a lane's first
                // block and its block-in-MCU phase need not agree -- its MCU row can run past the frame (found by
                // tools/scan_entropy_shapes.py: a fault behind the last image's plane; the decode is repeated after the next
                // rounds, so the result was right, the transient stores were not).
                if (my < a.g.mcus_h) {
#pragma unroll
                    for (uint32_t i = 0; i < 8u; ++i) dst[i] = r[i];
                }
#pragma unroll
                for (uint32_t i = 0; i < 8u; ++i) row4[i] = u32x4{0u, 0u, 0u, 0u};
                ++block;
                if (c == 0u) { ++mx; if (mx == a.g.mcus_w) { mx = 0u; ++my; } }      // the MCU is complete
                k = c;
                waiting = false;
                run = p < end && block < sg.n_blocks;
            }
        }
    });
    const bool last = s + 1u == sg.first_sub + sg.n_sub;
    if (last && block < sg.n_blocks) err |= 8u;              // the segment ran out of data
    if (err) atomicOr(a.errors, err);
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_jpeg_entropy {
    int device = -1;
    uint32_t n_images = 0;
    ParsedJpeg first;                                // geometry shared by the batch
    std::vector<uint16_t> qt;                        // [n][3][64]
    EntropyArgs a;
    std::vector<void*> owned;
    uint32_t* h_flags = nullptr;                     // pinned copy of changed[16] + errors
    uint8_t* h_tables = nullptr;                     // pinned staging of the batch's tables (create_prepared_impl)
    ~ifhip_jpeg_entropy() {
        for (void* p : owned) if (p) (void)DEV_FREE(p);
        if (h_flags) (void)cached_host_free(h_flags);
        if (h_tables) (void)cached_host_free(h_tables);
    }
};

template <typename T>
static int dev_alloc(ifhip_jpeg_entropy* e, T** out, size_t count, const T* init = nullptr) {
    *out = nullptr;
    HIP_TRY(DEV_MALLOC(out, std::max<size_t>(count, 1) * sizeof(T)));
    e->owned.push_back(*out);
    if (init && count) HIP_TRY(static_cast<hipError_t>(copy_to_device(*out, init, count * sizeof(T))));
    return IFHIP_OK;
}

// One file, prepared on the host by whoever owns it: parsed, its scan un-stuffed, cut at the restart markers and packed as
// big-endian words (every segment padded to 1 024 bits) in PINNED memory, its decode tables derived.  A batch is then
// assembled from n of these with no further pass over the data: n asynchronous uploads.  (A service that runs one job per
// thread prepares each job's file on that job's thread -- imageflow_abi/src/lib.rs:20-27 -- and hands the handles of
// whatever is waiting to ONE device call.)  The host part (PreparedHost, jpeg_entropy_plan.hpp) is what a batch is planned from.
struct ifhip_jpeg_prepared : PreparedHost {
    uint32_t* words = nullptr;                       // pinned (devmem cache)
    size_t n_words = 0;
    // ifhip_jpeg_prepared_upload: the words on the device already, queued on the owner's stream; `uploaded` marks the copy's end
    // (the event stays with a recycled handle, the block does not)
    uint32_t* d_words = nullptr;
    hipEvent_t uploaded = nullptr;
    int d_device = -1, event_device = -1;
    void drop_device_copy() {                        // nothing may still write the block when it goes back to the cache
        if (!d_words) return;
        if (uploaded && hipEventQuery(uploaded) != hipSuccess) { (void)hipGetLastError(); (void)hipEventSynchronize(uploaded); }
        (void)hipGetLastError();
        (void)DEV_FREE(d_words);
        d_words = nullptr; d_device = -1;
    }
    ~ifhip_jpeg_prepared() {
        if (words) (void)cached_host_free(words);
        drop_device_copy();
        if (uploaded) (void)hipEventDestroy(uploaded);
    }
};

// Prepared handles are recycled: 50 KB of tables each, one per job through the libimageflow ABI.
namespace {
struct PreparedPool { std::mutex mu; std::vector<ifhip_jpeg_prepared*> spare; };
PreparedPool& prepared_pool() { static PreparedPool* p = new PreparedPool; return *p; }   // (never destroyed: handles may outlive static teardown)
ifhip_jpeg_prepared* take_prepared() {
    {
        PreparedPool& pool = prepared_pool();
        std::lock_guard<std::mutex> lk(pool.mu);
        if (!pool.spare.empty()) { ifhip_jpeg_prepared* p = pool.spare.back(); pool.spare.pop_back(); return p; }
    }
    return new ifhip_jpeg_prepared;
}
void give_prepared(ifhip_jpeg_prepared* p) {
    if (!p) return;
    p->drop_device_copy();                                               // (before the pinned source goes: the copy reads it)
    if (p->words) { (void)cached_host_free(p->words); p->words = nullptr; }
    p->n_words = 0;
    p->seg.clear();
    PreparedPool& pool = prepared_pool();
    {
        std::lock_guard<std::mutex> lk(pool.mu);
        if (pool.spare.size() < 64) { pool.spare.push_back(p); return; }
    }
    delete p;
}
struct GivePrepared { void operator()(ifhip_jpeg_prepared* p) const { give_prepared(p); } };
}  // namespace

static int prepare_impl(ifhip_jpeg_prepared** out, const uint8_t* file, size_t len, uint32_t index_for_messages) {
    std::unique_ptr<ifhip_jpeg_prepared, GivePrepared> R(take_prepared());
    if (int rc = prepare_tables(R.get(), file, len, test_hook_u32("ent_test_pool", kPoolEntries, kPoolEntries))) return rc;
    void* pinned = nullptr;
    size_t pinned_bytes = 4096;                                          // powers of two: few size classes in the pinned cache, whatever the files
    const size_t bound = packed_scan_bound(len, R->P);
    while (pinned_bytes < bound) pinned_bytes *= 2;
    if (cached_host_malloc(&pinned, pinned_bytes) != 0)
        return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: %zu bytes of pinned staging", pinned_bytes);
    R->words = static_cast<uint32_t*>(pinned);                           // (R owns it from here: every return below releases it)
    if (int rc = prepare_scan(R.get(), file, len, R->words, pinned_bytes, index_for_messages, &R->n_words)) return rc;
    *out = R.release();
    return IFHIP_OK;
}

static int create_prepared_impl(ifhip_jpeg_entropy** out, ifhip_jpeg_prepared* const* prep, uint32_t n_images) {
    std::unique_ptr<ifhip_jpeg_entropy> e(new ifhip_jpeg_entropy);
    if (int arc = require_gfx950(&e->device)) return arc;
    e->n_images = n_images;
    e->qt.assign(static_cast<size_t>(n_images) * 192u, 0);
    // The batch's tables are laid out (plan_batch / fill_batch_tables, jpeg_entropy_plan.cpp) in ONE pinned staging block and go
    // to ONE device block in one copy (they were six allocations and six uploads, each with its own wait for the stream: most of
    // the 1.9 ms a 16-file batch spent here, profiles/r5_abi_jobs_cliff_7_decode_batches.txt).
    const std::vector<const PreparedHost*> host(prep, prep + n_images);
    BatchPlan plan;
    if (int prc = plan_batch(host.data(), n_images, &plan)) return prc;
    const size_t table_bytes = plan.table_bytes, n_words = plan.n_words;
    size_t stage_bytes = 4096;                                           // powers of two: few size classes in the pinned cache
    while (stage_bytes < table_bytes) stage_bytes *= 2;
    if (cached_host_malloc(reinterpret_cast<void**>(&e->h_tables), stage_bytes) != 0)
        return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: %zu bytes of pinned staging", stage_bytes);
    uint8_t* const stage = e->h_tables;
    fill_batch_tables(host.data(), n_images, plan, stage);
    e->first = prep[0]->P;
    for (uint32_t img = 0; img < n_images; ++img) std::memcpy(&e->qt[static_cast<size_t>(img) * 192u], prep[img]->qt, sizeof prep[img]->qt);
    EntropyArgs& a = e->a;
    std::memset(&a, 0, sizeof a);
    a.g = plan.g;
    a.inner_rounds = std::max<uint32_t>(1u, test_hook_u32("ent_test_inner", kInnerRounds, kInnerRounds));
    a.n_sub = plan.total_subs;
    a.n_seg = static_cast<uint32_t>(plan.n_segs);
    a.uniform_tables = plan.uniform_tables;
    int rc;
    uint32_t* d_words = nullptr;
    if ((rc = dev_alloc<uint32_t>(e.get(), &d_words, n_words))) return rc;
    // From here on copies into `d_words` FROM the callers' pinned buffers may be queued on the thread's stream.  On any failure
    // below `e` is destroyed and its blocks go back to the cache -- inside an ABI job without a device-wide wait (QuiescedScope)
    // -- and the callers free their pinned sources: neither may happen with a copy still in flight, or the next owner of
    // either block is written over.  Every exit path of this function therefore waits for the stream first.
    struct StreamDrain {
        hipStream_t st;
        ~StreamDrain() { (void)static_cast<hipError_t>(ifhip::wait_stream(st)); }
    } drain{static_cast<hipStream_t>(thread_stream())};
    {   // every file's words straight from its pinned buffer to its place: n asynchronous copies, one wait (below, with the tables')
        hipStream_t st = drain.st;
        for (uint32_t img = 0; img < n_images; ++img) {
            const ifhip_jpeg_prepared& R = *prep[img];
            if (!R.n_words) continue;
            uint32_t* const dst = d_words + static_cast<size_t>(plan.first_sub_of[img]) * kSubWords;
            if (R.d_words && R.d_device == e->device) {              // its owner queued the upload already (ifhip_jpeg_prepared_upload): behind that copy, device to device
                HIP_TRY(hipStreamWaitEvent(st, R.uploaded, 0));
                HIP_TRY(hipMemcpyAsync(dst, R.d_words, R.n_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
            } else {
                HIP_TRY(hipMemcpyAsync(dst, R.words, R.n_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            }
        }
        HIP_TRY(hipMemsetAsync(d_words + (n_words - 64u), 0, 64u * sizeof(uint32_t), st));
    }
    uint8_t* d_tables = nullptr;
    if ((rc = dev_alloc<uint8_t>(e.get(), &d_tables, table_bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(d_tables, stage, table_bytes, hipMemcpyHostToDevice, drain.st));      // (the wait: StreamDrain, on every way out)
    a.words = d_words;
    a.segs = reinterpret_cast<const Segment*>(d_tables + plan.o_segs); a.sub_seg = reinterpret_cast<const uint32_t*>(d_tables + plan.o_sub);
    a.ftabs = reinterpret_cast<const FastTabs*>(d_tables + plan.o_ftabs); a.ptabs = reinterpret_cast<const FastTabs*>(d_tables + plan.o_ptabs);
    a.ctabs = reinterpret_cast<const FastTabs*>(d_tables + plan.o_ctabs); a.stabs = reinterpret_cast<const SearchTab*>(d_tables + plan.o_stabs);
    a.wg_order = reinterpret_cast<const uint32_t*>(d_tables + plan.o_order);
    for (int b = 0; b < 2; ++b) {
        if ((rc = dev_alloc<uint32_t>(e.get(), &a.exit_p[b], a.n_sub))) return rc;
        if ((rc = dev_alloc<uint32_t>(e.get(), &a.exit_cz[b], a.n_sub))) return rc;
    }
    if ((rc = dev_alloc<uint32_t>(e.get(), &a.start_p, a.n_sub))) return rc;
    if ((rc = dev_alloc<uint32_t>(e.get(), &a.start_cz, a.n_sub))) return rc;
    if ((rc = dev_alloc<int4>(e.get(), &a.cnt, a.n_sub))) return rc;
    if ((rc = dev_alloc<int4>(e.get(), &a.tail, (a.n_sub + kChunkSubs - 1u) / kChunkSubs))) return rc;
    if ((rc = dev_alloc<uint32_t>(e.get(), &a.changed, kFlagWords))) return rc;
    a.errors = a.changed + 16;
    a.unsettled = a.changed + 17;
    HIP_TRY(static_cast<hipError_t>(cached_host_malloc(reinterpret_cast<void**>(&e->h_flags), kFlagWords * sizeof(uint32_t))));
    *out = e.release();
    return IFHIP_OK;
}

static int entropy_create_impl(ifhip_jpeg_entropy** out, const uint8_t* const* files, const size_t* lengths, uint32_t n_images) {
    if (!out) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *out = nullptr;
    if (!files || !lengths || n_images == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: empty batch");
    if (int arc = require_gfx950(nullptr)) return arc;
    // Host preparation runs on a few threads, one file at a time each: parsing and un-stuffing are independent per file
    // and would otherwise take several times longer than the GPU needs to decode the batch.
    std::vector<std::unique_ptr<ifhip_jpeg_prepared, GivePrepared>> prep(n_images);
    std::vector<int> rcs(n_images, IFHIP_OK);
    std::vector<std::string> messages(n_images);
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const uint32_t n_threads = std::min<uint32_t>(std::min<uint32_t>(n_images, hw), 16u);
    // Workers never let an exception escape (a bad_alloc on a huge scan becomes that file's error), and a thread that
    // cannot be created (container thread limits) leaves its share of the files to the calling thread.
    auto guarded = [&](uint32_t i) {
        try {
            ifhip_jpeg_prepared* one = nullptr;
            rcs[i] = prepare_impl(&one, files[i], lengths[i], i);
            if (rcs[i]) messages[i] = last_error();
            prep[i].reset(one);
        }
        catch (const std::bad_alloc&) { rcs[i] = IFHIP_ALLOCATION_FAILED; messages[i] = "AllocationFailed: host memory while preparing the scan"; }
        catch (const std::exception& ex) { rcs[i] = IFHIP_INVALID_STATE; messages[i] = std::string("InvalidState: ") + ex.what(); }
    };
    {
        std::vector<std::thread> pool;
        std::vector<uint32_t> inline_lanes{0u};
        for (uint32_t t = 1; t < n_threads; ++t) {
            try { pool.emplace_back([&, t] { for (uint32_t i = t; i < n_images; i += n_threads) guarded(i); }); }
            catch (const std::exception&) { inline_lanes.push_back(t); }
        }
        for (uint32_t t : inline_lanes)
            for (uint32_t i = t; i < n_images; i += n_threads) guarded(i);
        for (auto& th : pool) th.join();
    }
    for (uint32_t img = 0; img < n_images; ++img)                              // errors in file order
        if (rcs[img]) return fail(rcs[img], "%s", messages[img].c_str());
    std::vector<ifhip_jpeg_prepared*> raw(n_images);
    for (uint32_t img = 0; img < n_images; ++img) raw[img] = prep[img].get();
    return create_prepared_impl(out, raw.data(), n_images);
}

extern "C" {

int ifhip_jpeg_entropy_prepare(ifhip_jpeg_prepared** out, const uint8_t* jpeg, size_t len) {
    if (!out) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *out = nullptr;
    if (!jpeg) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file");
    return c_entry(" while preparing the scan", [&] { return prepare_impl(out, jpeg, len, 0); });
}
void ifhip_jpeg_prepared_destroy(ifhip_jpeg_prepared* p) { give_prepared(p); }
int ifhip_jpeg_prepared_upload(ifhip_jpeg_prepared* p, void* hip_stream) {
    if (!p) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null handle");
    if (p->d_words || !p->n_words) return IFHIP_OK;
    int dev = -1;
    if (int arc = require_gfx950(&dev)) return arc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (p->uploaded && p->event_device != dev) { (void)hipEventDestroy(p->uploaded); p->uploaded = nullptr; }   // (a recycled handle, last used on another device)
    if (!p->uploaded) { HIP_TRY(hipEventCreateWithFlags(&p->uploaded, hipEventDisableTiming)); p->event_device = dev; }
    HIP_TRY(DEV_MALLOC(&p->d_words, p->n_words * sizeof(uint32_t)));
    p->d_device = dev;
    hipError_t er = hipMemcpyAsync(p->d_words, p->words, p->n_words * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (er == hipSuccess) er = hipEventRecord(p->uploaded, st);
    if (er != hipSuccess) {
        (void)hipGetLastError();
        (void)static_cast<hipError_t>(ifhip::wait_stream(st));        // (whatever was queued is over before the block goes back)
        (void)DEV_FREE(p->d_words);
        p->d_words = nullptr; p->d_device = -1;
        return fail(IFHIP_GPU_ERROR, "GpuError: %s while queueing the scan upload", hipGetErrorString(er));
    }
    return IFHIP_OK;
}
int ifhip_jpeg_prepared_info(const ifhip_jpeg_prepared* p, uint32_t* width, uint32_t* height, int* n_components, uint8_t* h_samp3, uint8_t* v_samp3) {
    if (!p) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null handle");
    jpeg::report_frame(p->P, p->P, width, height, n_components, h_samp3, v_samp3);
    return IFHIP_OK;
}
int ifhip_jpeg_entropy_create_prepared(ifhip_jpeg_entropy** out, ifhip_jpeg_prepared* const* prepared, uint32_t n_images) {
    if (!out) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *out = nullptr;
    if (!prepared || n_images == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: empty batch");
    for (uint32_t i = 0; i < n_images; ++i) if (!prepared[i]) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null prepared file %u", i);
    return c_entry(" while assembling the batch", [&] { return create_prepared_impl(out, prepared, n_images); });
}

void ifhip_jpeg_entropy_destroy(ifhip_jpeg_entropy* e) { delete e; }

int ifhip_jpeg_entropy_create(ifhip_jpeg_entropy** out, const uint8_t* const* files, const size_t* lengths, uint32_t n_images) {
    // (*out is null on every failure: entropy_create_impl clears it first and create_prepared_impl sets it as its last step)
    return c_entry(" while preparing the batch", [&] { return entropy_create_impl(out, files, lengths, n_images); });
}

int ifhip_jpeg_entropy_info(const ifhip_jpeg_entropy* e, uint32_t* width, uint32_t* height, int* n_components, uint8_t* h_samp3,
                            uint8_t* v_samp3, uint32_t* blocks_w3, uint32_t* blocks_h3, uint32_t* n_subsequences, uint32_t* n_segments) {
    if (!e) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null handle");
    jpeg::report_frame(e->first, e->first, width, height, n_components, h_samp3, v_samp3, blocks_w3, blocks_h3);
    if (n_subsequences) *n_subsequences = e->a.n_sub;
    if (n_segments) *n_segments = e->a.n_seg;
    return IFHIP_OK;
}

int ifhip_jpeg_entropy_quant_tables(const ifhip_jpeg_entropy* e, uint16_t* qt_n3x64) {
    if (!e || !qt_n3x64) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    std::memcpy(qt_n3x64, e->qt.data(), e->qt.size() * sizeof(uint16_t));
    return IFHIP_OK;
}

// Decodes the whole batch into d_coef* (each [n_images][bh_c][bw_c][64] int16, natural order).  The fixpoint check needs
// its answer on the host, so the call synchronises the stream; *rounds (optional) reports how many synchronisation
// rounds ran (1 unless a correction crossed a workgroup boundary).
int ifhip_jpeg_entropy_decode_device(ifhip_jpeg_entropy* e, int16_t* d_coef0, int16_t* d_coef1, int16_t* d_coef2,
                                     uint32_t* rounds, void* hip_stream) {
    if (!e) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null handle");
    const ParsedJpeg& F = e->first;
    if (!d_coef0 || (F.ncomp == 3 && (!d_coef1 || !d_coef2))) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null coefficient plane");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != e->device) return fail(IFHIP_INVALID_STATE, "InvalidState: handle belongs to device %d, current device is %d", e->device, dev);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    EntropyArgs a = e->a;
    a.coef[0] = d_coef0; a.coef[1] = d_coef1; a.coef[2] = d_coef2;
    if ((reinterpret_cast<uintptr_t>(d_coef0) | reinterpret_cast<uintptr_t>(d_coef1) | reinterpret_cast<uintptr_t>(d_coef2)) & 15u)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: coefficient planes must be 16-byte aligned");
    const dim3 sync_grid((a.n_sub + kSyncLanes - 1u) / kSyncLanes), sync_block(kSyncLanes);
    const dim3 round_grid((a.n_sub + kOwnSubs - 1u) / kOwnSubs);
    const uint32_t max_rounds = a.n_sub + 2u;
    // Round 0 (speculative decode with the fixpoint iteration inside every workgroup; it also clears the flags), the
    // count pass (which checks that every sub-sequence was decoded from its predecessor's exit: with the warm-up lanes of
    // round 0 no correction crosses a workgroup boundary) and the write pass are enqueued back to back -- three launches,
    // every launch boundary costs ~8 us -- and the host looks at the flags once.  If the count pass found an unsettled
    // sub-sequence, further rounds run (one look per round) and count + write are repeated: the write pass stores every
    // block in full, so the repeat simply overwrites.
    uint32_t r = 0;
    a.round = 0u;
    hipLaunchKernelGGL(entropy_round_kernel, round_grid, sync_block, 0, st, a);
    HIP_TRY(hipGetLastError());
    for (;;) {
        a.round = r;
        hipLaunchKernelGGL(entropy_count_kernel, sync_grid, sync_block, 0, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(entropy_write_kernel, dim3((a.n_sub + kWriteLanes - 1u) / kWriteLanes), dim3(kWriteLanes), 0, st, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(e->h_flags, a.changed, kFlagWords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(static_cast<hipError_t>(ifhip::wait_stream(st)));
        if (e->h_flags[17] == 0u) break;                             // every sub-sequence starts where its predecessor ended
        for (;;) {                                                   // rare: corrections across workgroups
            ++r;
            if (r >= max_rounds) return fail(IFHIP_INVALID_STATE, "InvalidState: entropy decode did not converge");
            HIP_TRY(hipMemsetAsync(a.changed + (r & 15u), 0, sizeof(uint32_t), st));
            a.round = r;
            hipLaunchKernelGGL(entropy_round_kernel, round_grid, sync_block, 0, st, a);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(e->h_flags, a.changed, kFlagWords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(static_cast<hipError_t>(ifhip::wait_stream(st)));
            if (e->h_flags[r & 15u] == 0u) break;
        }
        HIP_TRY(hipMemsetAsync(a.errors, 0, 2u * sizeof(uint32_t), st));     // flags of the discarded count and write passes
    }
    if (rounds) *rounds = r + 1u;
    if (e->h_flags[16]) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: corrupt entropy-coded data (flags 0x%x)", e->h_flags[16]);
    return IFHIP_OK;
}

}  // extern "C"
