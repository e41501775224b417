// jpeg_encode_progressive.hip -- gfx950 kernels of the device entropy coder's two flagged forms: IFHIP_JPEG_OPTIMIZE_HUFFMAN
// (one sequential scan against per-image optimal tables) and IFHIP_JPEG_PROGRESSIVE (jpeg_simple_progression's scans, every
// scan with optimal tables of its own).  Byte-identical to the host writer (csrc/jpeg_write.cpp) and so to libjpeg-turbo.
//
// Progressive ENCODING is data-parallel: every coefficient is known, a block's symbols in a scan depend on the block alone
// plus two carried quantities -- the DC predecessor (it lies in the plane) and the end-of-band run the block belongs to,
// which a walk over maximal runs resolves (prog_run_kernel).  Launches per call, all images and all scans in each, no host
// round trip between them:
//   stats   (items)   head symbols -> LDS histograms -> hist[image][slot]; flags[item] = head | tail | correction bits
//   runs    (chunks)  one wave per 2048 items of an AC scan: the runs that start there, cut at 0x7FFF blocks / > 937 bits;
//                     eob[first item of a run] = its length, the EOBn symbols counted
//   tables  (slots)   one wave per (image, table): jpeg_gen_optimal_table, the DHT segment and the encode table
//   count   (items)   bits per item -> per-workgroup sums
//   scan              per scan: prefixes, bytes, the scan's first chunk in the word stream (every scan starts on a chunk)
//   write   (items)   bits into the zeroed word stream (first and last word of an item ORed, the ones between owned)
//   ff / scan / stuff as the baseline coder's, per chunk; the scan also places every segment, the stuffing pass writes them
// The arithmetic lives in jpeg_encode_progressive_core.hpp, shared with tests/enc_progressive_emulate.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>

#include "block_scan.hpp"
#include "hip_entry.hpp"
#include "jpeg_encode_progressive.hpp"
#include "jpeg_encode_progressive_core.hpp"
#include "jpeg_huff_wave.hpp"
#include "stage_scratch.hpp"

namespace ifhip {

namespace {

// per-image words of the small results: bytes per scan, first chunk per scan (+ the total), data offset per scan, file length, DHT lengths
constexpr uint32_t kSmBytes = 0, kSmChunk0 = 10, kSmDataOff = 21, kSmFileLen = 31, kSmDhtLen = 32, kSmWords = 48;

struct ProgArgs {
    EncGeom g;
    const ProgPlan* plan;
    const int16_t* coef[3];
    size_t plane_blocks[3];
    uint32_t n_images, item_cap, wg_cap, max_chunks;
    uint16_t* flags;                // [n_images][item_cap]
    uint16_t* eob;                  // [n_images][item_cap] run length at a run's first item, else 0
    uint16_t* nbits;                // [n_images][item_cap]
    uint32_t* hist;                 // [n_images][kProgMaxSlots][256]
    uint32_t* codes;                // [n_images][kProgMaxSlots][256] code | length << 16
    uint8_t* dht;                   // [n_images][kProgMaxSlots][kProgDhtPitch]
    uint32_t* wg_bits;              // [n_images][wg_cap] sums, then exclusive prefixes inside the scan
    uint32_t* small;                // [n_images][kSmWords]
    uint32_t* words;                // [n_images][cap_words] zero between calls
    size_t cap_words;
    uint32_t* ff;                   // [n_images][chunk_cap]
    uint32_t chunk_cap;
    uint32_t* status;
    uint32_t* status_out;
    const uint8_t* header;
    uint8_t* files;
    size_t file_pitch;
    uint32_t* lengths;
};

constexpr uint32_t kBlkPitch = 33;  // dwords per staged block in LDS (jpeg_encode.hip)

struct DeviceStore {
    __device__ __forceinline__ static void shared(uint32_t* p, uint32_t v) { atomicOr(p, v); }
    __device__ __forceinline__ static void owned(uint32_t* p, uint32_t v) { *p = v; }
};
struct LdsAdd {
    __device__ __forceinline__ static void add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
};
struct LdsCoef {
    const uint32_t* w;
    __device__ __forceinline__ int32_t operator()(int k) const { return reinterpret_cast<const int16_t*>(w)[enc_slot(static_cast<uint32_t>(k))]; }
    __device__ __forceinline__ uint32_t pair(int j) const { return w[j]; }
};

// the scan a workgroup of the block passes belongs to (uniform)
__device__ __forceinline__ uint32_t scan_of_wg(const ProgPlan& P, uint32_t wg) {
    uint32_t j = 0;
    while (j + 1u < P.nscans && wg >= P.scan[j + 1u].wg0) ++j;
    return j;
}

// The workgroup's (up to) 256 blocks into LDS in the walk's slot order: coalesced 16-byte loads, eight lanes per block, as
// the baseline coder stages them.  `n_here`: blocks of the tile (lanes behind it hold no address and name the last block).
__device__ __forceinline__ void stage_tile(const int16_t* mine, uint32_t n_here, uint32_t* blk, const int16_t** addr) {
    const uint32_t tid = threadIdx.x;
    addr[tid] = mine;
    __syncthreads();
    const uint32_t piece = tid & 7u;
    uint32_t pos[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pos[i] = enc_slot(static_cast<uint32_t>(enc_zigzag_position(static_cast<int>(piece) * 8 + i)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) const u32x4 global_u32x4;
    const uint32_t last = n_here - 1u;
    u32x4 v[8];
#pragma unroll
    for (uint32_t it = 0; it < 8u; ++it) {
        const int16_t* p = addr[min((it * kEncBlocksPerWg + tid) >> 3, last)];
        v[it] = *reinterpret_cast<global_u32x4*>(reinterpret_cast<uintptr_t>(p + piece * 8u));
    }
    uint16_t* d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = reinterpret_cast<uint16_t*>(blk + (tid >> 3) * kBlkPitch) + pos[i];
#pragma unroll
    for (uint32_t it = 0; it < 8u; ++it) {
        constexpr uint32_t kStep = (kEncBlocksPerWg / 8u) * kBlkPitch * 2u;
        d[0][it * kStep] = static_cast<uint16_t>(v[it].x); d[1][it * kStep] = static_cast<uint16_t>(v[it].x >> 16);
        d[2][it * kStep] = static_cast<uint16_t>(v[it].y); d[3][it * kStep] = static_cast<uint16_t>(v[it].y >> 16);
        d[4][it * kStep] = static_cast<uint16_t>(v[it].z); d[5][it * kStep] = static_cast<uint16_t>(v[it].z >> 16);
        d[6][it * kStep] = static_cast<uint16_t>(v[it].w); d[7][it * kStep] = static_cast<uint16_t>(v[it].w >> 16);
    }
    __syncthreads();
}

// one item of a progressive scan against `out`
template <class Out>
__device__ __forceinline__ uint32_t prog_item(uint32_t kind, uint32_t Ss, uint32_t Se, uint32_t Al, const LdsCoef& coef, int32_t coef0,
                                              int32_t pred, uint32_t eobrun, Out& out) {
    if (kind == kProgDcFirst) return prog_dc_first(coef0, pred, Al, out);
    if (kind == kProgDcRefine) { out.raw(static_cast<uint32_t>(coef0 >> Al) & 1u, 1u); return 0u; }
    if (kind == kProgAcFirst) return prog_ac_first(coef, Ss, Se, Al, eobrun, out);
    return prog_ac_refine(coef, Ss, Se, Al, eobrun, out);
}

// PASS 0: statistics + flags; 1: bit counts; 2: write
template <int PASS>
__global__ __launch_bounds__(256) void prog_block_kernel(const ProgArgs a, const uint32_t which) {
    __shared__ uint32_t blk[kEncBlocksPerWg * kBlkPitch];
    __shared__ const int16_t* addr[kEncBlocksPerWg];
    __shared__ uint32_t tabs[1024];                        // dc0, ac0, dc1, ac1: encode tables (pass 0: the histograms)
    __shared__ uint32_t ident[PASS == 0 ? 256 : 1];
    __shared__ uint32_t scratch[8];
    const ProgPlan& P = a.plan[which];
    const uint32_t tid = threadIdx.x, img = blockIdx.y, wg = blockIdx.x;
    if (PASS == 2 && a.status[img]) return;                // (uniform: a dropped image writes nothing)
    const uint32_t j = scan_of_wg(P, wg);
    const ProgScan& sc = P.scan[j];
    const uint32_t kind = sc.kind, Ss = sc.Ss, Se = sc.Se, Al = sc.Al, nblocks = sc.nblocks;
    if (PASS == 0 && kind == kProgDcRefine) return;        // raw bits: no symbol, no run
    const uint32_t s0 = (wg - sc.wg0) * kEncBlocksPerWg, s = s0 + tid;
    const bool valid = s < nblocks;
    const int16_t* mine = nullptr;
    const int16_t* before = nullptr;
    uint32_t t = 0;
    if (valid) {
        const EncBlockRef r = prog_locate(a.g, sc, s);
        const uint64_t planes[3] = {reinterpret_cast<uint64_t>(a.coef[0]), reinterpret_cast<uint64_t>(a.coef[1]), reinterpret_cast<uint64_t>(a.coef[2])};
        const uint64_t per_image[3] = {a.plane_blocks[0], a.plane_blocks[1], a.plane_blocks[2]};
        mine = reinterpret_cast<const int16_t*>(enc_sel3(planes, r.comp)) + (img * enc_sel3(per_image, r.comp) + r.offset) * 64u;
        if (r.pred_offset != 0xFFFFFFFFu) before = mine + (static_cast<ptrdiff_t>(r.pred_offset) - static_cast<ptrdiff_t>(r.offset)) * 64;
        t = r.comp ? 512u : 0u;
    }
    const bool dc_only = kind == kProgDcFirst || kind == kProgDcRefine;     // (uniform)
    int32_t coef0 = 0, pred = 0;
    if (dc_only) {
        if (valid) { coef0 = *mine; pred = before ? *before : 0; }
    } else {
        stage_tile(mine, min(kEncBlocksPerWg, nblocks - s0), blk, addr);
        if (kind == kProgSeq && before) pred = *before;
    }
    if (PASS == 0) {
        for (uint32_t i = tid; i < 1024u; i += kEncBlocksPerWg) tabs[i] = 0u;
        ident[tid] = tid;
    } else {
        const uint32_t* codes = a.codes + static_cast<size_t>(img) * kProgMaxSlots * 256u;
        for (uint32_t i = tid; i < 1024u; i += kEncBlocksPerWg) {
            const uint32_t slot = sc.slot[i >> 8];
            tabs[i] = slot == kProgNoSlot ? 0u : codes[slot * 256u + (i & 255u)];
        }
    }
    __syncthreads();
    const size_t item = static_cast<size_t>(img) * a.item_cap + sc.item0 + s;
    const LdsCoef coef{blk + tid * kBlkPitch};
    uint32_t* const table = tabs + t + (kind >= kProgAcFirst ? 256u : 0u);
    if (PASS == 0) {
        if (valid) {
            if (kind == kProgSeq) {
                EncStatSink<LdsAdd> sink{tabs + t, tabs + t + 256u};
                enc_block(coef, pred, ident, ident, sink);
            } else {
                ProgCounted<LdsAdd> out{table};
                const uint32_t f = prog_item(kind, Ss, Se, Al, coef, coef0, pred, 0u, out);
                if (kind >= kProgAcFirst) a.flags[item] = static_cast<uint16_t>(f);
            }
        }
        __syncthreads();
        uint32_t* hist = a.hist + static_cast<size_t>(img) * kProgMaxSlots * 256u;
        for (uint32_t i = tid; i < 1024u; i += kEncBlocksPerWg) {
            const uint32_t slot = sc.slot[i >> 8], c = tabs[i];
            if (c && slot != kProgNoSlot) atomicAdd(hist + slot * 256u + (i & 255u), c);
        }
        return;
    }
    const uint32_t eobrun = valid && kind >= kProgAcFirst ? a.eob[item] : 0u;
    if (PASS == 1) {
        uint32_t bits = 0, bad = 0;
        if (valid) {
            EncCountSink sink;
            if (kind == kProgSeq) {
                bad = enc_block(coef, pred, tabs + t, tabs + t + 256u, sink);
            } else {
                ProgCoded<EncCountSink> out{sink, table};
                bad = prog_item(kind, Ss, Se, Al, coef, coef0, pred, eobrun, out) & kProgBad;
            }
            bits = sink.bits;
            a.nbits[item] = static_cast<uint16_t>(bits);
        }
        uint32_t total;
        block_exclusive_scan<256>(bits, scratch, &total);
        if (tid == 0u) a.wg_bits[static_cast<size_t>(img) * a.wg_cap + wg] = total;
        if (bad) atomicOr(a.status + img, kEncBadCoef);
        return;
    }
    // PASS 2
    const uint32_t mine_bits = valid ? a.nbits[item] : 0u;
    uint32_t total;
    const uint32_t local = block_exclusive_scan<256>(mine_bits, scratch, &total);
    const uint32_t chunk0 = a.small[static_cast<size_t>(img) * kSmWords + kSmChunk0 + j];
    const uint32_t base = chunk0 * (kEncChunkBytes * 8u) + a.wg_bits[static_cast<size_t>(img) * a.wg_cap + wg];
    // (an item without bits -- a block inside an end-of-band run -- touches no word; the scan's last item still pads)
    if (valid && (mine_bits != 0u || s == nblocks - 1u)) {
        EncWordSink<DeviceStore> sink(a.words + static_cast<size_t>(img) * a.cap_words, base + local);
        if (kind == kProgSeq) {
            enc_block(coef, pred, tabs + t, tabs + t + 256u, sink);
        } else {
            ProgCoded<EncWordSink<DeviceStore>> out{sink, table};
            prog_item(kind, Ss, Se, Al, coef, coef0, pred, eobrun, out);
        }
        if (s == nblocks - 1u) {                           // jchuff.c flush_bits: every scan's last byte is filled with 1 bits
            const uint32_t pad = (8u - sink.bits_in_last_byte()) & 7u;
            if (pad) sink.put((1u << pad) - 1u, pad);
        }
        sink.finish();
    }
}

// ---- runs ---------------------------------------------------------------------------------------------------------------
struct DeviceWave {
    const uint16_t* flags;          // the scan's items
    uint16_t* eob;
    uint32_t* cnt;                  // LDS: EOBn symbols by n
    uint32_t lane;
    uint32_t tail = 0, pb = 0, prev = 0;
    uint64_t H = 0, T = 0;
    __device__ __forceinline__ void load(uint32_t base, uint32_t nv) {
        const uint32_t f = lane < nv ? flags[base + lane] : 0u;
        tail = (f >> 1) & 1u;
        H = __ballot(f & 1u);
        T = __ballot(tail);
        pb = wave_inclusive_scan(tail ? prog_ncorr(f) : 0u, lane);
        prev = base ? (flags[base - 1u] >> 1) & 1u : 0u;
    }
    __device__ __forceinline__ uint64_t heads() const { return H; }
    __device__ __forceinline__ uint64_t tails() const { return T; }
    __device__ __forceinline__ bool prev_tail() const { return prev != 0u; }
    __device__ __forceinline__ uint32_t incl_bits(uint32_t l) const { return __shfl(pb, static_cast<int>(l), 64); }
    __device__ __forceinline__ uint64_t crossing(uint32_t q, uint32_t h, uint32_t len0, uint32_t bits0, uint32_t ptq, uint32_t pbq) const {
        const uint32_t pt = static_cast<uint32_t>(__builtin_popcountll(T & prog_below(lane + 1u)));
        return __ballot(prog_run_crosses(lane, q, h, tail != 0u, pt, pb, ptq, pbq, len0, bits0));
    }
    __device__ __forceinline__ void emit(uint32_t start, uint32_t len, uint32_t) {
        if (lane == 0u) { eob[start] = static_cast<uint16_t>(len); cnt[31u - static_cast<uint32_t>(__builtin_clz(len))]++; }
    }
};

__global__ __launch_bounds__(64) void prog_run_kernel(const ProgArgs a, const uint32_t which) {
    __shared__ uint32_t cnt[16];
    const ProgPlan& P = a.plan[which];
    const uint32_t lane = threadIdx.x, img = blockIdx.y, chunk = blockIdx.x;
    uint32_t j = 0;
    for (uint32_t i = 0; i < P.nscans; ++i) if (P.scan[i].kind >= kProgAcFirst && P.scan[i].chunk0 <= chunk) j = i;
    const ProgScan& sc = P.scan[j];
    if (lane < 16u) cnt[lane] = 0u;
    __syncthreads();
    const uint32_t n = sc.nblocks, c0 = (chunk - sc.chunk0) * kProgRunChunk, c1 = min(c0 + kProgRunChunk, n);
    const size_t first = static_cast<size_t>(img) * a.item_cap + sc.item0;
    DeviceWave w{a.flags + first, a.eob + first, cnt, lane};
    prog_run_chunk(w, c0, c1, n);
    __syncthreads();
    const uint32_t slot = sc.slot[sc.comp ? 3 : 1];
    if (lane < 15u && cnt[lane]) atomicAdd(a.hist + (static_cast<size_t>(img) * kProgMaxSlots + slot) * 256u + (lane << 4), cnt[lane]);
}

// ---- tables -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void prog_table_kernel(const ProgArgs a, const uint32_t which) {
    __shared__ uint32_t freq[257], codesize[257], bits[33], codes[256];
    __shared__ int32_t others[257];
    __shared__ uint8_t vals[256], dht[kProgDhtPitch];
    __shared__ uint32_t dht_len;
    const ProgPlan& P = a.plan[which];
    const uint32_t lane = threadIdx.x, img = blockIdx.y, slot = blockIdx.x;
    const size_t at = static_cast<size_t>(img) * kProgMaxSlots + slot;
    huff_init(a.hist + at * 256u, lane, freq, codesize, others);
    for (uint32_t i = lane; i < 256u; i += 64u) { codes[i] = 0u; vals[i] = 0; }
    __syncthreads();
    huff_wave_merge(lane, freq, codesize, others);
    if (lane == 0u) huff_limit(codesize, bits);
    for (uint32_t i = lane; i < 256u; i += 64u) if (codesize[i] && codesize[i] <= 32u) vals[huff_rank(codesize, i)] = static_cast<uint8_t>(i);
    __syncthreads();
    if (lane == 0u) dht_len = huff_emit(bits, vals, P.slot_id[slot], dht, codes);
    __syncthreads();
    for (uint32_t i = lane; i < 256u; i += 64u) a.codes[at * 256u + i] = codes[i];
    for (uint32_t i = lane; i < dht_len; i += 64u) a.dht[at * kProgDhtPitch + i] = dht[i];
    if (lane == 0u) a.small[static_cast<size_t>(img) * kSmWords + kSmDhtLen + slot] = dht_len;
}

// ---- scans --------------------------------------------------------------------------------------------------------------
// mode 0: per scan the exclusive prefixes of the workgroups' bit sums, the scan's bytes and its first chunk in the word stream;
// mode 1: the exclusive prefixes of the chunks' 0xFF counts, then where every scan's data lies in the file and the file's length
__global__ __launch_bounds__(1024) void prog_scan_kernel(const ProgArgs a, const uint32_t which, const int mode) {
    __shared__ uint32_t scratch[20];
    const ProgPlan& P = a.plan[which];
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    uint32_t* sm = a.small + static_cast<size_t>(img) * kSmWords;
    if (mode == 0) {
        uint64_t chunk_at = 0;
        bool overflow = false;
        for (uint32_t j = 0; j < P.nscans; ++j) {
            const ProgScan& sc = P.scan[j];
            const uint32_t n = (sc.nblocks + kEncBlocksPerWg - 1u) / kEncBlocksPerWg;
            uint32_t* v = a.wg_bits + static_cast<size_t>(img) * a.wg_cap + sc.wg0;
            uint32_t carry = 0;
            for (uint32_t base = 0; base < n; base += 1024u) {
                const uint32_t i = base + tid, x = i < n ? v[i] : 0u;
                uint32_t total;
                const uint32_t ex = block_exclusive_scan<1024>(x, scratch, &total);
                if (i < n) v[i] = carry + ex;
                overflow |= carry + total < carry;
                carry += total;
            }
            const uint32_t bytes = static_cast<uint32_t>((static_cast<uint64_t>(carry) + 7u) >> 3);
            if (tid == 0u) { sm[kSmBytes + j] = bytes; sm[kSmChunk0 + j] = static_cast<uint32_t>(chunk_at); }
            chunk_at += (bytes + kEncChunkBytes - 1u) / kEncChunkBytes;
            overflow |= chunk_at > a.max_chunks;           // (also keeps every bit position below 2^32)
        }
        if (tid == 0u) {
            sm[kSmChunk0 + P.nscans] = static_cast<uint32_t>(chunk_at);
            if (overflow) atomicOr(a.status + img, kEncScanOverflow);
        }
        return;
    }
    const uint32_t st = a.status[img], n = st ? 0u : sm[kSmChunk0 + P.nscans];
    uint32_t* v = a.ff + static_cast<size_t>(img) * a.chunk_cap;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024u) {
        const uint32_t i = base + tid, x = i < n ? v[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<1024>(x, scratch, &total);
        if (i < n) v[i] = carry + ex;
        carry += total;
    }
    __syncthreads();
    if (tid == 0u && !st) {                                // the per-image scan over segment lengths: where every scan's data starts
        uint64_t off = P.header0_len;
        for (uint32_t j = 0; j < P.nscans; ++j) {
            const ProgScan& sc = P.scan[j];
            for (uint32_t i = 0; i < sc.ndht; ++i) off += sm[kSmDhtLen + sc.dht[i]];
            off += sc.sos_len;
            sm[kSmDataOff + j] = static_cast<uint32_t>(off);
            const uint32_t ff_end = j + 1u < P.nscans ? v[sm[kSmChunk0 + j + 1u]] : carry;
            off += static_cast<uint64_t>(sm[kSmBytes + j]) + (ff_end - v[sm[kSmChunk0 + j]]);
        }
        off += 2u;
        sm[kSmFileLen] = off > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(off);
    }
}

// the scan a chunk of the word stream belongs to; c0s: the scans' first chunks (LDS)
__device__ __forceinline__ uint32_t scan_of_chunk(const uint32_t* c0s, uint32_t nscans, uint32_t chunk) {
    uint32_t j = 0;
    while (j + 1u < nscans && chunk >= c0s[j + 1u]) ++j;
    return j;
}

__global__ __launch_bounds__(256) void prog_ff_count_kernel(const ProgArgs a, const uint32_t which) {
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sm[kSmWords];
    const ProgPlan& P = a.plan[which];
    const uint32_t tid = threadIdx.x, img = blockIdx.y;
    if (a.status[img]) return;
    if (tid < kSmWords) sm[tid] = a.small[static_cast<size_t>(img) * kSmWords + tid];
    __syncthreads();
    const uint32_t chunks = sm[kSmChunk0 + P.nscans];
    const uint4* w = reinterpret_cast<const uint4*>(a.words + static_cast<size_t>(img) * a.cap_words);
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint32_t j = scan_of_chunk(sm + kSmChunk0, P.nscans, chunk);
        const uint32_t at = (chunk - sm[kSmChunk0 + j]) * kEncChunkBytes + tid * 16u;
        uint32_t c = 0;
        if (at < sm[kSmBytes + j]) {
            const uint4 v = w[(static_cast<size_t>(chunk) * kEncChunkBytes + tid * 16u) >> 4];
            c = enc_count_ff(v.x) + enc_count_ff(v.y) + enc_count_ff(v.z) + enc_count_ff(v.w);
        }
        uint32_t total;
        block_exclusive_scan<256>(c, scratch, &total);
        if (tid == 0u) a.ff[static_cast<size_t>(img) * a.chunk_cap + chunk] = total;
    }
}

__global__ __launch_bounds__(256) void prog_stuff_kernel(const ProgArgs a, const uint32_t which) {
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sm[kSmWords];
    __shared__ uint8_t obuf[2u * kEncChunkBytes];
    const ProgPlan& P = a.plan[which];
    const uint32_t tid = threadIdx.x, img = blockIdx.y;
    const uint32_t st = a.status[img];
    if (tid < kSmWords) sm[tid] = a.small[static_cast<size_t>(img) * kSmWords + tid];
    __syncthreads();
    const uint32_t chunks = st ? 0u : sm[kSmChunk0 + P.nscans];
    const uint32_t file_len = sm[kSmFileLen];
    const bool fits = !st && file_len <= a.file_pitch;
    uint4* w = reinterpret_cast<uint4*>(a.words + static_cast<size_t>(img) * a.cap_words);
    uint8_t* out = a.files + static_cast<size_t>(img) * a.file_pitch;
    if (blockIdx.x == 0u) {
        if (fits) {
            for (uint32_t i = tid; i < P.header0_len; i += 256u) out[i] = i == P.sof_marker_at && P.progressive ? 0xC2 : a.header[i];
            for (uint32_t j = 0; j < P.nscans; ++j) {      // DHT segments of the scan's tables, then its SOS, in front of its data
                const ProgScan& sc = P.scan[j];
                uint32_t at = sm[kSmDataOff + j] - sc.sos_len;
                for (uint32_t i = tid; i < sc.sos_len; i += 256u) out[at + i] = sc.sos[i];
                for (uint32_t k = sc.ndht; k-- > 0u;) {
                    const uint32_t slot = sc.dht[k], len = sm[kSmDhtLen + slot];
                    at -= len;
                    const uint8_t* src = a.dht + (static_cast<size_t>(img) * kProgMaxSlots + slot) * kProgDhtPitch;
                    for (uint32_t i = tid; i < len; i += 256u) out[at + i] = src[i];
                }
            }
            if (tid == 0u) { out[file_len - 2u] = 0xFF; out[file_len - 1u] = 0xD9; }
        }
        if (tid == 0u) {
            a.lengths[img] = fits ? file_len : 0u;
            if (a.status_out) a.status_out[img] = st | (!fits && !st ? kEncFileOverflow : 0u);
        }
    }
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint32_t j = scan_of_chunk(sm + kSmChunk0, P.nscans, chunk);
        const uint32_t rel = chunk - sm[kSmChunk0 + j], bytes = sm[kSmBytes + j];
        const uint32_t at = rel * kEncChunkBytes + tid * 16u;
        const size_t wi = (static_cast<size_t>(chunk) * kEncChunkBytes + tid * 16u) >> 4;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        uint32_t c = 0;
        if (at < bytes) {
            v = w[wi];
            w[wi] = make_uint4(0u, 0u, 0u, 0u);            // the stream is zero again for the next call
            c = enc_count_ff(v.x) + enc_count_ff(v.y) + enc_count_ff(v.z) + enc_count_ff(v.w);
        }
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<256>(c, scratch, &total);
        if (!fits) continue;                               // (uniform)
        if (at < bytes) {
            uint8_t* d = obuf + tid * 16u + ex;
            const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
            const uint32_t nb = bytes - at < 16u ? bytes - at : 16u;
#pragma unroll
            for (uint32_t q = 0; q < 16u; ++q) {
                if (q < nb) {
                    const uint32_t b = (ws[q >> 2] >> (8u * (q & 3u))) & 255u;
                    *d++ = static_cast<uint8_t>(b);
                    if (b == 255u) *d++ = 0u;
                }
            }
        }
        __syncthreads();
        const uint32_t left = bytes - rel * kEncChunkBytes, n_in = left < kEncChunkBytes ? left : kEncChunkBytes;
        const uint32_t* ffv = a.ff + static_cast<size_t>(img) * a.chunk_cap;
        uint8_t* dst = out + sm[kSmDataOff + j] + rel * kEncChunkBytes + (ffv[chunk] - ffv[sm[kSmChunk0 + j]]);
        for (uint32_t i = tid; i < n_in + total; i += 256u) dst[i] = obuf[i];
        __syncthreads();
    }
}

// stream capacity of one image for a plan: the caller's bound or the worst case, in whole chunks, plus the chunk every scan
// may leave partly empty (each scan starts on a chunk boundary)
uint64_t stream_cap_bytes(const ProgPlan& p, size_t scan_capacity) {
    const uint64_t worst = prog_worst_stream_bytes(p);
    const uint64_t cap = scan_capacity ? std::min<uint64_t>(scan_capacity, worst) : worst;
    return (cap + kEncChunkBytes - 1u) / kEncChunkBytes * kEncChunkBytes + static_cast<uint64_t>(p.nscans + 1u) * kEncChunkBytes;
}

}  // namespace

struct ProgScratch {
    EncGeom g;
    ProgPlan plan[2];               // [0] optimised tables, [1] progressive
    uint32_t max_images = 0, item_cap = 0, wg_cap = 0, chunk_cap = 0, max_chunks[2] = {0, 0};
    size_t cap_words = 0;
    ProgPlan* d_plan = nullptr;
    uint16_t *d_flags = nullptr, *d_eob = nullptr, *d_nbits = nullptr;
    uint32_t *d_hist = nullptr, *d_codes = nullptr, *d_wg_bits = nullptr, *d_small = nullptr, *d_words = nullptr, *d_ff = nullptr, *d_status = nullptr;
    uint8_t* d_dht = nullptr;
    StageScratch blocks{&d_plan, &d_flags, &d_eob, &d_nbits, &d_hist, &d_codes, &d_wg_bits, &d_small, &d_words, &d_ff, &d_status, &d_dht};
};

size_t prog_max_file_bytes(const EncGeom& g, uint32_t width, uint32_t height, int flags, size_t scan_capacity) {
    ProgPlan p;
    prog_make_plan(g, width, height, flags, &p);
    const uint64_t cap = stream_cap_bytes(p, scan_capacity);
    if (cap * 8u >= (1ull << 32)) return 0;
    return static_cast<size_t>(prog_segment_bytes(p) + 2u * cap);
}

int prog_scratch_create(ProgScratch** out, const EncGeom& g, uint32_t width, uint32_t height, uint32_t max_images, size_t scan_capacity) {
    *out = nullptr;
    std::unique_ptr<ProgScratch> s(new ProgScratch);
    s->g = g;
    s->max_images = max_images;
    uint64_t cap = 0;
    for (int m = 0; m < 2; ++m) {
        prog_make_plan(g, width, height, m ? 3 : 1, &s->plan[m]);
        const uint64_t c = stream_cap_bytes(s->plan[m], scan_capacity);
        if (c * 8u >= (1ull << 32))
            return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a stream of up to %llu bytes per image exceeds 32-bit bit positions (bound it with scan_capacity)",
                        static_cast<unsigned long long>(c));
        s->max_chunks[m] = static_cast<uint32_t>(c / kEncChunkBytes);
        cap = std::max(cap, c);
        s->item_cap = std::max(s->item_cap, s->plan[m].n_items);
        s->wg_cap = std::max(s->wg_cap, s->plan[m].n_wg);
    }
    s->item_cap = (s->item_cap + 7u) & ~7u;
    s->cap_words = static_cast<size_t>(cap / 4u);
    s->chunk_cap = static_cast<uint32_t>(cap / kEncChunkBytes);
    const size_t n = max_images;
    if (int rc = s->blocks.ensure([&]() -> int {
        HIP_TRY(DEV_MALLOC(&s->d_plan, sizeof s->plan));
        HIP_TRY(DEV_MALLOC(&s->d_flags, n * s->item_cap * sizeof(uint16_t)));
        HIP_TRY(DEV_MALLOC(&s->d_eob, n * s->item_cap * sizeof(uint16_t)));
        HIP_TRY(DEV_MALLOC(&s->d_nbits, n * s->item_cap * sizeof(uint16_t)));
        HIP_TRY(DEV_MALLOC(&s->d_hist, n * kProgMaxSlots * 256u * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_codes, n * kProgMaxSlots * 256u * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_wg_bits, n * s->wg_cap * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_small, n * kSmWords * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_words, n * s->cap_words * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_ff, n * s->chunk_cap * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_status, n * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_dht, n * kProgMaxSlots * kProgDhtPitch));
        return IFHIP_OK;
    })) return rc;
    HIP_TRY(static_cast<hipError_t>(copy_to_device(s->d_plan, s->plan, sizeof s->plan)));
    HIP_TRY(static_cast<hipError_t>(zero_device(s->d_words, n * s->cap_words * sizeof(uint32_t))));   // the stuffing pass keeps it zero from here on
    *out = s.release();
    return IFHIP_OK;
}

void prog_scratch_destroy(ProgScratch* s) { delete s; }
int prog_scratch_check_device(const ProgScratch* s) { return s->blocks.check_device(); }

int prog_encode(ProgScratch* s, const ProgCall& call, int flags, void* hip_stream) {
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint32_t which = (flags & 2) ? 1u : 0u, n = call.n_images;
    const ProgPlan& P = s->plan[which];
    ProgArgs a;
    std::memset(&a, 0, sizeof a);
    a.g = s->g;
    a.plan = s->d_plan;
    for (int c = 0; c < 3; ++c) { a.coef[c] = call.coef[c]; a.plane_blocks[c] = call.plane_blocks[c]; }
    a.n_images = n; a.item_cap = s->item_cap; a.wg_cap = s->wg_cap; a.max_chunks = s->max_chunks[which];
    a.flags = s->d_flags; a.eob = s->d_eob; a.nbits = s->d_nbits; a.hist = s->d_hist; a.codes = s->d_codes; a.dht = s->d_dht;
    a.wg_bits = s->d_wg_bits; a.small = s->d_small; a.words = s->d_words; a.cap_words = s->cap_words; a.ff = s->d_ff; a.chunk_cap = s->chunk_cap;
    a.status = s->d_status; a.status_out = call.status_out; a.header = call.d_header; a.files = call.files; a.file_pitch = call.file_pitch;
    a.lengths = call.lengths;
    HIP_TRY(hipMemsetAsync(s->d_status, 0, n * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(s->d_hist, 0, static_cast<size_t>(n) * kProgMaxSlots * 256u * sizeof(uint32_t), st));
    if (P.n_chunks) HIP_TRY(hipMemsetAsync(s->d_eob, 0, static_cast<size_t>(n) * s->item_cap * sizeof(uint16_t), st));
    const dim3 items_grid(P.n_wg, n);
    const dim3 chunk_grid(std::min<uint32_t>(s->max_chunks[which], 256u), n);
    hipLaunchKernelGGL(prog_block_kernel<0>, items_grid, dim3(256), 0, st, a, which);
    if (P.n_chunks) hipLaunchKernelGGL(prog_run_kernel, dim3(P.n_chunks, n), dim3(64), 0, st, a, which);
    hipLaunchKernelGGL(prog_table_kernel, dim3(P.nslots, n), dim3(64), 0, st, a, which);
    hipLaunchKernelGGL(prog_block_kernel<1>, items_grid, dim3(256), 0, st, a, which);
    hipLaunchKernelGGL(prog_scan_kernel, dim3(n), dim3(1024), 0, st, a, which, 0);
    hipLaunchKernelGGL(prog_block_kernel<2>, items_grid, dim3(256), 0, st, a, which);
    hipLaunchKernelGGL(prog_ff_count_kernel, chunk_grid, dim3(256), 0, st, a, which);
    hipLaunchKernelGGL(prog_scan_kernel, dim3(n), dim3(1024), 0, st, a, which, 1);
    hipLaunchKernelGGL(prog_stuff_kernel, chunk_grid, dim3(256), 0, st, a, which);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

}  // namespace ifhip
