// png_encode.hip -- gfx950 kernels + C ABI of the device PNG coder: BGRA / BGRX frames in HBM -> complete PNG files in HBM.
//
// Replaces what EncoderPreset::Libpng runs on the host (codecs/libpng_encoder.rs:43-72,134-160 ->
// c_components/lib/codec_png_wrapper.c:349-430): libpng's row filtering with its default adaptive choice, zlib's deflate
// and the chunk framing with its CRCs.  8-bit RGB or RGBA, non-interlaced, gAMA / sRGB / cHRM in front of one IDAT.
// Deflate is serial through three running values, and each is cut or turned into a prefix sum:
//   * the window: the filtered stream is fully known before the search starts, so a chunk of 32 KiB searches its own bytes
//     and the 32 KiB before them from LDS -- chunks are independent workgroups and still share the window;
//   * the greedy parse: 1024 positions search in parallel against the hash table as it stood before the round, the parse
//     over the round is resolved by pointer jumping, and the table takes the round's positions by atomic max;
//   * the bit position: a chunk is one deflate block closed to a byte boundary (an empty stored block, as a zlib sync
//     flush writes), so chunks meet at byte offsets: exact sizes from the histograms -> scan -> write.
// Launches per batch (all images in each): filter (a wave per row), match (a workgroup per chunk), codes (a wave per
// chunk: 316 symbols), layout (scan of the chunk sizes per image), emit (a workgroup per chunk), finish (framing and the
// IDAT CRC from the chunks' CRCs).  Every rule with a bit in it lives in png_encode_core.hpp, shared with the CPU
// emulation of the tests (tests/png_emulate.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "hip_entry.hpp"
#include "png_encode_args.hpp"
#include "png_encode_core.hpp"

namespace ifhip {

__device__ __forceinline__ uint32_t png_wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= static_cast<uint32_t>(d)) v += u;
    }
    return v;
}
// exclusive scan over the T lanes of a workgroup; *total = the sum.  `scratch`: T / 64 dwords.
template <uint32_t T>
__device__ __forceinline__ uint32_t png_block_scan(uint32_t v, uint32_t* scratch, uint32_t* total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t incl = png_wave_inclusive_scan(v, lane);
    __syncthreads();
    if (lane == 63u) scratch[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < T / 64u; ++w) {
        const uint32_t t = scratch[w];
        if (w < wave) before += t;
        sum += t;
    }
    *total = sum;
    return before + incl - v;
}
// XOR of v over the workgroup, valid in thread 0.  `scratch`: T / 64 dwords.
template <uint32_t T>
__device__ __forceinline__ uint32_t png_block_xor(uint32_t v, uint32_t* scratch) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v ^= __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (uint32_t w = 0; w < T / 64u; ++w) r ^= scratch[w];
    return r;
}
// Adler-32 of T pieces in order (ad / ln: checksum and length of every lane's piece, in LDS): a tree of combinations;
// the result is ad[0], ln[0]
template <uint32_t T>
__device__ __forceinline__ void png_block_adler(uint32_t* ad, uint32_t* ln) {
    const uint32_t tid = threadIdx.x;
    __syncthreads();
    for (uint32_t s = 1; s < T; s <<= 1) {
        if ((tid & (2u * s - 1u)) == 0u) {
            ad[tid] = png_adler_combine(ad[tid], ad[tid + s], ln[tid + s]);
            ln[tid] += ln[tid + s];
        }
        __syncthreads();
    }
}

// ---- filter: a wave per row ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_filter_kernel(const PngArgs a) {
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6), img = blockIdx.y;
    if (row >= a.h) return;                                  // (the whole wave)
    const uint8_t* frame = a.images + static_cast<size_t>(img) * a.image_bytes;
    const uint32_t* cur = reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(row) * a.stride);
    const uint32_t* prev = reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(row ? row - 1u : 0u) * a.stride);   // the row above comes from HBM / L2 again
    const bool top = row == 0u;
    uint32_t sums[5] = {0, 0, 0, 0, 0};
    for (uint32_t x = lane; x < a.w; x += 64u) {
        const uint32_t px = cur[x], pa = x ? cur[x - 1u] : 0u, pb = top ? 0u : prev[x], pc = (top || !x) ? 0u : prev[x - 1u];
        for (uint32_t ch = 0; ch < a.bpp; ++ch) {
            const uint32_t v = png_channel(px, ch), l = png_channel(pa, ch), u = png_channel(pb, ch), ul = png_channel(pc, ch);
#pragma unroll
            for (uint32_t f = 0; f < 5u; ++f) sums[f] += png_filter_cost(png_filter_byte(f, v, l, u, ul));
        }
    }
#pragma unroll
    for (uint32_t f = 0; f < 5u; ++f)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sums[f] += __shfl_xor(sums[f], d, 64);
    const uint32_t f = png_choose_filter(sums);
    uint8_t* out = a.streams + static_cast<size_t>(img) * a.stream_pitch + static_cast<size_t>(row) * a.pitch;
    if (lane == 0u) out[0] = static_cast<uint8_t>(f);
    for (uint32_t x = lane; x < a.w; x += 64u) {
        const uint32_t px = cur[x], pa = x ? cur[x - 1u] : 0u, pb = top ? 0u : prev[x], pc = (top || !x) ? 0u : prev[x - 1u];
        for (uint32_t ch = 0; ch < a.bpp; ++ch)
            out[1u + x * a.bpp + ch] = static_cast<uint8_t>(png_filter_byte(f, png_channel(px, ch), png_channel(pa, ch), png_channel(pb, ch), png_channel(pc, ch)));
    }
}

// ---- match: a workgroup per chunk ----------------------------------------------------------------------------------------------
struct MatchLds {
    uint32_t buf[(kPngWindow + kPngChunk) / 4u + 4u];        // the window and the chunk, 16 bytes to spare for png_load4
    union {
        uint32_t table[1u << kPngHashBits];                  // position + 1 of the latest 3 bytes with this hash, 0 = none
        struct { uint32_t ad[kPngRound], ln[kPngRound]; } sum;   // (the Adler-32 tree, before the table is in use)
    };
    uint32_t cnt[kPngSyms + 4u];
    uint16_t nxt[2][kPngRound];
    uint8_t mark[kPngRound];
    uint32_t scratch[kPngRound / 64u];
    uint32_t covered;
};
static_assert(sizeof(MatchLds) <= 112u * 1024u, "one workgroup per CU with room to spare (DESIGN 4.9)");

__global__ __launch_bounds__(kPngRound) void png_match_kernel(const PngArgs a) {
    __shared__ __attribute__((aligned(16))) MatchLds s;
    const uint32_t tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
    const uint32_t start = c * kPngChunk, n = min(kPngChunk, a.stream_bytes - start);
    const uint32_t win_start = start >= kPngWindow ? start - kPngWindow : 0u, woff = start - win_start, end = woff + n;
    const uint8_t* stream = a.streams + static_cast<size_t>(img) * a.stream_pitch;
    {   // (win_start is a multiple of 32 KiB and the streams are 16-byte aligned; the last quad may reach into the stream's spare 16 bytes)
        const uint4* src = reinterpret_cast<const uint4*>(stream + win_start);
        uint4* dst = reinterpret_cast<uint4*>(s.buf);
        const uint32_t quads = (end + 15u) >> 4;
        for (uint32_t i = tid; i < quads; i += kPngRound) dst[i] = src[i];
        if (tid == 0u) dst[quads] = make_uint4(0u, 0u, 0u, 0u);
    }
    for (uint32_t i = tid; i < kPngSyms + 4u; i += kPngRound) s.cnt[i] = 0u;
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(s.buf);
    {   // Adler-32 of the chunk: 32 bytes per lane, then the tree
        constexpr uint32_t per = kPngChunk / kPngRound;
        const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
        s.sum.ad[tid] = png_adler32(bytes + woff + lo, hi - lo);
        s.sum.ln[tid] = hi - lo;
        png_block_adler<kPngRound>(s.sum.ad, s.sum.ln);
        if (tid == 0u) *chunk_word(a, kAdler, img, c) = s.sum.ad[0];
        __syncthreads();
    }
    uint32_t ntok = 0;
    if (!a.stored_only) {
        for (uint32_t i = tid; i < (1u << kPngHashBits); i += kPngRound) s.table[i] = 0u;
        if (tid == 0u) s.covered = woff;
        __syncthreads();
        for (uint32_t lp = tid; lp < woff; lp += kPngRound)                       // the window's positions: the highest wins
            if (lp + 3u <= end) atomicMax(&s.table[png_hash3(png_load4(s.buf, lp))], lp + 1u);
        __syncthreads();
        uint32_t* tokens = a.tokens + chunk_index(a, img, c) * kPngChunk;
        for (uint32_t base = woff; base < end; base += kPngRound) {
            const uint32_t covered = s.covered, lp = base + tid;
            const bool valid = lp < end, hashed = lp + 3u <= end;
            const uint32_t h = hashed ? png_hash3(png_load4(s.buf, lp)) : 0u;
            uint32_t len = 1, dist = 0;
            if (valid && lp >= covered) {
                const uint32_t l = png_best_match(s.buf, lp, min(kPngMaxMatch, end - lp), a.bpp, a.pitch, hashed ? s.table[h] : 0u, &dist);
                if (l) len = l;
            }
            s.nxt[0][tid] = static_cast<uint16_t>(min(tid + len, kPngRound));
            s.mark[tid] = tid == covered - base ? 1 : 0;
            __syncthreads();                                                       // every lane has read the table as it stood before the round
            if (hashed) atomicMax(&s.table[h], lp + 1u);
            // The greedy parse over the round by pointer jumping: a marked lane marks the lane its token ends in front of,
            // and every lane's pointer doubles its reach.  Only lanes of the chain are ever marked, so a mark seen early is
            // still a right one; after ten steps the chain is marked through all 1024 lanes.
            uint32_t cur = 0;
            for (int it = 0; it < 10; ++it) {
                const uint32_t j = s.nxt[cur][tid];
                if (j < kPngRound) {
                    if (s.mark[tid]) s.mark[j] = 1;
                    s.nxt[cur ^ 1u][tid] = s.nxt[cur][j];
                } else {
                    s.nxt[cur ^ 1u][tid] = static_cast<uint16_t>(kPngRound);
                }
                __syncthreads();
                cur ^= 1u;
            }
            const bool emitted = valid && s.mark[tid];
            uint32_t total;
            const uint32_t ex = png_block_scan<kPngRound>(emitted ? 1u : 0u, s.scratch, &total);
            if (emitted) {
                if (len >= kPngMinMatch) {
                    uint32_t sym, eb, ev;
                    png_length_symbol(len, &sym, &eb, &ev); atomicAdd(&s.cnt[sym], 1u);
                    png_dist_symbol(dist, &sym, &eb, &ev); atomicAdd(&s.cnt[kPngLL + sym], 1u);
                    tokens[ntok + ex] = len << 16 | dist;
                } else {
                    const uint32_t b = bytes[lp];
                    atomicAdd(&s.cnt[b], 1u);
                    tokens[ntok + ex] = b;
                }
                atomicMax(&s.covered, lp + len);
            }
            ntok += total;
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0u) { s.cnt[256] = 1u; *chunk_word(a, kNtok, img, c) = ntok; }
    __syncthreads();
    uint32_t* counts = a.counts + chunk_index(a, img, c) * (kPngSyms + 4u);
    for (uint32_t i = tid; i < kPngSyms + 4u; i += kPngRound) counts[i] = s.cnt[i];
}

// ---- codes: a wave per chunk (316 symbols) -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void png_codes_kernel(const PngArgs a) {
    __shared__ PngCodeWork W;
    __shared__ uint32_t plan[2];
    const uint32_t lane = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
    const uint32_t* counts = a.counts + chunk_index(a, img, c) * (kPngSyms + 4u);
    for (uint32_t i = lane; i < kPngSyms + 4u; i += 64u) W.cnt[i] = counts[i];
    __syncthreads();
    png_rank_sort_lane(W.cnt, kPngLL, lane, 64u, W.sorted);
    __syncthreads();
    if (lane == 0u) {
        png_build_lengths(W, W.cnt, kPngLL, 15, W.len, 256, true);
        png_rank_sort_lane(W.cnt + kPngLL, kPngD, 0, 1, W.sorted);
        png_build_lengths(W, W.cnt + kPngLL, kPngD, 15, W.len + kPngLL, 0, false);
        const uint32_t n = min(kPngChunk, a.stream_bytes - c * kPngChunk);
        uint32_t type;
        plan[1] = png_plan_block(W, n, c + 1u == a.n_chunks, a.stored_only != 0u, &type);
        plan[0] = type;
    }
    __syncthreads();
    if (plan[0] != 0u) {
        uint32_t* tabs = a.tabs + chunk_index(a, img, c) * (kPngSyms + 4u);
        for (uint32_t i = lane; i < kPngSyms; i += 64u) tabs[i] = W.tab[i];
        uint32_t* prefix = a.prefix + chunk_index(a, img, c) * kPngPrefixWords;
        for (uint32_t i = lane; i < (W.prefix_bits + 31u) / 32u; i += 64u) prefix[i] = W.prefix[i];
    }
    if (lane == 0u) {
        *chunk_word(a, kType, img, c) = plan[0];
        *chunk_word(a, kPrefixBits, img, c) = W.prefix_bits;
        *chunk_word(a, kBytes, img, c) = plan[1];
    }
}

// ---- layout: the chunks' byte offsets, the stream's Adler-32 and the file's size, a workgroup per image -----------------------
__global__ __launch_bounds__(1024) void png_layout_kernel(const PngArgs a) {
    __shared__ uint32_t scratch[16];
    __shared__ uint32_t ad[1024], ln[1024];
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    uint32_t carry = 0, adler = 1;
    for (uint32_t base = 0; base < a.n_chunks; base += 1024u) {
        const uint32_t c = base + tid;
        const bool in = c < a.n_chunks;
        const uint32_t nb = in ? *chunk_word(a, kBytes, img, c) : 0u;
        uint32_t total;
        const uint32_t ex = png_block_scan<1024>(nb, scratch, &total);
        if (in) *chunk_word(a, kOffset, img, c) = carry + ex;
        carry += total;
        ad[tid] = in ? *chunk_word(a, kAdler, img, c) : 1u;
        ln[tid] = in ? min(kPngChunk, a.stream_bytes - c * kPngChunk) : 0u;
        png_block_adler<1024>(ad, ln);
        adler = png_adler_combine(adler, ad[0], ln[0]);
        __syncthreads();
    }
    if (tid == 0u) {
        a.image[img] = carry;
        a.image[a.n_images + img] = adler;
        a.image[2u * a.n_images + img] = static_cast<uint64_t>(kPngFraming) + 6u + carry > a.file_pitch ? 1u : 0u;
    }
}

// ---- emit: a workgroup per chunk -------------------------------------------------------------------------------------------------
constexpr uint32_t kEmitThreads = 512;
constexpr uint32_t kEmitWords = (kPngChunk + 8u) / 4u + 4u;

__global__ __launch_bounds__(kEmitThreads) void png_emit_kernel(const PngArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t out[kEmitWords];
    __shared__ uint32_t tab[kPngSyms + 4u];
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t scratch[kEmitThreads / 64u];
    const uint32_t tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
    if (a.image[2u * a.n_images + img]) return;              // (uniform: the file does not fit its pitch; nothing is written)
    const uint32_t type = *chunk_word(a, kType, img, c), nb = *chunk_word(a, kBytes, img, c);
    const uint32_t n = min(kPngChunk, a.stream_bytes - c * kPngChunk);
    const bool last = c + 1u == a.n_chunks;
    uint8_t* out8 = reinterpret_cast<uint8_t*>(out);
    if (tid < 256u) crc_tab[tid] = png_crc_step(0u, tid);
    if (nb > kPngChunk + 5u) return;                         // (cannot happen: stored is the floor)
    if (type == 0u) {
        const uint8_t* src = a.streams + static_cast<size_t>(img) * a.stream_pitch + static_cast<size_t>(c) * kPngChunk;
        if (tid == 0u) {
            out8[0] = last ? 1 : 0;
            out8[1] = static_cast<uint8_t>(n); out8[2] = static_cast<uint8_t>(n >> 8);
            out8[3] = static_cast<uint8_t>(~n); out8[4] = static_cast<uint8_t>(~n >> 8);
        }
        for (uint32_t i = tid; i < n; i += kEmitThreads) out8[5u + i] = src[i];
    } else {
        const uint32_t ntok = *chunk_word(a, kNtok, img, c), prefix_bits = *chunk_word(a, kPrefixBits, img, c);
        const uint32_t* tabs = a.tabs + chunk_index(a, img, c) * (kPngSyms + 4u);
        const uint32_t* prefix = a.prefix + chunk_index(a, img, c) * kPngPrefixWords;
        const uint32_t* tokens = a.tokens + chunk_index(a, img, c) * kPngChunk;
        const uint32_t pw = (prefix_bits + 31u) / 32u;
        for (uint32_t i = tid; i < kEmitWords; i += kEmitThreads) out[i] = i < pw ? prefix[i] : 0u;
        for (uint32_t i = tid; i < kPngSyms; i += kEmitThreads) tab[i] = tabs[i];
        __syncthreads();
        auto or_word = [](uint32_t* p, uint32_t v) { atomicOr(p, v); };
        uint32_t pos = prefix_bits;
        for (uint32_t base = 0; base <= ntok; base += kEmitThreads) {
            const uint32_t i = base + tid;
            uint32_t bits = 0;
            uint64_t val = 0;
            if (i < ntok) bits = png_token_bits(tab, tokens[i], &val);
            else if (i == ntok) { val = tab[256] & 0xFFFFu; bits = tab[256] >> 16; }
            uint32_t total;
            const uint32_t at = pos + png_block_scan<kEmitThreads>(bits, scratch, &total);
            if (bits && (at >> 5) + 3u <= kEmitWords) png_or_bits(out, at, val, or_word);
            pos += total;
        }
        __syncthreads();
        if (!last && tid == 0u) { out8[nb - 2u] = 0xFF; out8[nb - 1u] = 0xFF; }   // the empty stored block's NLEN; its other bits are zero
    }
    __syncthreads();
    // the chunk's CRC-32: a slice per lane, every piece shifted behind the bytes that follow it, the pieces meet by XOR
    const uint32_t per = (nb + kEmitThreads - 1u) / kEmitThreads, lo = min(nb, tid * per), hi = min(nb, lo + per);
    uint32_t crc = 0;
    if (hi > lo) {
        uint32_t r = 0xFFFFFFFFu;
        for (uint32_t i = lo; i < hi; ++i) r = crc_tab[(r ^ out8[i]) & 255u] ^ (r >> 8);
        crc = png_crc_shift(~r, nb - hi);
    }
    crc = png_block_xor<kEmitThreads>(crc, scratch);
    if (tid == 0u) *chunk_word(a, kCrc, img, c) = crc;
    uint8_t* dst = a.files + static_cast<size_t>(img) * a.file_pitch + kPngHeadBytes + 8u + 2u + *chunk_word(a, kOffset, img, c);
    for (uint32_t i = tid; i < nb; i += kEmitThreads) dst[i] = out8[i];
}

// ---- finish: the framing and the IDAT chunk's CRC, a workgroup per image -----------------------------------------------------
__global__ __launch_bounds__(1024) void png_finish_kernel(const PngArgs a) {
    __shared__ uint32_t scratch[16];
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    const uint32_t body = a.image[img], adler = a.image[a.n_images + img];
    if (a.image[2u * a.n_images + img]) {
        if (tid == 0u) { a.lengths[img] = 0u; if (a.status_out) a.status_out[img] = kPngFileOverflow; }
        return;
    }
    const uint32_t zlen = 2u + body + 4u;
    uint8_t* file = a.files + static_cast<size_t>(img) * a.file_pitch;
    uint8_t* idat = file + kPngHeadBytes;
    uint32_t crc = 0;
    for (uint32_t c = tid; c < a.n_chunks; c += 1024u)
        crc ^= png_crc_shift(*chunk_word(a, kCrc, img, c), static_cast<uint64_t>(body) - *chunk_word(a, kOffset, img, c) - *chunk_word(a, kBytes, img, c) + 4u);
    if (tid == 1023u) {                                      // the chunk type and the zlib header in front, the Adler-32 behind
        png_be32(idat, zlen);
        png_be32(idat + 4, kPngIDAT);
        idat[8] = static_cast<uint8_t>(a.zlib_header >> 8); idat[9] = static_cast<uint8_t>(a.zlib_header);
        png_be32(idat + 10u + body, adler);
        crc ^= png_crc_shift(png_crc32(idat + 4, 6), static_cast<uint64_t>(body) + 4u) ^ png_crc32(idat + 10u + body, 4);
    }
    crc = png_block_xor<1024>(crc, scratch);
    if (tid == 0u) {
        png_write_head(file, a.w, a.h, a.color_type);
        png_be32(idat + 8u + zlen, crc);
        png_close_chunk(idat + 12u + zlen, kPngIEND, 0);
        a.lengths[img] = kPngFraming + zlen;
        if (a.status_out) a.status_out[img] = 0u;
    }
}

void png_launch_deflate(const PngArgs& a, hipStream_t st) {
    const dim3 chunk_grid(a.n_chunks, a.n_images);
    hipLaunchKernelGGL(png_match_kernel, chunk_grid, dim3(kPngRound), 0, st, a);
    hipLaunchKernelGGL(png_codes_kernel, chunk_grid, dim3(64), 0, st, a);
    hipLaunchKernelGGL(png_layout_kernel, dim3(a.n_images), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(png_emit_kernel, chunk_grid, dim3(kEmitThreads), 0, st, a);
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_png_enc_stage {
    uint32_t width = 0, height = 0, bpp = 0, color_type = 0, max_images = 0;
    uint32_t pitch = 0, stream_bytes = 0, n_chunks = 0;
    size_t stream_pitch = 0;
    int device = -1;                    // -1: the scratch is not allocated yet (the first batch does it, behind the argument checks)
    uint8_t* d_streams = nullptr;
    uint32_t *d_tokens = nullptr, *d_counts = nullptr, *d_tabs = nullptr, *d_prefix = nullptr, *d_chunk = nullptr, *d_image = nullptr;
    ~ifhip_png_enc_stage() {
        (void)DEV_FREE(d_streams); (void)DEV_FREE(d_tokens); (void)DEV_FREE(d_counts); (void)DEV_FREE(d_tabs); (void)DEV_FREE(d_prefix);
        (void)DEV_FREE(d_chunk); (void)DEV_FREE(d_image);
    }
};

namespace {
int png_stage_allocate(ifhip_png_enc_stage* s) {
    int dev = -1;
    if (int rc = require_gfx950(&dev)) return rc;
    if (s->device >= 0) {
        if (dev != s->device) return fail(IFHIP_INVALID_STATE, "InvalidState: stage belongs to device %d, current device is %d", s->device, dev);
        return IFHIP_OK;
    }
    const size_t n = s->max_images, chunks = n * s->n_chunks;
    HIP_TRY(DEV_MALLOC(&s->d_streams, n * s->stream_pitch));
    HIP_TRY(DEV_MALLOC(&s->d_tokens, chunks * kPngChunk * sizeof(uint32_t)));
    HIP_TRY(DEV_MALLOC(&s->d_counts, chunks * (kPngSyms + 4u) * sizeof(uint32_t)));
    HIP_TRY(DEV_MALLOC(&s->d_tabs, chunks * (kPngSyms + 4u) * sizeof(uint32_t)));
    HIP_TRY(DEV_MALLOC(&s->d_prefix, chunks * kPngPrefixWords * sizeof(uint32_t)));
    HIP_TRY(DEV_MALLOC(&s->d_chunk, chunks * kChunkWords * sizeof(uint32_t)));
    HIP_TRY(DEV_MALLOC(&s->d_image, n * 3u * sizeof(uint32_t)));
    s->device = dev;
    return IFHIP_OK;
}
}  // namespace

extern "C" {

int ifhip_png_enc_stage_create(ifhip_png_enc_stage** stage, uint32_t width, uint32_t height, int color_type, uint32_t max_images) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage out-pointer");
    *stage = nullptr;
    if (color_type != IFHIP_PNG_RGB && color_type != IFHIP_PNG_RGBA) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: color_type is 2 (RGB) or 6 (RGBA)");
    if (width == 0 || height == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (max_images == 0 || max_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 images per stage");
    const uint32_t bpp = color_type == IFHIP_PNG_RGB ? 3u : 4u;
    const uint64_t pitch = 1ull + static_cast<uint64_t>(width) * bpp, bytes = pitch * height;
    if (bytes > 0x7FFF0000ull) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a filtered image of %llu bytes (one IDAT chunk holds 2^31 - 1)", static_cast<unsigned long long>(bytes));
    std::unique_ptr<ifhip_png_enc_stage> s(new ifhip_png_enc_stage);
    s->width = width; s->height = height; s->bpp = bpp; s->color_type = static_cast<uint32_t>(color_type); s->max_images = max_images;
    s->pitch = static_cast<uint32_t>(pitch);
    s->stream_bytes = static_cast<uint32_t>(bytes);
    s->n_chunks = (s->stream_bytes + kPngChunk - 1u) / kPngChunk;
    s->stream_pitch = ((static_cast<size_t>(bytes) + 15u) & ~static_cast<size_t>(15u)) + 16u;
    *stage = s.release();
    return IFHIP_OK;
}

void ifhip_png_enc_stage_destroy(ifhip_png_enc_stage* stage) { delete stage; }

size_t ifhip_png_enc_stage_max_file_bytes(const ifhip_png_enc_stage* stage) {
    // every chunk stored (its bytes + 5), the zlib header and Adler-32, the framing
    return stage ? static_cast<size_t>(stage->stream_bytes) + 5u * stage->n_chunks + 6u + kPngFraming : 0u;
}

int ifhip_png_encode_batch_device(ifhip_png_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, uint32_t n_images,
                                  int zlib_level, uint8_t* d_files, size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status, void* hip_stream) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage");
    if (n_images == 0) return IFHIP_OK;
    if (n_images > stage->max_images) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: %u images exceed the stage capacity %u", n_images, stage->max_images);
    if (int rc = check_frames(d_images, image_bytes, stage->width, stage->height, stride, "image")) return rc;
    if (!d_files || !d_lengths) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    if (zlib_level < -1 || zlib_level > 9) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: zlib_level is -1 or 0..9");
    if (file_pitch < kPngFraming + 6u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: file_pitch below %u bytes", kPngFraming + 6u);
    if (int rc = png_stage_allocate(stage)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    PngArgs a;
    std::memset(&a, 0, sizeof a);
    a.images = d_images; a.image_bytes = image_bytes; a.stride = stride; a.w = stage->width; a.h = stage->height; a.bpp = stage->bpp;
    a.pitch = stage->pitch; a.color_type = stage->color_type; a.stream_bytes = stage->stream_bytes; a.n_chunks = stage->n_chunks;
    a.stream_pitch = stage->stream_pitch; a.streams = stage->d_streams; a.tokens = stage->d_tokens; a.counts = stage->d_counts;
    a.tabs = stage->d_tabs; a.prefix = stage->d_prefix; a.chunk = stage->d_chunk; a.image = stage->d_image;
    a.n_images = n_images; a.stored_only = zlib_level == 0 ? 1u : 0u; a.zlib_header = png_zlib_header(zlib_level);
    a.files = d_files; a.file_pitch = file_pitch; a.lengths = d_lengths; a.status_out = d_status;
    hipLaunchKernelGGL(png_filter_kernel, dim3((stage->height + 3u) / 4u, n_images), dim3(256), 0, st, a);
    png_launch_deflate(a, st);
    hipLaunchKernelGGL(png_finish_kernel, dim3(n_images), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_png_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int color_type, int zlib_level, uint8_t* out,
                     size_t capacity, size_t* len) {
    if (!len) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null length out-pointer");
    *len = 0;
    ifhip_png_enc_stage* stage = nullptr;
    if (int rc = ifhip_png_enc_stage_create(&stage, width, height, color_type, 1)) return rc;
    std::unique_ptr<ifhip_png_enc_stage, void (*)(ifhip_png_enc_stage*)> guard(stage, [](ifhip_png_enc_stage* s) { (void)hipStreamSynchronize(nullptr); ifhip_png_enc_stage_destroy(s); });
    const size_t pitch = (ifhip_png_enc_stage_max_file_bytes(stage) + 15u) & ~static_cast<size_t>(15u);
    HostFrame f;
    if (int rc = f.up(bgra, width, height, stride, pitch + 16u)) return rc;
    uint8_t* d_file = f.side_output();
    uint32_t* d_len = reinterpret_cast<uint32_t*>(d_file + pitch);
    if (int rc = ifhip_png_encode_batch_device(stage, f.d, f.image_bytes, stride, 1, zlib_level, d_file, pitch, d_len, d_len + 1, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    uint32_t len_status[2] = {0, 0};
    HIP_TRY(hipMemcpy(len_status, d_len, 8, hipMemcpyDeviceToHost));
    if (len_status[1] || !len_status[0]) return fail(IFHIP_INVALID_STATE, "InvalidState: the file did not fit its worst-case size (status %u)", len_status[1]);
    *len = len_status[0];
    if (!out) return IFHIP_OK;
    if (capacity < *len) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: the file needs %zu bytes, the buffer has %zu", *len, capacity);
    HIP_TRY(hipMemcpy(out, d_file, *len, hipMemcpyDeviceToHost));
    return IFHIP_OK;
}

}  // extern "C"
