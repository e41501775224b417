// png_deflate.hip -- the deflate back end of the device PNG coders: the filtered streams of a batch in HBM -> a zlib body
// per image in HBM, with its Adler-32 and the CRC-32 of every chunk of it (png_deflate.hpp).  Deflate is serial through three running values, and each is cut or turned into a prefix sum:
//   * the window: the filtered stream is fully known before the search starts, so a chunk of 32 KiB searches its own bytes
//     and the 32 KiB before them from LDS -- chunks are independent workgroups and still share the window;
//   * the greedy parse: 1024 positions search in parallel against the hash table as it stood before the round, the parse
//     over the round is resolved by pointer jumping, and the table takes the round's positions by atomic max;
//   * the bit position: a chunk is one deflate block closed to a byte boundary (an empty stored block, as a zlib sync
//     flush writes), so chunks meet at byte offsets: exact sizes from the histograms -> scan -> write.
// Launches per batch (all images in each): match (a workgroup per chunk), codes (a wave per chunk: 316 symbols), layout
// (scan of the chunk sizes per image), emit (a workgroup per chunk).  Every rule with a bit in it lives in png_encode_core.hpp
// and, where every prefix code shares it, prefix_code_core.hpp; the CPU emulation of the tests compiles both (tests/png_emulate.cpp).
#include <hip/hip_runtime.h>

#include "block_scan.hpp"
#include "hip_entry.hpp"
#include "png_frame_device.hpp"      // (with png_deflate.hpp and png_encode_core.hpp)

namespace ifhip {

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

__global__ __launch_bounds__(kPngRound) void png_match_kernel(const PngDeflateArgs a) {
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
            const uint32_t ex = block_exclusive_scan<kPngRound>(emitted ? 1u : 0u, s.scratch, &total);
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
__global__ __launch_bounds__(64) void png_codes_kernel(const PngDeflateArgs a) {
    __shared__ PngCodeWork W;
    __shared__ uint32_t plan[2];
    const uint32_t lane = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
    const uint32_t* counts = a.counts + chunk_index(a, img, c) * (kPngSyms + 4u);
    for (uint32_t i = lane; i < kPngSyms + 4u; i += 64u) W.cnt[i] = counts[i];
    __syncthreads();
    code_rank_sort_lane(W.cnt, kPngLL, lane, 64u, W.sorted);
    __syncthreads();
    if (lane == 0u) {
        code_build_lengths(W, W.cnt, kPngLL, 15, W.len, 256, true);
        code_rank_sort_lane(W.cnt + kPngLL, kPngD, 0, 1, W.sorted);
        code_build_lengths(W, W.cnt + kPngLL, kPngD, 15, W.len + kPngLL, 0, false);
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

// ---- layout: the chunks' byte offsets, the stream's Adler-32 and the body's size, a workgroup per image -----------------------
__global__ __launch_bounds__(1024) void png_layout_kernel(const PngDeflateArgs a) {
    __shared__ uint32_t scratch[16];
    __shared__ uint32_t ad[1024], ln[1024];
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    uint32_t carry = 0, adler = 1;
    for (uint32_t base = 0; base < a.n_chunks; base += 1024u) {
        const uint32_t c = base + tid;
        const bool in = c < a.n_chunks;
        const uint32_t nb = in ? *chunk_word(a, kBytes, img, c) : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<1024>(nb, scratch, &total);
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
        a.image[2u * a.n_images + img] = carry > a.body_cap ? 1u : 0u;
    }
}

// ---- emit: a workgroup per chunk -------------------------------------------------------------------------------------------------
constexpr uint32_t kEmitThreads = 512;
constexpr uint32_t kEmitWords = (kPngChunk + 8u) / 4u + 4u;

__global__ __launch_bounds__(kEmitThreads) void png_emit_kernel(const PngDeflateArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t out[kEmitWords];
    __shared__ uint32_t tab[kPngSyms + 4u];
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t scratch[kEmitThreads / 64u];
    const uint32_t tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
    if (a.image[2u * a.n_images + img]) return;              // (uniform: the body does not fit its place; nothing is written)
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
            const uint32_t at = pos + block_exclusive_scan<kEmitThreads>(bits, scratch, &total);
            if (bits && (at >> 5) + 3u <= kEmitWords) or_bits(out, at, val, or_word);
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
    uint8_t* dst = a.body + static_cast<size_t>(img) * a.body_pitch + *chunk_word(a, kOffset, img, c);
    for (uint32_t i = tid; i < nb; i += kEmitThreads) dst[i] = out8[i];
}

void png_launch_deflate(const PngDeflateArgs& a, hipStream_t st) {
    const dim3 chunk_grid(a.n_chunks, a.n_images);
    hipLaunchKernelGGL(png_match_kernel, chunk_grid, dim3(kPngRound), 0, st, a);
    hipLaunchKernelGGL(png_codes_kernel, chunk_grid, dim3(64), 0, st, a);
    hipLaunchKernelGGL(png_layout_kernel, dim3(a.n_images), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(png_emit_kernel, chunk_grid, dim3(kEmitThreads), 0, st, a);
}

// ---- the scratch ----------------------------------------------------------------------------------------------------------------
void PngDeflateScratch::shape(uint32_t width, uint32_t bytes_per_pixel, uint32_t height) {
    bpp = bytes_per_pixel;
    pitch = png_stream_pitch(width, bpp);
    stream_bytes = static_cast<uint32_t>(static_cast<uint64_t>(pitch) * height);
    n_chunks = (stream_bytes + kPngChunk - 1u) / kPngChunk;
    stream_pitch = ((static_cast<size_t>(stream_bytes) + 15u) & ~static_cast<size_t>(15u)) + 16u;
}
int PngDeflateScratch::allocate(uint32_t max_images) {
    const size_t n = max_images, chunks = n * n_chunks;
    return blocks.ensure([&]() -> int {
        HIP_TRY(DEV_MALLOC(&d_streams, n * stream_pitch));
        HIP_TRY(DEV_MALLOC(&d_tokens, chunks * kPngChunk * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&d_counts, chunks * (kPngSyms + 4u) * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&d_tabs, chunks * (kPngSyms + 4u) * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&d_prefix, chunks * kPngPrefixWords * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&d_chunk, chunks * kChunkWords * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&d_image, n * 3u * sizeof(uint32_t)));
        return IFHIP_OK;
    });
}
PngDeflateArgs PngDeflateScratch::args(uint32_t n_images, int zlib_level, uint8_t* body, size_t body_pitch, uint32_t body_cap) const {
    return PngDeflateArgs{d_streams, stream_pitch, stream_bytes, pitch, bpp, n_chunks, n_images, zlib_level == 0 ? 1u : 0u,
                          d_tokens, d_counts, d_tabs, d_prefix, d_chunk, d_image, body, body_pitch, body_cap};
}

}  // namespace ifhip
