// webp_encode.hip -- gfx950 kernels + C ABI of the device lossless-WebP coder: BGRA / BGRX frames in HBM -> complete
// WebP (VP8L) files in HBM.
//
// Replaces what EncoderPreset::WebPLossless runs on the host (codecs/webp.rs:281-345, codecs/auto.rs:282-319:
// WebPEncodeLosslessBGRA / WebPEncodeLosslessBGR of libwebp).  A lossless coder is free in its choices as long as the
// pixels come back: the contract is exact pixels through libwebp's decoder, not libwebp's bytes.
// Launches per batch (all images in each):
//   residual  a workgroup per 16 x 16 tile: subtract green, the 14 predictor modes on the original neighbours, the mode
//             with the smallest sum of |residual bytes|, the residual pixels
//   parse     a workgroup per segment of 4096 pixels (segments do not cross the 64-row bands): runs of equal residual
//             pixels at the distances 1 and width, the greedy parse by pointer jumping, tokens and the counts of the five
//             alphabets; whether the segment is one residual pixel throughout
//   codes     a workgroup per band: the band's counts (the sum of its segments'), its five prefix codes with their
//             headers, the exact bits of each of its segments.  A band of one residual pixel throughout is coded as
//             literals instead: five one-symbol codes, no bits for its pixels
//   layout    a workgroup per image: the codes of the mode and entropy sub-images, one running sum over head, group
//             headers and segments, the overflow check, and the head's bits
//   emit      a workgroup per segment (bits into an LDS window, shifted by the segment's bit offset; the one word two
//             neighbours share is ORed atomically into the zeroed file) and per group header
//   finish    RIFF framing, lengths, status
// Every rule with a bit in it lives in webp_encode_core.hpp (VP8L's own) and prefix_code_core.hpp (what every prefix
// code shares), both compiled into the CPU emulation of the tests as well (tests/webp_emulate.cpp).  Everything reduced across lanes is an integer sum or an OR: the same pixels give the same
// bytes on every run and in every batch position.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "block_scan.hpp"
#include "encode_handoff.hpp"
#include "stage_scratch.hpp"
#include "webp_encode_core.hpp"

namespace ifhip {

struct WebpArgs {
    const uint8_t* images;
    size_t image_bytes;
    uint32_t stride, alpha_or, n_images;
    WebpShape S;
    size_t px_pitch;                    // dwords between two images' residuals / tokens
    uint32_t *resid, *tok;              // [n_images][px_pitch]
    uint8_t* modes;                     // [n_images][tiles_y * tiles_x]
    uint32_t *seg_hist, *seg_bits;      // [n_images][n_segs][kWebpSyms], [n_images][n_segs]
    uint32_t* seg_flat;                 // [n_images][n_segs][2]: all of the segment's residual pixels are equal; the pixel
    uint64_t *seg_off, *grp_off;        // [n_images][n_segs], [n_images][n_bands]: bit offsets in the payload
    uint32_t *grp_tab, *grp_hdr, *grp_hbits;   // [n_images][n_bands][kWebpSyms | kWebpGroupWords | 1]
    uint32_t* grp_literal;              // [n_images][n_bands]: the band is written as literals (its tokens are set aside)
    uint32_t flat_group_bits;           // webp_flat_group_bits(): the headers of a band written as literals under flat codes
    uint32_t* image;                    // [n_images][4]: overflow, payload bytes, the tail dword (zeroed per batch), unused
    uint8_t* files;
    size_t file_pitch;
    uint32_t *lengths, *status_out;
};

// The payload of image img as a dword stream: the file need not start on a dword, so the stream starts at the dword
// that holds the payload's first byte and *origin is the payload's first bit in it.
__device__ __forceinline__ uint32_t* webp_payload_words(const WebpArgs& a, uint32_t img, uint32_t* origin) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a.files) + static_cast<size_t>(img) * a.file_pitch + kWebpRiff;
    *origin = static_cast<uint32_t>(p & 3u) * 8u;
    return reinterpret_cast<uint32_t*>(p & ~static_cast<uintptr_t>(3));
}
// How a dword of the file is ORed.  A file_pitch that is no multiple of 4 leaves the image's last bytes in a dword that
// reaches past its pitch -- for the last image past the caller's buffer.  That dword (`tail`) is never touched: its bits
// are gathered in the image's spare word and webp_finish_kernel stores the bytes that belong to the image one by one.
struct GlobalOr {
    uint32_t *tail, *spare;
    __device__ void operator()(uint32_t* p, uint32_t v) const { atomicOr(p == tail ? spare : p, v); }
};
__device__ __forceinline__ GlobalOr webp_global_or(const WebpArgs& a, uint32_t img) {
    const uintptr_t end = reinterpret_cast<uintptr_t>(a.files) + static_cast<size_t>(img + 1u) * a.file_pitch;
    return GlobalOr{(end & 3u) ? reinterpret_cast<uint32_t*>(end & ~static_cast<uintptr_t>(3)) : nullptr, a.image + 4u * img + 2u};
}

// ---- residual: a workgroup per tile, a lane per pixel ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void webp_residual_kernel(const WebpArgs a) {
    __shared__ uint32_t sums[4][14];
    __shared__ uint32_t chosen;
    const uint32_t tid = threadIdx.x, img = blockIdx.z;
    const uint32_t x = blockIdx.x * kWebpTile + (tid & 15u), y = blockIdx.y * kWebpTile + (tid >> 4);
    const bool inside = x < a.S.w && y < a.S.h;
    const uint8_t* frame = a.images + static_cast<size_t>(img) * a.image_bytes;
    uint32_t px = 0;
    WebpNeighbours nb = {0, 0, 0, 0};
    if (inside) { px = webp_source(frame, a.stride, x, y, a.alpha_or); nb = webp_neighbours(frame, a.stride, a.S.w, x, y, a.alpha_or); }
#pragma unroll
    for (uint32_t m = 0; m < 14u; ++m) {
        uint32_t c = inside ? webp_residual_cost(webp_sub_pixels(px, webp_predict_at(m, x, y, nb))) : 0u;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
        if ((tid & 63u) == 0u) sums[tid >> 6][m] = c;
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t best = 0, least = 0xFFFFFFFFu;
        for (uint32_t m = 0; m < 14u; ++m) {                  // the smallest sum; a tie goes to the lowest number
            const uint32_t s = sums[0][m] + sums[1][m] + sums[2][m] + sums[3][m];
            if (s < least) { least = s; best = m; }
        }
        chosen = best;
        a.modes[static_cast<size_t>(img) * a.S.tiles_x * a.S.tiles_y + blockIdx.y * a.S.tiles_x + blockIdx.x] = static_cast<uint8_t>(best);
    }
    __syncthreads();
    if (inside) a.resid[static_cast<size_t>(img) * a.px_pitch + static_cast<size_t>(y) * a.S.w + x] = webp_sub_pixels(px, webp_predict_at(chosen, x, y, nb));
}

// ---- parse: a workgroup per segment ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void webp_parse_kernel(const WebpArgs a) {
    __shared__ uint32_t r[kWebpSeg];
    __shared__ uint16_t len16[kWebpSeg], nxt[2][kWebpSeg];
    __shared__ uint8_t sel[kWebpSeg], mark[kWebpSeg];
    __shared__ uint16_t suf[2][2][1024 + 1];                   // [distance][buffer]: the first break at or behind a lane's positions
    __shared__ uint32_t hist[kWebpSyms];
    const uint32_t tid = threadIdx.x, seg = blockIdx.x, img = blockIdx.y;
    uint32_t start;
    const uint32_t n = webp_segment(a.S, seg, &start);
    uint32_t* out_hist = a.seg_hist + (static_cast<size_t>(img) * a.S.n_segs + seg) * kWebpSyms;
    for (uint32_t s = tid; s < kWebpSyms; s += 1024u) hist[s] = 0;
    if (n == 0u) {                                             // (the whole workgroup) an empty segment of the last band counts nothing
        for (uint32_t s = tid; s < kWebpSyms; s += 1024u) out_hist[s] = 0;
        return;
    }
    const uint32_t* resid = a.resid + static_cast<size_t>(img) * a.px_pitch;
    uint32_t* tok = a.tok + static_cast<size_t>(img) * a.px_pitch;
    const uint32_t w = a.S.w;
    for (uint32_t i = tid; i < kWebpSeg; i += 1024u) r[i] = i < n ? resid[start + i] : 0u;
    __syncthreads();
    {
        bool same = true;
        for (uint32_t i = tid; i < n; i += 1024u) same = same && r[i] == r[0];
        const int flat = __syncthreads_and(same ? 1 : 0);
        if (tid == 0u) {
            uint32_t* f = a.seg_flat + (static_cast<size_t>(img) * a.S.n_segs + seg) * 2u;
            f[0] = flat ? 1u : 0u; f[1] = r[0];
        }
    }
    // where the runs of equal pixels break: per lane over its four positions, then a suffix minimum over the lanes
    uint32_t brk1[4], brkw[4];
    {
        uint32_t first1 = 0xFFFFu, firstw = 0xFFFFu;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            const uint32_t i = 4u * tid + static_cast<uint32_t>(k), g = start + i;
            bool e1 = false, ew = false;
            if (i < n) {
                e1 = g >= 1u && r[i] == (i >= 1u ? r[i - 1u] : resid[g - 1u]);
                ew = g >= w && r[i] == (i >= w ? r[i - w] : resid[g - w]);
            }
            if (!e1) first1 = i;
            if (!ew) firstw = i;
            brk1[k] = first1; brkw[k] = firstw;                // the first break at or behind position k among the lane's own
        }
        suf[0][0][tid] = static_cast<uint16_t>(first1); suf[1][0][tid] = static_cast<uint16_t>(firstw);
    }
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t o = tid + d;
        uint32_t v1 = suf[0][cur][tid], vw = suf[1][cur][tid];
        if (o < 1024u) { v1 = min(v1, static_cast<uint32_t>(suf[0][cur][o])); vw = min(vw, static_cast<uint32_t>(suf[1][cur][o])); }
        suf[0][cur ^ 1u][tid] = static_cast<uint16_t>(v1); suf[1][cur ^ 1u][tid] = static_cast<uint16_t>(vw);
        cur ^= 1u;
        __syncthreads();
    }
    {
        const uint32_t behind1 = tid + 1u < 1024u ? suf[0][cur][tid + 1u] : 0xFFFFu, behindw = tid + 1u < 1024u ? suf[1][cur][tid + 1u] : 0xFFFFu;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t i = 4u * tid + k;
            uint32_t t = 1u;
            if (i < n) {
                const uint32_t b1 = min(min(brk1[k], behind1), n), bw = min(min(brkw[k], behindw), n);
                t = webp_choose_match(b1 - i, bw - i, n - i);
            }
            len16[i] = static_cast<uint16_t>(t & 0xFFFFu); sel[i] = static_cast<uint8_t>(t >> 16);
            nxt[0][i] = static_cast<uint16_t>(min(i + (t & 0xFFFFu), kWebpSeg));
            mark[i] = i == 0u ? 1 : 0;
        }
    }
    __syncthreads();
    // the greedy parse: the positions the chain from 0 visits.  Pointers double their reach every step; a mark is only ever
    // set, and only on a position of the chain, so the order of the lanes does not show.
    cur = 0;
    for (uint32_t step = 0; step < 12u; ++step) {
        for (uint32_t i = tid; i < kWebpSeg; i += 1024u) {
            const uint32_t j = nxt[cur][i];
            if (j < kWebpSeg) { if (mark[i]) mark[j] = 1; nxt[cur ^ 1u][i] = nxt[cur][j]; } else nxt[cur ^ 1u][i] = static_cast<uint16_t>(kWebpSeg);
        }
        cur ^= 1u;
        __syncthreads();
    }
    for (uint32_t i = tid; i < n; i += 1024u) {
        uint32_t t = 0;
        if (mark[i]) {
            t = len16[i] | (static_cast<uint32_t>(sel[i]) << 16);
            const WebpTokenSymbols sy = webp_count_token(t, r[i]);
            atomicAdd(&hist[sy.s0], 1u); atomicAdd(&hist[sy.s1], 1u);
            if (sy.n == 4u) { atomicAdd(&hist[sy.s2], 1u); atomicAdd(&hist[sy.s3], 1u); }
        }
        tok[start + i] = t;
    }
    __syncthreads();
    for (uint32_t s = tid; s < kWebpSyms; s += 1024u) out_hist[s] = hist[s];
}

// the five codes of the counts in cnt (LDS), by the whole workgroup: the rank sort by all lanes, the construction by lane 0
__device__ __forceinline__ void webp_build_codes(WebpCodeWork& W, const uint32_t* cnt, uint32_t* tab, uint32_t* hdr, uint32_t* pos, bool force_flat) {
    for (uint32_t al = 0; al < 5u; ++al) {
        const uint32_t off = webp_alphabet_offset(al);
        code_rank_sort_lane(cnt + off, webp_alphabet_size(al), threadIdx.x, blockDim.x, W.P.sorted);
        __syncthreads();
        if (threadIdx.x == 0u) { uint32_t fixed; webp_build_code(W, cnt + off, al, tab + off, hdr, pos, &fixed, force_flat); }
        __syncthreads();
    }
}

// ---- codes: a workgroup per band -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void webp_codes_kernel(const WebpArgs a) {
    __shared__ WebpCodeWork W;
    __shared__ uint32_t cnt[kWebpSyms], tab[kWebpSyms], hdr[kWebpGroupWords];
    __shared__ uint32_t pos, acc, own, constant, constant_px, constant_value, seg_own[256];
    const uint32_t tid = threadIdx.x, band = blockIdx.x, img = blockIdx.y;
    const size_t seg0 = static_cast<size_t>(img) * a.S.n_segs + static_cast<size_t>(band) * a.S.segs_per_band;
    for (uint32_t s = tid; s < kWebpSyms; s += 256u) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < a.S.segs_per_band; ++j) c += a.seg_hist[(seg0 + j) * kWebpSyms + s];
        cnt[s] = c;
    }
    for (uint32_t i = tid; i < kWebpGroupWords; i += 256u) hdr[i] = 0;
    if (tid == 0u) {
        pos = 0; acc = 0; own = 0;
        uint32_t flat = 1u, px = 0;                              // (at most 256 segments)
        const uint32_t value = a.seg_flat[seg0 * 2u + 1u];
        for (uint32_t j = 0; j < a.S.segs_per_band; ++j) {
            uint32_t start;
            const uint32_t n = webp_segment(a.S, band * a.S.segs_per_band + j, &start);
            if (n && (!a.seg_flat[(seg0 + j) * 2u] || a.seg_flat[(seg0 + j) * 2u + 1u] != value)) flat = 0u;
            px += n;
        }
        constant = flat; constant_px = px; constant_value = value;
    }
    __syncthreads();
    if (constant) {                                            // (the whole workgroup) literals of one pixel: no match symbols
        for (uint32_t s = tid; s < kWebpSyms; s += 256u) cnt[s] = 0;
        __syncthreads();
        if (tid == 0u) {
            const WebpTokenSymbols sy = webp_count_token(1u, constant_value);
            cnt[sy.s0] = constant_px; cnt[sy.s1] = constant_px; cnt[sy.s2] = constant_px; cnt[sy.s3] = constant_px;
        }
        __syncthreads();
    }
    webp_build_codes(W, cnt, tab, hdr, &pos, false);
    for (uint32_t j = 0; j < a.S.segs_per_band; ++j) {         // histogram . (lengths + extra bits): no count pass over the tokens
        uint32_t bits = 0;
        for (uint32_t s = tid; s < kWebpSyms; s += 256u) bits += a.seg_hist[(seg0 + j) * kWebpSyms + s] * webp_symbol_cost(tab, s);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) bits += __shfl_xor(bits, d, 64);
        if ((tid & 63u) == 0u) atomicAdd(&acc, bits);
        __syncthreads();
        if (tid == 0u) { seg_own[j] = constant ? 0u : acc; own += seg_own[j]; acc = 0; }
        __syncthreads();
    }
    // the band as literals under four flat codes, when that is smaller than its own codes with their headers: this is what
    // holds every band to 32 bits a pixel (webp_max_file_bytes)
    const bool literals = !constant && static_cast<uint64_t>(a.flat_group_bits) + 32ull * constant_px < static_cast<uint64_t>(pos) + own;
    __syncthreads();
    if (literals) {                                            // (the whole workgroup)
        for (uint32_t s = tid; s < kWebpSyms; s += 256u) cnt[s] = s < kWebpD && (s < 256u || s >= kWebpR) ? 1u : 0u;
        for (uint32_t i = tid; i < kWebpGroupWords; i += 256u) hdr[i] = 0;
        if (tid == 0u) pos = 0;
        __syncthreads();
        webp_build_codes(W, cnt, tab, hdr, &pos, true);
    }
    const size_t g = static_cast<size_t>(img) * a.S.n_bands + band;
    for (uint32_t s = tid; s < kWebpSyms; s += 256u) a.grp_tab[g * kWebpSyms + s] = tab[s];
    for (uint32_t i = tid; i < kWebpGroupWords; i += 256u) a.grp_hdr[g * kWebpGroupWords + i] = hdr[i];
    if (tid == 0u) { a.grp_hbits[g] = pos; a.grp_literal[g] = (literals || constant) ? 1u : 0u; }
    for (uint32_t j = tid; j < a.S.segs_per_band; j += 256u) {
        uint32_t start;
        a.seg_bits[seg0 + j] = literals ? 32u * webp_segment(a.S, band * a.S.segs_per_band + j, &start) : seg_own[j];
    }
}

// ---- layout: a workgroup per image -----------------------------------------------------------------------------------------------
// `count` literal pixels of a sub-image (pixel(i): its ARGB) under tab, from bit `where` of the payload
template <typename Pixel>
__device__ __forceinline__ void webp_emit_sub_image(uint32_t* words, uint64_t where, const uint32_t* tab, uint32_t count, uint32_t* wsum, GlobalOr go, Pixel pixel) {
    for (uint32_t base = 0; base < count; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        uint64_t v = 0;
        const uint32_t nb = i < count ? webp_token_bits(tab, 1u, pixel(i), &v) : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<1024>(nb, wsum, &total);
        if (nb) or_bits(words, where + ex, v, go);
        where += total;
    }
}
__global__ __launch_bounds__(1024) void webp_layout_kernel(const WebpArgs a) {
    __shared__ WebpCodeWork W;
    __shared__ uint32_t cnt[kWebpSyms], mode_tab[kWebpSyms], ent_tab[kWebpSyms], front[kWebpSubWords], middle[kWebpSubWords];
    __shared__ uint32_t front_bits, middle_bits, wsum[16], overflow;
    __shared__ uint64_t at_mode_px, at_middle, at_ent_px, at_groups, at_segs;
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    const uint32_t n_tiles = a.S.tiles_x * a.S.tiles_y, n_ent = a.S.ent_x * a.S.n_bands, ent_x = a.S.ent_x;
    const uint8_t* modes = a.modes + static_cast<size_t>(img) * n_tiles;
    for (uint32_t s = tid; s < kWebpSyms; s += 1024u) cnt[s] = 0;
    for (uint32_t i = tid; i < kWebpSubWords; i += 1024u) { front[i] = 0; middle[i] = 0; }
    __syncthreads();
    for (uint32_t t = tid; t < n_tiles; t += 1024u) atomicAdd(&cnt[kWebpG + modes[t]], 1u);
    if (tid == 0u) {
        cnt[kWebpR] = n_tiles; cnt[kWebpB] = n_tiles; cnt[kWebpA + 255u] = n_tiles;
        front_bits = 0; middle_bits = 0;
        webp_put_front(front, &front_bits, a.S.w, a.S.h, a.alpha_or ? 0u : 1u);
    }
    __syncthreads();
    webp_build_codes(W, cnt, mode_tab, front, &front_bits, false);
    if (tid == 0u) {
        uint64_t bits = 0;
        for (uint32_t s = 0; s < 14u; ++s) bits += static_cast<uint64_t>(cnt[kWebpG + s]) * (mode_tab[kWebpG + s] >> 16);   // the other four codes have one symbol
        at_mode_px = front_bits; at_middle = front_bits + bits;
    }
    __syncthreads();
    for (uint32_t s = tid; s < kWebpSyms; s += 1024u) cnt[s] = 0;
    __syncthreads();
    if (tid < a.S.n_bands) cnt[kWebpG + tid] = ent_x;
    if (tid == 0u) {
        cnt[kWebpR] = n_ent; cnt[kWebpB] = n_ent; cnt[kWebpA + 255u] = n_ent;
        webp_put_middle(middle, &middle_bits);
    }
    __syncthreads();
    webp_build_codes(W, cnt, ent_tab, middle, &middle_bits, false);
    if (tid == 0u) {
        uint64_t bits = 0;
        for (uint32_t s = 0; s < 256u; ++s) bits += static_cast<uint64_t>(cnt[kWebpG + s]) * (ent_tab[kWebpG + s] >> 16);
        at_ent_px = at_middle + middle_bits;
        uint64_t at = at_ent_px + bits;
        at_groups = at;
        for (uint32_t b = 0; b < a.S.n_bands; ++b) {           // at most 256 groups
            a.grp_off[static_cast<size_t>(img) * a.S.n_bands + b] = at;
            at += a.grp_hbits[static_cast<size_t>(img) * a.S.n_bands + b];
        }
        at_segs = at;
    }
    __syncthreads();
    uint64_t at = at_segs;
    for (uint32_t base = 0; base < a.S.n_segs; base += 1024u) {
        const uint32_t seg = base + tid;
        const uint32_t bits = seg < a.S.n_segs ? a.seg_bits[static_cast<size_t>(img) * a.S.n_segs + seg] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<1024>(bits, wsum, &total);  // (1024 segments hold fewer than 2^32 bits)
        if (seg < a.S.n_segs) a.seg_off[static_cast<size_t>(img) * a.S.n_segs + seg] = at + ex;
        at += total;
    }
    const uint64_t payload = (at + 7u) >> 3, file_len = kWebpRiff + payload + (payload & 1u);
    if (tid == 0u) {
        overflow = file_len > a.file_pitch ? 1u : 0u;
        a.image[4u * img] = overflow;
        a.image[4u * img + 1u] = static_cast<uint32_t>(payload);
    }
    __syncthreads();
    if (overflow) return;                                      // (the whole workgroup) nothing of this image is written
    uint32_t origin;
    uint32_t* words = webp_payload_words(a, img, &origin);
    const GlobalOr go = webp_global_or(a, img);
    for (uint32_t i = tid; i < (front_bits + 31u) / 32u; i += 1024u) or_bits(words, origin + 32ull * i, front[i], go);
    for (uint32_t i = tid; i < (middle_bits + 31u) / 32u; i += 1024u) or_bits(words, origin + at_middle + 32ull * i, middle[i], go);
    webp_emit_sub_image(words, origin + at_mode_px, mode_tab, n_tiles, wsum, go, [&](uint32_t i) { return 0xFF000000u | (static_cast<uint32_t>(modes[i]) << 8); });
    webp_emit_sub_image(words, origin + at_ent_px, ent_tab, n_ent, wsum, go, [&](uint32_t i) { return 0xFF000000u | ((i / ent_x) << 8); });
}

// ---- emit: a workgroup per segment, then one per group header --------------------------------------------------------------------
constexpr uint32_t kWebpWindowWords = kWebpSegMaxBits / 32u + 2u;
__global__ __launch_bounds__(1024) void webp_emit_kernel(const WebpArgs a) {
    __shared__ uint32_t tab[kWebpSyms], win[kWebpWindowWords], wsum[16];
    const uint32_t tid = threadIdx.x, img = blockIdx.y;
    if (a.image[4u * img]) return;
    uint32_t origin;
    uint32_t* words = webp_payload_words(a, img, &origin);
    const GlobalOr go = webp_global_or(a, img);
    if (blockIdx.x >= a.S.n_segs) {                            // a group's header: its dwords, shifted to the group's bit offset
        const size_t g = static_cast<size_t>(img) * a.S.n_bands + (blockIdx.x - a.S.n_segs);
        const uint32_t bits = a.grp_hbits[g];
        const uint64_t where = origin + a.grp_off[g];
        for (uint32_t i = tid; i < (bits + 31u) / 32u; i += 1024u) or_bits(words, where + 32ull * i, a.grp_hdr[g * kWebpGroupWords + i], go);
        return;
    }
    const uint32_t seg = blockIdx.x;
    uint32_t start;
    const uint32_t n = webp_segment(a.S, seg, &start);
    if (n == 0u) return;
    const size_t si = static_cast<size_t>(img) * a.S.n_segs + seg;
    const uint32_t seg_bits = a.seg_bits[si];
    if (seg_bits == 0u) return;                                // a band of one residual pixel throughout: its one-symbol codes take no bits
    const uint64_t where = origin + a.seg_off[si];
    const uint32_t shift = static_cast<uint32_t>(where) & 31u, n_words = (shift + seg_bits + 31u) / 32u;
    const size_t g = static_cast<size_t>(img) * a.S.n_bands + seg / a.S.segs_per_band;
    const uint32_t* gtab = a.grp_tab + g * kWebpSyms;
    const bool literals = a.grp_literal[g] != 0u;
    for (uint32_t s = tid; s < kWebpSyms; s += 1024u) tab[s] = gtab[s];
    for (uint32_t i = tid; i < n_words; i += 1024u) win[i] = 0;
    __syncthreads();
    const uint32_t* resid = a.resid + static_cast<size_t>(img) * a.px_pitch + start;
    const uint32_t* tok = a.tok + static_cast<size_t>(img) * a.px_pitch + start;
    uint64_t v[4];
    uint32_t nb[4], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = 4u * tid + k;
        const uint32_t t = i < n ? (literals ? 1u : tok[i]) : 0u;
        v[k] = 0;
        nb[k] = t ? webp_token_bits(tab, t, resid[i], &v[k]) : 0u;
        mine += nb[k];
    }
    uint32_t total;
    uint32_t at = shift + block_exclusive_scan<1024>(mine, wsum, &total);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (nb[k]) or_bits(win, at, v[k], [](uint32_t* p, uint32_t x) { atomicOr(p, x); });
        at += nb[k];
    }
    __syncthreads();
    // the first and the last dword may be shared with what lies in front and behind; the others are this segment's alone
    uint32_t* out = words + (where >> 5);
    for (uint32_t i = tid; i < n_words; i += 1024u) {
        if (i == 0u || i + 1u == n_words) { if (win[i]) go(out + i, win[i]); } else out[i] = win[i];   // (the tail dword is nobody's inner dword)
    }
}

// ---- finish: a lane per image ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void webp_finish_kernel(const WebpArgs a) {
    const uint32_t img = blockIdx.x * 64u + threadIdx.x;
    if (img >= a.n_images) return;
    if (a.image[4u * img]) {
        a.lengths[img] = 0u;
        if (a.status_out) a.status_out[img] = kWebpFileOverflow;
        return;
    }
    a.lengths[img] = webp_write_riff(a.files + static_cast<size_t>(img) * a.file_pitch, a.image[4u * img + 1u]);
    const GlobalOr go = webp_global_or(a, img);
    if (go.tail) {                                             // the image's bytes of the dword that reaches past its pitch
        const uint32_t mine = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(a.files) + static_cast<size_t>(img + 1u) * a.file_pitch) & 3u);
        for (uint32_t k = 0; k < mine; ++k) reinterpret_cast<uint8_t*>(go.tail)[k] = static_cast<uint8_t>(*go.spare >> (8u * k));
    }
    if (a.status_out) a.status_out[img] = 0u;
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_webp_enc_stage {
    uint32_t width = 0, height = 0, alpha = 0, max_images = 0;
    WebpShape S{};
    size_t px_pitch = 0;
    uint32_t *d_resid = nullptr, *d_tok = nullptr, *d_seg_hist = nullptr, *d_seg_bits = nullptr, *d_seg_flat = nullptr, *d_grp_tab = nullptr, *d_grp_hdr = nullptr,
             *d_grp_hbits = nullptr, *d_grp_literal = nullptr, *d_image = nullptr;
    uint8_t* d_modes = nullptr;
    uint64_t *d_seg_off = nullptr, *d_grp_off = nullptr;
    uint32_t flat_group_bits = 0;
    StageScratch blocks{&d_resid, &d_tok, &d_modes, &d_seg_hist, &d_seg_bits, &d_seg_flat, &d_seg_off, &d_grp_off, &d_grp_tab, &d_grp_hdr, &d_grp_hbits, &d_grp_literal, &d_image};
    int allocate() {                    // (the first batch does it, behind the argument checks)
        const size_t n = max_images, segs = n * S.n_segs, bands = n * S.n_bands;
        return blocks.ensure([&]() -> int {
            HIP_TRY(DEV_MALLOC(&d_resid, n * px_pitch * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_tok, n * px_pitch * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_modes, n * S.tiles_x * S.tiles_y));
            HIP_TRY(DEV_MALLOC(&d_seg_hist, segs * kWebpSyms * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_seg_bits, segs * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_seg_flat, segs * 2u * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_seg_off, segs * sizeof(uint64_t)));
            HIP_TRY(DEV_MALLOC(&d_grp_off, bands * sizeof(uint64_t)));
            HIP_TRY(DEV_MALLOC(&d_grp_tab, bands * kWebpSyms * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_grp_hdr, bands * kWebpGroupWords * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_grp_hbits, bands * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_grp_literal, bands * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_image, n * 4u * sizeof(uint32_t)));
            return IFHIP_OK;
        });
    }
};

extern "C" {

int ifhip_webp_enc_stage_create(ifhip_webp_enc_stage** stage, uint32_t width, uint32_t height, int alpha_meaningful, uint32_t max_images) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage out-pointer");
    *stage = nullptr;
    if (width == 0 || height == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (width > kWebpMaxDim || height > kWebpMaxDim) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a WebP frame is at most %u x %u (14 bits each), not %u x %u", kWebpMaxDim, kWebpMaxDim, width, height);
    if (max_images == 0 || max_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 images per stage");
    std::unique_ptr<ifhip_webp_enc_stage> s(new ifhip_webp_enc_stage);
    s->width = width; s->height = height; s->alpha = alpha_meaningful ? 1u : 0u; s->max_images = max_images;
    s->S = webp_shape(width, height);
    s->px_pitch = (static_cast<size_t>(width) * height + 3u) & ~static_cast<size_t>(3u);
    { WebpCodeWork work; s->flat_group_bits = webp_flat_group_bits(work); }
    *stage = s.release();
    return IFHIP_OK;
}

void ifhip_webp_enc_stage_destroy(ifhip_webp_enc_stage* stage) { delete stage; }

size_t ifhip_webp_enc_stage_max_file_bytes(const ifhip_webp_enc_stage* stage) { return stage ? static_cast<size_t>(webp_max_file_bytes(stage->width, stage->height)) : 0u; }

int ifhip_webp_encode_batch_device(ifhip_webp_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, uint32_t n_images,
                                   uint8_t* d_files, size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status, void* hip_stream) {
    bool go = false;
    if (int rc = open_encode_batch(stage, d_images, image_bytes, stride, n_images, d_files, d_lengths, &go); rc || !go) return rc;
    if (reinterpret_cast<uintptr_t>(d_files) & 3u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: d_files must be 4-byte aligned");
    if (file_pitch < kWebpRiff + 8u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: file_pitch below %u bytes", kWebpRiff + 8u);
    if (int rc = stage->allocate()) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const WebpShape& S = stage->S;
    const WebpArgs a{d_images, image_bytes, stride, stage->alpha ? 0u : 0xFF000000u, n_images, S, stage->px_pitch, stage->d_resid, stage->d_tok, stage->d_modes,
                     stage->d_seg_hist, stage->d_seg_bits, stage->d_seg_flat, stage->d_seg_off, stage->d_grp_off, stage->d_grp_tab, stage->d_grp_hdr,
                     stage->d_grp_hbits, stage->d_grp_literal, stage->flat_group_bits, stage->d_image, d_files, file_pitch, d_lengths, d_status};
    // everything of the payload is ORed into place: the files start out as zeros (which also is the pad byte)
    HIP_TRY(hipMemsetAsync(d_files, 0, static_cast<size_t>(n_images) * file_pitch, st));
    HIP_TRY(hipMemsetAsync(stage->d_image, 0, static_cast<size_t>(n_images) * 4u * sizeof(uint32_t), st));
    hipLaunchKernelGGL(webp_residual_kernel, dim3(S.tiles_x, S.tiles_y, n_images), dim3(256), 0, st, a);
    hipLaunchKernelGGL(webp_parse_kernel, dim3(S.n_segs, n_images), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(webp_codes_kernel, dim3(S.n_bands, n_images), dim3(256), 0, st, a);
    hipLaunchKernelGGL(webp_layout_kernel, dim3(n_images), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(webp_emit_kernel, dim3(S.n_segs + S.n_bands, n_images), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(webp_finish_kernel, dim3((n_images + 63u) / 64u), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_webp_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful, uint8_t* out, size_t capacity, size_t* len) {
    uint32_t status = 0;
    if (int rc = encode_host_frame(
            bgra, width, height, stride, out, capacity, len, &status, [&](ifhip_webp_enc_stage** s) { return ifhip_webp_enc_stage_create(s, width, height, alpha_meaningful, 1); },
            ifhip_webp_enc_stage_destroy, ifhip_webp_enc_stage_max_file_bytes, [&](ifhip_webp_enc_stage* s, const HostFrame& f, size_t pitch, uint32_t* d_len) {
                return ifhip_webp_encode_batch_device(s, f.d, f.image_bytes, stride, 1, f.side_output(), pitch, d_len, d_len + 1, nullptr);
            })) return rc;
    return refuse_unfitted_file(status, *len);
}

}  // extern "C"
