// webp_encode_device.hpp -- the device code the kernels of the lossless-WebP coder share: webp_encode.hip launches it over
// the stage's own geometry (subtract green and a predictor per tile), webp_encode_indexed.hip over the packed image of a
// frame of few colours, whose shape only the device knows.  So every body takes the image's shape `S` beside the arguments:
// `a.S` is the stage's full geometry and sets the pitch of the per-image arrays, `S` says where the image's own segments,
// bands and pixels lie within them (S.n_segs <= a.S.n_segs, S.n_bands == a.S.n_bands).
#pragma once
#include <hip/hip_runtime.h>

#include "block_scan.hpp"
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
    uint32_t* image;                    // [n_images][4]: overflow, payload bytes, the tail dword (zeroed per batch), the variant written (0 plain, 1 indexed)
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

// ---- parse: a workgroup of 1024 per segment --------------------------------------------------------------------------------------
__device__ __forceinline__ void webp_parse_segment(const WebpArgs& a, const WebpShape& S, uint32_t seg, uint32_t img) {
    __shared__ uint32_t r[kWebpSeg];
    __shared__ uint16_t len16[kWebpSeg], nxt[2][kWebpSeg];
    __shared__ uint8_t sel[kWebpSeg], mark[kWebpSeg];
    __shared__ uint16_t suf[2][2][1024 + 1];                   // [distance][buffer]: the first break at or behind a lane's positions
    __shared__ uint32_t hist[kWebpSyms];
    const uint32_t tid = threadIdx.x;
    uint32_t start;
    const uint32_t n = webp_segment(S, seg, &start);
    uint32_t* out_hist = a.seg_hist + (static_cast<size_t>(img) * a.S.n_segs + seg) * kWebpSyms;
    for (uint32_t s = tid; s < kWebpSyms; s += 1024u) hist[s] = 0;
    if (n == 0u) {                                             // (the whole workgroup) an empty segment of the last band counts nothing
        for (uint32_t s = tid; s < kWebpSyms; s += 1024u) out_hist[s] = 0;
        return;
    }
    const uint32_t* resid = a.resid + static_cast<size_t>(img) * a.px_pitch;
    uint32_t* tok = a.tok + static_cast<size_t>(img) * a.px_pitch;
    const uint32_t w = S.w;
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

// ---- codes: a workgroup of 256 per band ------------------------------------------------------------------------------------------
__device__ __forceinline__ void webp_code_band(const WebpArgs& a, const WebpShape& S, uint32_t band, uint32_t img) {
    __shared__ WebpCodeWork W;
    __shared__ uint32_t cnt[kWebpSyms], tab[kWebpSyms], hdr[kWebpGroupWords];
    __shared__ uint32_t pos, acc, own, constant, constant_px, constant_value, seg_own[256];
    const uint32_t tid = threadIdx.x;
    const size_t seg0 = static_cast<size_t>(img) * a.S.n_segs + static_cast<size_t>(band) * S.segs_per_band;
    for (uint32_t s = tid; s < kWebpSyms; s += 256u) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < S.segs_per_band; ++j) c += a.seg_hist[(seg0 + j) * kWebpSyms + s];
        cnt[s] = c;
    }
    for (uint32_t i = tid; i < kWebpGroupWords; i += 256u) hdr[i] = 0;
    if (tid == 0u) {
        pos = 0; acc = 0; own = 0;
        uint32_t flat = 1u, px = 0;                              // (at most 256 segments)
        const uint32_t value = a.seg_flat[seg0 * 2u + 1u];
        for (uint32_t j = 0; j < S.segs_per_band; ++j) {
            uint32_t start;
            const uint32_t n = webp_segment(S, band * S.segs_per_band + j, &start);
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
    for (uint32_t j = 0; j < S.segs_per_band; ++j) {           // histogram . (lengths + extra bits): no count pass over the tokens
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
    for (uint32_t j = tid; j < S.segs_per_band; j += 256u) {
        uint32_t start;
        a.seg_bits[seg0 + j] = literals ? 32u * webp_segment(S, band * S.segs_per_band + j, &start) : seg_own[j];
    }
}

// ---- layout: a workgroup of 1024 per image ---------------------------------------------------------------------------------------
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
// What the layout keeps in LDS of a variant's head: the codes of its first sub-image (the tiles' modes, or the colour
// table) behind the front's own bits, the codes of the entropy sub-image behind the middle's, and where their pixels go.
struct WebpHead {
    uint32_t sub_tab[kWebpSyms], ent_tab[kWebpSyms], front[kWebpGroupWords], middle[kWebpSubWords];
    uint32_t front_bits, middle_bits;
    uint64_t at_sub_px, at_middle, at_ent_px, at_segs;
};
struct WebpLayoutWork {
    WebpCodeWork W;
    uint32_t cnt[kWebpSyms], wsum[16];
};
// The head's codes and every bit offset of the image under `a` and `S`.  kIndexed: the first sub-image is the colour table
// `pal` of `n_colours` entries (its differences); otherwise the tiles' modes.  Returns the payload's bits, in every lane.
template <bool kIndexed>
__device__ __forceinline__ uint64_t webp_plan_layout(const WebpArgs& a, const WebpShape& S, uint32_t img, WebpHead& H, WebpLayoutWork& L, uint32_t frame_w,
                                                      const uint32_t* pal, uint32_t n_colours) {
    const uint32_t tid = threadIdx.x;
    const uint32_t n_tiles = S.tiles_x * S.tiles_y, n_ent = S.ent_x * S.n_bands;
    const uint8_t* modes = a.modes + static_cast<size_t>(img) * a.S.tiles_x * a.S.tiles_y;
    for (uint32_t s = tid; s < kWebpSyms; s += 1024u) L.cnt[s] = 0;
    for (uint32_t i = tid; i < kWebpGroupWords; i += 1024u) H.front[i] = 0;
    for (uint32_t i = tid; i < kWebpSubWords; i += 1024u) H.middle[i] = 0;
    __syncthreads();
    if (kIndexed) {
        if (tid < n_colours) {
            const WebpTokenSymbols sy = webp_count_token(1u, webp_palette_delta(pal, tid));
            atomicAdd(&L.cnt[sy.s0], 1u); atomicAdd(&L.cnt[sy.s1], 1u); atomicAdd(&L.cnt[sy.s2], 1u); atomicAdd(&L.cnt[sy.s3], 1u);
        }
    } else {
        for (uint32_t t = tid; t < n_tiles; t += 1024u) atomicAdd(&L.cnt[kWebpG + modes[t]], 1u);
    }
    if (tid == 0u) {
        H.front_bits = 0; H.middle_bits = 0;
        if (kIndexed) {
            webp_put_front_indexed(H.front, &H.front_bits, frame_w, S.h, a.alpha_or ? 0u : 1u, n_colours);
        } else {
            L.cnt[kWebpR] = n_tiles; L.cnt[kWebpB] = n_tiles; L.cnt[kWebpA + 255u] = n_tiles;
            webp_put_front(H.front, &H.front_bits, S.w, S.h, a.alpha_or ? 0u : 1u);
        }
    }
    __syncthreads();
    webp_build_codes(L.W, L.cnt, H.sub_tab, H.front, &H.front_bits, false);
    if (tid == 0u) {
        uint64_t bits = 0;
        const uint32_t used = kIndexed ? kWebpD : 14u;          // (the modes' other four codes have one symbol)
        for (uint32_t s = 0; s < used; ++s) bits += static_cast<uint64_t>(L.cnt[s]) * (H.sub_tab[s] >> 16);
        H.at_sub_px = H.front_bits; H.at_middle = H.front_bits + bits;
    }
    __syncthreads();
    for (uint32_t s = tid; s < kWebpSyms; s += 1024u) L.cnt[s] = 0;
    __syncthreads();
    if (tid < S.n_bands) L.cnt[kWebpG + tid] = S.ent_x;
    if (tid == 0u) {
        L.cnt[kWebpR] = n_ent; L.cnt[kWebpB] = n_ent; L.cnt[kWebpA + 255u] = n_ent;
        webp_put_middle(H.middle, &H.middle_bits);
    }
    __syncthreads();
    webp_build_codes(L.W, L.cnt, H.ent_tab, H.middle, &H.middle_bits, false);
    if (tid == 0u) {
        uint64_t bits = 0;
        for (uint32_t s = 0; s < 256u; ++s) bits += static_cast<uint64_t>(L.cnt[kWebpG + s]) * (H.ent_tab[kWebpG + s] >> 16);
        H.at_ent_px = H.at_middle + H.middle_bits;
        uint64_t at = H.at_ent_px + bits;
        for (uint32_t b = 0; b < S.n_bands; ++b) {             // at most 256 groups
            a.grp_off[static_cast<size_t>(img) * a.S.n_bands + b] = at;
            at += a.grp_hbits[static_cast<size_t>(img) * a.S.n_bands + b];
        }
        H.at_segs = at;
    }
    __syncthreads();
    uint64_t at = H.at_segs;
    for (uint32_t base = 0; base < S.n_segs; base += 1024u) {
        const uint32_t seg = base + tid;
        const uint32_t bits = seg < S.n_segs ? a.seg_bits[static_cast<size_t>(img) * a.S.n_segs + seg] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<1024>(bits, L.wsum, &total);  // (1024 segments hold fewer than 2^32 bits)
        if (seg < S.n_segs) a.seg_off[static_cast<size_t>(img) * a.S.n_segs + seg] = at + ex;
        at += total;
    }
    return at;
}
IFHIP_HD uint64_t webp_file_bytes(uint64_t payload_bits) {
    const uint64_t payload = (payload_bits + 7u) >> 3;
    return kWebpRiff + payload + (payload & 1u);
}
// the head's bits into the (zeroed) file
template <bool kIndexed>
__device__ __forceinline__ void webp_write_head(const WebpArgs& a, const WebpShape& S, uint32_t img, const WebpHead& H, WebpLayoutWork& L, const uint32_t* pal,
                                                uint32_t n_colours) {
    const uint32_t tid = threadIdx.x, ent_x = S.ent_x;
    uint32_t origin;
    uint32_t* words = webp_payload_words(a, img, &origin);
    const GlobalOr go = webp_global_or(a, img);
    for (uint32_t i = tid; i < (H.front_bits + 31u) / 32u; i += 1024u) or_bits(words, origin + 32ull * i, H.front[i], go);
    for (uint32_t i = tid; i < (H.middle_bits + 31u) / 32u; i += 1024u) or_bits(words, origin + H.at_middle + 32ull * i, H.middle[i], go);
    if (kIndexed) {
        webp_emit_sub_image(words, origin + H.at_sub_px, H.sub_tab, n_colours, L.wsum, go, [&](uint32_t i) { return webp_palette_delta(pal, i); });
    } else {
        const uint8_t* modes = a.modes + static_cast<size_t>(img) * a.S.tiles_x * a.S.tiles_y;
        webp_emit_sub_image(words, origin + H.at_sub_px, H.sub_tab, S.tiles_x * S.tiles_y, L.wsum, go,
                            [&](uint32_t i) { return 0xFF000000u | (static_cast<uint32_t>(modes[i]) << 8); });
    }
    webp_emit_sub_image(words, origin + H.at_ent_px, H.ent_tab, ent_x * S.n_bands, L.wsum, go, [&](uint32_t i) { return 0xFF000000u | ((i / ent_x) << 8); });
}

// ---- emit: a workgroup of 1024 per segment, and one per group header ---------------------------------------------------------------
constexpr uint32_t kWebpWindowWords = kWebpSegMaxBits / 32u + 2u;
// a group's header: its dwords, shifted to the group's bit offset
__device__ __forceinline__ void webp_emit_group_header(const WebpArgs& a, uint32_t band, uint32_t img) {
    uint32_t origin;
    uint32_t* words = webp_payload_words(a, img, &origin);
    const GlobalOr go = webp_global_or(a, img);
    const size_t g = static_cast<size_t>(img) * a.S.n_bands + band;
    const uint32_t bits = a.grp_hbits[g];
    const uint64_t where = origin + a.grp_off[g];
    for (uint32_t i = threadIdx.x; i < (bits + 31u) / 32u; i += 1024u) or_bits(words, where + 32ull * i, a.grp_hdr[g * kWebpGroupWords + i], go);
}
// a segment's tokens: bits into an LDS window, shifted by the segment's bit offset
__device__ __forceinline__ void webp_emit_segment(const WebpArgs& a, const WebpShape& S, uint32_t seg, uint32_t img) {
    __shared__ uint32_t tab[kWebpSyms], win[kWebpWindowWords], wsum[16];
    const uint32_t tid = threadIdx.x;
    uint32_t origin;
    uint32_t* words = webp_payload_words(a, img, &origin);
    const GlobalOr go = webp_global_or(a, img);
    uint32_t start;
    const uint32_t n = webp_segment(S, seg, &start);
    if (n == 0u) return;
    const size_t si = static_cast<size_t>(img) * a.S.n_segs + seg;
    const uint32_t seg_bits = a.seg_bits[si];
    if (seg_bits == 0u) return;                                // a band of one residual pixel throughout: its one-symbol codes take no bits
    const uint64_t where = origin + a.seg_off[si];
    const uint32_t shift = static_cast<uint32_t>(where) & 31u, n_words = (shift + seg_bits + 31u) / 32u;
    const size_t g = static_cast<size_t>(img) * a.S.n_bands + seg / S.segs_per_band;
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

}  // namespace ifhip
