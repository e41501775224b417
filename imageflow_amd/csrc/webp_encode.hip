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
// The bodies of parse, codes, layout and emit are webp_encode_device.hpp's, shared with the colour indexing a stage may carry
// as a flag (webp_encode_indexed.hip): its launches go around these, and without the flag these are all there is.
// Every rule with a bit in it lives in webp_encode_core.hpp (VP8L's own) and prefix_code_core.hpp (what every prefix
// code shares), both compiled into the CPU emulation of the tests as well (tests/webp_emulate.cpp).  Everything reduced across lanes is an integer sum or an OR: the same pixels give the same
// bytes on every run and in every batch position.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "encode_handoff.hpp"
#include "stage_scratch.hpp"
#include "webp_encode_device.hpp"
#include "webp_encode_indexed.hpp"

namespace ifhip {

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
__global__ __launch_bounds__(1024) void webp_parse_kernel(const WebpArgs a) { webp_parse_segment(a, a.S, blockIdx.x, blockIdx.y); }

// ---- codes: a workgroup per band -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void webp_codes_kernel(const WebpArgs a) { webp_code_band(a, a.S, blockIdx.x, blockIdx.y); }

// ---- layout: a workgroup per image -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void webp_layout_kernel(const WebpArgs a) {
    __shared__ WebpHead H;
    __shared__ WebpLayoutWork L;
    __shared__ uint32_t overflow;
    const uint32_t img = blockIdx.x;
    const uint64_t at = webp_plan_layout<false>(a, a.S, img, H, L, a.S.w, nullptr, 0u);
    if (threadIdx.x == 0u) {
        overflow = webp_file_bytes(at) > a.file_pitch ? 1u : 0u;
        a.image[4u * img] = overflow;
        a.image[4u * img + 1u] = static_cast<uint32_t>((at + 7u) >> 3);
    }
    __syncthreads();
    if (overflow) return;                                      // (the whole workgroup) nothing of this image is written
    webp_write_head<false>(a, a.S, img, H, L, nullptr, 0u);
}

// ---- emit: a workgroup per segment, then one per group header --------------------------------------------------------------------
__global__ __launch_bounds__(1024) void webp_emit_kernel(const WebpArgs a) {
    const uint32_t img = blockIdx.y;
    if (a.image[4u * img]) return;
    if (blockIdx.x >= a.S.n_segs) webp_emit_group_header(a, blockIdx.x - a.S.n_segs, img);
    else webp_emit_segment(a, a.S, blockIdx.x, img);
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
    // IFHIP_WEBP_ENC_COLOR_INDEXING: the packed image's own scratch (bits 0 pack nothing, so it is the plain one's size), the
    // colour sets and the images' records
    uint32_t flags = 0;
    struct Packed {
        uint32_t *d_resid = nullptr, *d_tok = nullptr, *d_seg_hist = nullptr, *d_seg_bits = nullptr, *d_seg_flat = nullptr, *d_grp_tab = nullptr, *d_grp_hdr = nullptr,
                 *d_grp_hbits = nullptr, *d_grp_literal = nullptr, *d_sets = nullptr;
        uint64_t *d_seg_off = nullptr, *d_grp_off = nullptr;
        WebpIndexRecord* d_rec = nullptr;
        StageScratch blocks{&d_resid, &d_tok, &d_seg_hist, &d_seg_bits, &d_seg_flat, &d_seg_off, &d_grp_off, &d_grp_tab, &d_grp_hdr, &d_grp_hbits, &d_grp_literal, &d_sets, &d_rec};
    } packed;
    int allocate_packed() {
        const size_t n = max_images, segs = n * S.n_segs, bands = n * S.n_bands;
        Packed& p = packed;
        return p.blocks.ensure([&]() -> int {
            HIP_TRY(DEV_MALLOC(&p.d_resid, n * px_pitch * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_tok, n * px_pitch * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_seg_hist, segs * kWebpSyms * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_seg_bits, segs * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_seg_flat, segs * 2u * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_seg_off, segs * sizeof(uint64_t)));
            HIP_TRY(DEV_MALLOC(&p.d_grp_off, bands * sizeof(uint64_t)));
            HIP_TRY(DEV_MALLOC(&p.d_grp_tab, bands * kWebpSyms * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_grp_hdr, bands * kWebpGroupWords * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_grp_hbits, bands * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_grp_literal, bands * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_sets, n * kWebpSetWords * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&p.d_rec, n * sizeof(WebpIndexRecord)));
            return IFHIP_OK;
        });
    }
};

extern "C" {

int ifhip_webp_enc_stage_create(ifhip_webp_enc_stage** stage, uint32_t width, uint32_t height, int alpha_meaningful, uint32_t max_images) {
    return ifhip_webp_enc_stage_create_flags(stage, width, height, alpha_meaningful, max_images, 0u);
}

int ifhip_webp_enc_stage_create_flags(ifhip_webp_enc_stage** stage, uint32_t width, uint32_t height, int alpha_meaningful, uint32_t max_images, uint32_t flags) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage out-pointer");
    *stage = nullptr;
    if (width == 0 || height == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (width > kWebpMaxDim || height > kWebpMaxDim) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a WebP frame is at most %u x %u (14 bits each), not %u x %u", kWebpMaxDim, kWebpMaxDim, width, height);
    if (max_images == 0 || max_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 images per stage");
    if (flags & ~IFHIP_WEBP_ENC_COLOR_INDEXING) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: unknown WebP stage flags 0x%x", flags & ~IFHIP_WEBP_ENC_COLOR_INDEXING);
    std::unique_ptr<ifhip_webp_enc_stage> s(new ifhip_webp_enc_stage);
    s->flags = flags;
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
    if (stage->flags & IFHIP_WEBP_ENC_COLOR_INDEXING) if (int rc = stage->allocate_packed()) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const WebpShape& S = stage->S;
    const WebpArgs a{d_images, image_bytes, stride, stage->alpha ? 0u : 0xFF000000u, n_images, S, stage->px_pitch, stage->d_resid, stage->d_tok, stage->d_modes,
                     stage->d_seg_hist, stage->d_seg_bits, stage->d_seg_flat, stage->d_seg_off, stage->d_grp_off, stage->d_grp_tab, stage->d_grp_hdr,
                     stage->d_grp_hbits, stage->d_grp_literal, stage->flat_group_bits, stage->d_image, d_files, file_pitch, d_lengths, d_status};
    // everything of the payload is ORed into place: the files start out as zeros (which also is the pad byte)
    HIP_TRY(hipMemsetAsync(d_files, 0, static_cast<size_t>(n_images) * file_pitch, st));
    HIP_TRY(hipMemsetAsync(stage->d_image, 0, static_cast<size_t>(n_images) * 4u * sizeof(uint32_t), st));
    if (stage->flags & IFHIP_WEBP_ENC_COLOR_INDEXING) {
        // the packed image beside the plain one: both are sized, webp_ix_layout_kernel picks the file that is written
        const ifhip_webp_enc_stage::Packed& p = stage->packed;
        WebpArgs b = a;
        b.resid = p.d_resid; b.tok = p.d_tok; b.modes = nullptr; b.seg_hist = p.d_seg_hist; b.seg_bits = p.d_seg_bits; b.seg_flat = p.d_seg_flat;
        b.seg_off = p.d_seg_off; b.grp_off = p.d_grp_off; b.grp_tab = p.d_grp_tab; b.grp_hdr = p.d_grp_hdr; b.grp_hbits = p.d_grp_hbits; b.grp_literal = p.d_grp_literal;
        const WebpIndexArgs ix{p.d_sets, p.d_rec};
        if (int rc = webp_indexed_front(b, ix, st)) return rc;
        hipLaunchKernelGGL(webp_residual_kernel, dim3(S.tiles_x, S.tiles_y, n_images), dim3(256), 0, st, a);
        hipLaunchKernelGGL(webp_parse_kernel, dim3(S.n_segs, n_images), dim3(1024), 0, st, a);
        hipLaunchKernelGGL(webp_codes_kernel, dim3(S.n_bands, n_images), dim3(256), 0, st, a);
        if (int rc = webp_indexed_back(a, b, ix, st)) return rc;
        hipLaunchKernelGGL(webp_finish_kernel, dim3((n_images + 63u) / 64u), dim3(64), 0, st, a);
        HIP_TRY(hipGetLastError());
        return IFHIP_OK;
    }
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
