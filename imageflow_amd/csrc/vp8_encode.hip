// vp8_encode.hip -- gfx950 kernels + C ABI of the device lossy WebP coder: BGRA / BGRX frames in HBM -> complete lossy WebP
// files (`VP8 `, with `VP8X` + `ALPH` where a frame has meaningful alpha below 255) in HBM.
//
// Replaces what EncoderPreset::WebPLossy runs on the host (codecs/webp.rs: WebPEncodeBGRA / WebPEncodeBGR of libwebp).  The
// contract is not libwebp's bytes: the file equals the CPU emulation's (tests/vp8_encode_emulate.cpp) byte for byte, and
// libwebp decodes it to the pixels the coder itself reconstructed.  Launches per batch, every image in each:
//   convert   grid-wide, a thread per 2x2 pixels: Y and the box-averaged U, V into planes of whole macroblocks (edges
//             replicated), the grey frame B = G = R = alpha for the inner lossless coder, "any alpha below 255" per image
//   (inner)   the lossless coder's own launches over the grey frames (csrc/webp_encode.hip), where the stage has alpha
//   code      (a stage with IFHIP_VP8_ENC_INTRA4 launches vp8e_code4_kernel of csrc/vp8_encode_intra4.hip in its place)
//             ONE WORKGROUP OF 8 WAVES PER IMAGE: whole-macroblock modes need the left, above and above-left neighbours,
//             so macroblock (x, y) runs in step x + y, the macroblocks of a step dealt to the waves, a workgroup barrier
//             between steps.  A wave tries the 4 x 16 (mode, luma block) and 4 x 8 (mode, chroma block) pairs a lane each:
//             prediction, forward DCT / WHT, dead-zone quantisation, the decoder's own reconstruction, squared error +
//             lambda * bits; then stores levels, the decoder's record and the reconstruction of the chosen modes.  A lone
//             large image keeps one compute unit busy: the limit of the decoder's wavefront, stated again.
//   count     grid-wide, a thread per macroblock: the branch counts of every (type, band, context, node) in an LDS
//             histogram per workgroup, summed into the image's by integer atomics; the skipped macroblocks
//   decide    one wave per image: which coefficient probabilities are updated, the skip probability
//   streams   the first partition and every token partition are serial bool-coded streams: one lane each, walking the
//             dense levels itself (the (bit, probability) record form was not built: its memory is tens of bytes a pixel)
//   layout    a workgroup per image: sizes, the overflow check, then every dword of the image's file_pitch bytes by the
//             lane that owns it (vp8e_file_byte: framing, ALPH from the inner file, partitions, zeros behind the file)
// No wave waits for another by polling; all control flow around a barrier is uniform in the workgroup.  Everything reduced
// across lanes is an integer sum or an OR: the same pixels give the same bytes on every run and in every batch position.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "../../include/imageflow_hip_webp_lossy_enc.h"
#include "encode_handoff.hpp"
#include "stage_scratch.hpp"
#include "vp8_encode_args.hpp"
#include "vp8_encode_core.hpp"
#include "webp_encode_core.hpp"

namespace ifhip {

__global__ __launch_bounds__(256) void vp8e_convert_kernel(const Vp8eArgs a) {
    const uint32_t img = blockIdx.y;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint32_t cw = a.mbw * 8u, ch = a.mbh * 8u;
    if (i >= static_cast<uint64_t>(cw) * ch) return;
    const Vp8Planes P = vp8e_planes(a, img, false);
    const Vp8eSource S{a.images + static_cast<size_t>(img) * a.image_bytes, a.stride, a.w, a.h, a.alpha, P.y, P.u, P.v,
                       a.grey ? a.grey + static_cast<size_t>(img) * a.w * a.h : nullptr, a.mbw, a.mbh};
    if (vp8e_convert_quad(S, static_cast<uint32_t>(i % cw), static_cast<uint32_t>(i / cw))) atomicOr(a.counts + static_cast<size_t>(img) * kVp8eCountWords + 2u * kVp8eProbs + 1u, 1u);
}

__global__ __launch_bounds__(64 * kVp8eWaves) void vp8e_code_kernel(const Vp8eArgs a) {
    __shared__ Vp8eMbWork work[kVp8eWaves];
    const uint32_t img = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    Vp8eFrame F;
    F.src = vp8e_planes(a, img, false); F.rec = vp8e_planes(a, img, true);
    F.mbs = a.mbs + static_cast<size_t>(img) * vp8e_mb_count(a);
    F.levels = a.levels + static_cast<size_t>(img) * vp8e_mb_count(a) * kVp8MbLevels;
    F.p = a.p;
    Vp8eMbWork& W = work[wave];
    auto sync = [] {                                                      // the wave's own LDS stores, before its other lanes read them
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    const uint32_t steps = a.mbw + a.mbh - 1u;
    for (uint32_t s = 0; s < steps; ++s) {
        const uint32_t lo = s >= a.mbw ? s - a.mbw + 1u : 0u, hi = min(a.mbh - 1u, s);
        for (uint32_t y = lo + wave; y <= hi; y += kVp8eWaves) vp8e_code_mb(*a.T, F, W, s - y, y, lane, 64u, sync);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");            // this step's pixels, before another wave's next step reads them
        __syncthreads();
    }
}

struct Vp8eAtomicCountSink {            // Vp8eCountSink over a histogram that many lanes share
    uint32_t* counts;
    __device__ void coef(uint32_t bit, uint32_t type, uint32_t band, uint32_t ctx, uint32_t node) { atomicAdd(&counts[2u * vp8e_prob_index(type, band, ctx, node) + bit], 1u); }
    __device__ void fixed(uint32_t, uint32_t) {}
};
__global__ __launch_bounds__(256) void vp8e_count_kernel(const Vp8eArgs a) {
    __shared__ uint32_t hist[kVp8eCountWords];
    const uint32_t img = blockIdx.y, tid = threadIdx.x;
    for (uint32_t i = tid; i < kVp8eCountWords; i += 256u) hist[i] = 0u;
    __syncthreads();
    const size_t n = vp8e_mb_count(a), m = static_cast<size_t>(blockIdx.x) * 256u + tid;
    if (m < n) {
        const Vp8Mb* mbs = a.mbs + static_cast<size_t>(img) * n;
        if (vp8e_mb_skipped(mbs[m])) atomicAdd(&hist[2u * kVp8eProbs], 1u);
        else {
            Vp8eAtomicCountSink s{hist};
            vp8e_mb_tokens(*a.T, a.levels + (static_cast<size_t>(img) * n + m) * kVp8MbLevels, mbs[m], m >= a.mbw ? vp8e_ctx_above(mbs[m - a.mbw]) : 0u, m % a.mbw ? vp8e_ctx_left(mbs[m - 1u]) : 0u, s);
        }
    }
    __syncthreads();
    uint32_t* out = a.counts + static_cast<size_t>(img) * kVp8eCountWords;
    for (uint32_t i = tid; i <= 2u * kVp8eProbs; i += 256u) if (hist[i]) atomicAdd(out + i, hist[i]);
}

__global__ __launch_bounds__(64) void vp8e_decide_kernel(const Vp8eArgs a) {
    const uint32_t img = blockIdx.x, lane = threadIdx.x;
    const uint32_t* counts = a.counts + static_cast<size_t>(img) * kVp8eCountWords;
    uint8_t* probs = a.probs + static_cast<size_t>(img) * kVp8eProbBytes;
    for (uint32_t i = lane; i < kVp8eProbs; i += 64u) {
        uint32_t updated;
        probs[i] = static_cast<uint8_t>(vp8e_decide_prob(counts[2u * i], counts[2u * i + 1u], a.T->proba0[i], a.T->update[i], &updated));
        probs[kVp8eProbs + i] = static_cast<uint8_t>(updated);
    }
    if (lane == 0u) probs[2u * kVp8eProbs] = static_cast<uint8_t>(vp8e_skip_prob(counts[2u * kVp8eProbs], static_cast<uint32_t>(vp8e_mb_count(a))));
}

__device__ __forceinline__ uint8_t* vp8e_stream(const Vp8eArgs& a, uint32_t img, uint32_t k) {
    return a.streams + static_cast<size_t>(img) * a.stream_pitch + (k ? a.first_cap + static_cast<size_t>(k - 1u) * a.part_cap : 0u);
}
__global__ __launch_bounds__(64) void vp8e_streams_kernel(const Vp8eArgs a) {
    const uint32_t k = blockIdx.x, img = blockIdx.y;
    if (threadIdx.x != 0u || k > a.p.n_parts) return;                     // a stream is one lane's
    const size_t n = vp8e_mb_count(a);
    const uint8_t* probs = a.probs + static_cast<size_t>(img) * kVp8eProbBytes;
    const Vp8Mb* mbs = a.mbs + static_cast<size_t>(img) * n;
    uint32_t len;
    if (k == 0u) len = vp8e_first_partition(*a.T, a.p, probs, probs + kVp8eProbs, probs[2u * kVp8eProbs], mbs, n, vp8e_stream(a, img, 0u), a.first_cap, a.mbw);
    else len = vp8e_token_partition(*a.T, probs, mbs, a.levels + static_cast<size_t>(img) * n * kVp8MbLevels, a.mbw, a.mbh, k - 1u, a.p.n_parts, vp8e_stream(a, img, k), a.part_cap);
    a.stream_len[static_cast<size_t>(img) * kVp8eStreams + k] = len;
}

__global__ __launch_bounds__(256) void vp8e_layout_kernel(const Vp8eArgs a) {
    __shared__ Vp8eLayout L;
    __shared__ uint32_t overflowed;
    const uint32_t img = blockIdx.x, tid = threadIdx.x;
    if (tid == 0u) {
        const uint32_t* len = a.stream_len + static_cast<size_t>(img) * kVp8eStreams;
        L = Vp8eLayout{};
        L.w = a.w; L.h = a.h; L.n_parts = a.p.n_parts;
        L.alpha = a.alpha ? a.counts[static_cast<size_t>(img) * kVp8eCountWords + 2u * kVp8eProbs + 1u] : 0u;
        bool overflow = len[0] > a.first_cap || len[0] > kVp8eFirstPartMax;
        L.first_len = len[0]; L.first = vp8e_stream(a, img, 0u);
        for (uint32_t p = 0; p < L.n_parts; ++p) { L.part_len[p] = len[1u + p]; L.part[p] = vp8e_stream(a, img, 1u + p); overflow = overflow || len[1u + p] > a.part_cap; }
        if (L.alpha) {
            const uint8_t* inner = a.inner_files + static_cast<size_t>(img) * a.inner_pitch;
            if (a.inner_status[img] || a.inner_len[img] < kWebpRiff + 5u) overflow = true;       // (cannot happen under the inner stage's own pitch)
            else {
                const uint32_t payload = static_cast<uint32_t>(inner[16]) | inner[17] << 8 | inner[18] << 16 | static_cast<uint32_t>(inner[19]) << 24;
                L.alph_len = 1u + payload - 5u;
                L.alph_stream = inner + kWebpRiff + 5u;
            }
        }
        if (!overflow) { vp8e_layout_sizes(L); overflow = L.file_len > a.file_pitch; }
        overflowed = overflow ? 1u : 0u;
        a.lengths[img] = overflow ? 0u : L.file_len;
        if (a.status_out) a.status_out[img] = overflow ? kVp8eFileOverflow : 0u;
    }
    __syncthreads();
    if (overflowed) return;                                               // (uniform) nothing of this image's file is written
    // the aligned dwords that touch the image's file_pitch bytes; a dword that reaches beyond them is stored byte by byte
    const uintptr_t base = reinterpret_cast<uintptr_t>(a.files) + static_cast<size_t>(img) * a.file_pitch, end = base + a.file_pitch;
    const uintptr_t first = base & ~static_cast<uintptr_t>(3);
    for (uintptr_t at = first + 4u * static_cast<uintptr_t>(tid); at < end; at += 1024u) {
        if (at >= base && at + 4u <= end) {
            const uint32_t i = static_cast<uint32_t>(at - base);
            *reinterpret_cast<uint32_t*>(at) = vp8e_file_byte(L, i) | vp8e_file_byte(L, i + 1u) << 8 | vp8e_file_byte(L, i + 2u) << 16 | vp8e_file_byte(L, i + 3u) << 24;
        } else {
            for (uint32_t k = 0; k < 4u; ++k)
                if (at + k >= base && at + k < end) *reinterpret_cast<uint8_t*>(at + k) = static_cast<uint8_t>(vp8e_file_byte(L, static_cast<uint32_t>(at + k - base)));
        }
    }
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_webp_lossy_enc_stage {
    uint32_t width = 0, height = 0, alpha = 0, max_images = 0, mbw = 0, mbh = 0, flags = 0;
    ifhip_webp_enc_stage* inner = nullptr;       // the lossless coder of the alpha planes
    size_t inner_pitch = 0, stream_pitch = 0;
    uint32_t first_cap = 0, part_cap = 0;
    Vp8eTables* d_tables = nullptr;
    uint8_t *d_planes = nullptr, *d_probs = nullptr, *d_streams = nullptr, *d_inner_files = nullptr;
    uint32_t *d_grey = nullptr, *d_counts = nullptr, *d_stream_len = nullptr, *d_inner_len = nullptr;
    Vp8Mb* d_mbs = nullptr;
    int16_t* d_levels = nullptr;
    StageScratch blocks{&d_tables, &d_planes, &d_probs, &d_streams, &d_inner_files, &d_grey, &d_counts, &d_stream_len, &d_inner_len, &d_mbs, &d_levels};
    ~ifhip_webp_lossy_enc_stage() { ifhip_webp_enc_stage_destroy(inner); }
    int allocate() {                    // (the first batch does it, behind the argument checks)
        const size_t n = max_images, mbs = static_cast<size_t>(mbw) * mbh;
        return blocks.ensure([&]() -> int {
            HIP_TRY(DEV_MALLOC(&d_tables, sizeof(Vp8eTables)));
            HIP_TRY(hipMemcpy(d_tables, &vp8e_host_tables(), sizeof(Vp8eTables), hipMemcpyHostToDevice));
            HIP_TRY(DEV_MALLOC(&d_planes, n * mbs * 768u));
            HIP_TRY(DEV_MALLOC(&d_mbs, n * mbs * sizeof(Vp8Mb)));
            HIP_TRY(DEV_MALLOC(&d_levels, n * mbs * kVp8MbLevels * sizeof(int16_t)));
            HIP_TRY(DEV_MALLOC(&d_counts, n * kVp8eCountWords * sizeof(uint32_t)));
            HIP_TRY(DEV_MALLOC(&d_probs, n * kVp8eProbBytes));
            HIP_TRY(DEV_MALLOC(&d_streams, n * stream_pitch));
            HIP_TRY(DEV_MALLOC(&d_stream_len, n * kVp8eStreams * sizeof(uint32_t)));
            if (alpha) {
                HIP_TRY(DEV_MALLOC(&d_grey, n * width * height * sizeof(uint32_t)));
                HIP_TRY(DEV_MALLOC(&d_inner_files, n * inner_pitch));
                HIP_TRY(DEV_MALLOC(&d_inner_len, n * 2u * sizeof(uint32_t)));
            }
            return IFHIP_OK;
        });
    }
};

extern "C" {

int ifhip_webp_lossy_enc_stage_create(ifhip_webp_lossy_enc_stage** stage, uint32_t width, uint32_t height, int alpha_meaningful, uint32_t max_images) {
    return ifhip_webp_lossy_enc_stage_create_flags(stage, width, height, alpha_meaningful, max_images, 0u);
}

int ifhip_webp_lossy_enc_stage_create_flags(ifhip_webp_lossy_enc_stage** stage, uint32_t width, uint32_t height, int alpha_meaningful, uint32_t max_images, uint32_t flags) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage out-pointer");
    *stage = nullptr;
    if (flags & ~static_cast<uint32_t>(IFHIP_VP8_ENC_INTRA4)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: unknown lossy WebP coder flags 0x%x", flags);
    if (width == 0 || height == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (width > kVp8eMaxDim || height > kVp8eMaxDim)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a WebP frame is at most %u x %u (14 bits each), not %u x %u", kVp8eMaxDim, kVp8eMaxDim, width, height);
    if (max_images == 0 || max_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 images per stage");
    std::unique_ptr<ifhip_webp_lossy_enc_stage> s(new ifhip_webp_lossy_enc_stage);
    s->width = width; s->height = height; s->alpha = alpha_meaningful ? 1u : 0u; s->max_images = max_images; s->flags = flags;
    s->mbw = (width + 15u) / 16u; s->mbh = (height + 15u) / 16u;
    const uint64_t mbs = static_cast<uint64_t>(s->mbw) * s->mbh;
    const uint64_t first = vp8e_first_cap(mbs, flags), part = vp8e_part_cap(s->mbw, s->mbh, 1u << vp8e_partitions_log2(s->mbh));
    s->first_cap = static_cast<uint32_t>(((first > kVp8eFirstPartMax ? kVp8eFirstPartMax : first) + 15u) & ~15ull);
    s->part_cap = static_cast<uint32_t>((part + 15u) & ~15ull);           // (at most 2^20 macroblocks of 2664 bytes: below 2^32)
    s->stream_pitch = s->first_cap + (static_cast<size_t>(s->part_cap) << vp8e_partitions_log2(s->mbh));
    if (s->alpha) {
        if (int rc = ifhip_webp_enc_stage_create(&s->inner, width, height, 0, max_images)) return rc;
        s->inner_pitch = (ifhip_webp_enc_stage_max_file_bytes(s->inner) + 15u) & ~static_cast<size_t>(15u);
    }
    *stage = s.release();
    return IFHIP_OK;
}

void ifhip_webp_lossy_enc_stage_destroy(ifhip_webp_lossy_enc_stage* stage) { delete stage; }

size_t ifhip_webp_lossy_enc_stage_max_file_bytes(const ifhip_webp_lossy_enc_stage* stage) {
    if (!stage) return 0u;
    return static_cast<size_t>(vp8e_max_file_bytes(stage->width, stage->height, stage->alpha ? webp_max_file_bytes(stage->width, stage->height) : 0u, stage->flags));
}

int ifhip_webp_lossy_encode_batch_device(ifhip_webp_lossy_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, uint32_t n_images, float quality,
                                         uint8_t* d_files, size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status, void* hip_stream) {
    bool go = false;
    if (int rc = open_encode_batch(stage, d_images, image_bytes, stride, n_images, d_files, d_lengths, &go); rc || !go) return rc;
    if (!(quality == quality)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: quality is not a number");
    if (file_pitch < 32u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: file_pitch below %u bytes", 32u);
    if (int rc = stage->allocate()) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Vp8eArgs a{};
    a.images = d_images; a.image_bytes = image_bytes; a.stride = stride; a.w = stage->width; a.h = stage->height; a.mbw = stage->mbw; a.mbh = stage->mbh;
    a.alpha = stage->alpha; a.n_images = n_images; a.flags = stage->flags;
    a.p = vp8e_params(vp8e_host_tables(), vp8e_quality_to_index(quality), stage->mbh, kVp8eFilterNum);
    a.T = stage->d_tables; a.planes = stage->d_planes; a.grey = stage->d_grey; a.mbs = stage->d_mbs; a.levels = stage->d_levels; a.counts = stage->d_counts;
    a.probs = stage->d_probs; a.streams = stage->d_streams; a.stream_pitch = stage->stream_pitch; a.first_cap = stage->first_cap; a.part_cap = stage->part_cap;
    a.stream_len = stage->d_stream_len; a.inner_files = stage->d_inner_files; a.inner_pitch = stage->inner_pitch; a.inner_len = stage->d_inner_len;
    a.inner_status = stage->d_inner_len ? stage->d_inner_len + stage->max_images : nullptr;
    a.files = d_files; a.file_pitch = file_pitch; a.lengths = d_lengths; a.status_out = d_status;
    const uint64_t mbs = static_cast<uint64_t>(stage->mbw) * stage->mbh;
    const char* stop = debug_switch("vp8_encode_stop_after");     // tools/bench_webp_lossy_encode.py: the kernels' times by difference
    auto stops = [&](const char* name) { return stop && std::strcmp(stop, name) == 0; };
    HIP_TRY(hipMemsetAsync(stage->d_counts, 0, static_cast<size_t>(n_images) * kVp8eCountWords * sizeof(uint32_t), st));
    hipLaunchKernelGGL(vp8e_convert_kernel, dim3(static_cast<uint32_t>((mbs * 64u + 255u) / 256u), n_images), dim3(256), 0, st, a);
    if (stops("convert")) { HIP_TRY(hipGetLastError()); return IFHIP_OK; }
    if (stage->alpha)
        if (int rc = ifhip_webp_encode_batch_device(stage->inner, reinterpret_cast<const uint8_t*>(stage->d_grey), static_cast<size_t>(stage->width) * stage->height * 4u,
                                                    stage->width * 4u, n_images, stage->d_inner_files, stage->inner_pitch, stage->d_inner_len,
                                                    stage->d_inner_len + stage->max_images, hip_stream)) return rc;
    if (stops("alpha")) { HIP_TRY(hipGetLastError()); return IFHIP_OK; }
    if (stage->flags & kVp8eIntra4) vp8e_launch_code4(a, st);
    else hipLaunchKernelGGL(vp8e_code_kernel, dim3(n_images), dim3(64u * kVp8eWaves), 0, st, a);
    if (stops("code")) { HIP_TRY(hipGetLastError()); return IFHIP_OK; }
    hipLaunchKernelGGL(vp8e_count_kernel, dim3(static_cast<uint32_t>((mbs + 255u) / 256u), n_images), dim3(256), 0, st, a);
    hipLaunchKernelGGL(vp8e_decide_kernel, dim3(n_images), dim3(64), 0, st, a);
    if (stops("decide")) { HIP_TRY(hipGetLastError()); return IFHIP_OK; }
    hipLaunchKernelGGL(vp8e_streams_kernel, dim3(kVp8eStreams, n_images), dim3(64), 0, st, a);
    if (stops("streams")) { HIP_TRY(hipGetLastError()); return IFHIP_OK; }
    hipLaunchKernelGGL(vp8e_layout_kernel, dim3(n_images), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_webp_lossy_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful, float quality, uint8_t* out, size_t capacity,
                            size_t* len) {
    return ifhip_webp_lossy_encode_flags(bgra, width, height, stride, alpha_meaningful, quality, 0u, out, capacity, len);
}

int ifhip_webp_lossy_encode_flags(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful, float quality, uint32_t flags, uint8_t* out,
                                  size_t capacity, size_t* len) {
    uint32_t status = 0;
    if (int rc = encode_host_frame(
            bgra, width, height, stride, out, capacity, len, &status,
            [&](ifhip_webp_lossy_enc_stage** s) { return ifhip_webp_lossy_enc_stage_create_flags(s, width, height, alpha_meaningful, 1, flags); }, ifhip_webp_lossy_enc_stage_destroy,
            ifhip_webp_lossy_enc_stage_max_file_bytes, [&](ifhip_webp_lossy_enc_stage* s, const HostFrame& f, size_t pitch, uint32_t* d_len) {
                return ifhip_webp_lossy_encode_batch_device(s, f.d, f.image_bytes, stride, 1, quality, f.side_output(), pitch, d_len, d_len + 1, nullptr);
            })) return rc;
    return refuse_unfitted_file(status, *len);
}

}  // extern "C"
