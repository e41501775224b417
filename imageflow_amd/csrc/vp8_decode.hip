// vp8_decode.hip -- gfx950 kernels + C ABI of the device lossy WebP decoder: still lossy WebP files (host) -> BGRA frames in HBM.
//
// Replaces what WebPDecoder runs on the host for a `VP8 ` (+ `ALPH`) file (imageflow_core/src/codecs/webp.rs:162-248 ->
// WebPDecode into MODE_BGRA).  The shape of the progressive-JPEG path: what is serial by construction -- the bool decoder
// behind the header, the modes and the coefficient tokens -- is the host's (csrc/vp8_read.cpp), everything that touches a
// pixel runs here.  Up go each macroblock's record and its un-dequantised levels (dense: 800 B a macroblock) and the ALPH
// payload.  A batch of files of any mix of sizes runs five launches, every file in each, plus the VP8L reader's for the
// files whose alpha plane is VP8L-coded:
//
//   vp8_residual_kernel     grid-wide, a thread per 4x4 block of every file: dequantise, the inverse WHT's output for the
//                           luma blocks of a 16x16-mode macroblock, the inverse DCT (a constant for a DC-only block);
//                           the residuals take the levels' place.
//   vp8_predict_kernel      ONE WORKGROUP OF 16 WAVES PER FILE: intra prediction plus residual into Y/U/V planes of whole
//                           macroblocks, from UNFILTERED neighbours.  Macroblock (x, y) needs (x-1, y), (x, y-1), (x-1, y-1)
//                           and (x+1, y-1): a wavefront of skew 2, macroblock (x, y) in step x + 2y, the macroblocks of a
//                           step dealt to the waves, a workgroup barrier between steps.  The pixels of a whole-macroblock
//                           mode and of chroma are spread over the wave's lanes; the sixteen sub-blocks of a 4x4-mode
//                           macroblock are lane 0's, in raster order (a thread's own stores and loads need no fence).
//   vp8_loop_filter_kernel  the same wavefront, in place: raster macroblock order asks (x-1, y), (x, y-1) and (x+1, y-1) --
//                           whose left edge rewrites columns this macroblock's top edge reads -- to be complete.  Within a
//                           step every macroblock's rows (left edge, inner vertical edges: a lane a row) come before every
//                           macroblock's columns (top edge, inner horizontal edges), a barrier between.  Files with level
//                           0 leave at once.
//   vp8_alpha_kernel        one wave per file: settles the file's status word (the VP8L reader's verdict on the alpha
//                           stream comes in here), then un-filters the coded bytes -- the green of the VP8L plane or the
//                           raw bytes -- into the alpha plane.  Row 0 and column 0 are prefix sums mod 256 (wave scans);
//                           behind them horizontal is a lane per row, vertical a lane per column, gradient a skewed
//                           wavefront over bands of 64 rows with the upper neighbours handed down by a lane shift, as the
//                           VP8L predictor and the PNG un-filter do.
//   vp8_to_bgra_kernel      grid-wide, a thread per pixel: fancy chroma upsampling, YUV -> BGR, alpha from the plane or 255;
//                           4 * w bytes a row at the caller's stride, the padding untouched.  Only a file whose status
//                           word is 0 is written: a damaged file gets its word and nothing else.
// No wave ever waits for another by polling: steps are separated by workgroup barriers or lane shifts only.
// Every rule with a bit in it lives in vp8_decode_core.hpp, shared with the CPU emulation (tests/vp8_decode_emulate.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/imageflow_hip_webp_lossy.h"
#include "decode_handoff.hpp"
#include "vp8_decode_core.hpp"
#include "vp8_read.hpp"
#include "webp_decode_core.hpp"
#include "webp_read.hpp"

namespace ifhip {

struct Vp8File {
    uint64_t mb_off, levels_off, raw_off;        // uploaded; into the batch's block, multiples of 16
    uint64_t y_off, u_off, v_off, alpha_off, argb_off;
    uint8_t* frame;
    uint32_t w, h, stride, mbw, mbh;
    uint32_t filter, alpha_kind, alpha_filter;
    uint32_t alpha_index;                        // kVp8AlphaVp8l: which word of the VP8L reader's status words
    uint32_t preset_status;                      // non-zero: the host refused the file; nothing runs for it
    Vp8Quant quant[4];
};
struct Vp8DecArgs {
    const Vp8File* files;
    uint8_t* block;
    uint32_t* status;
    const uint32_t* alpha_status;
    uint32_t n_files;
};
constexpr uint32_t kVp8WaveCount = 16u;          // waves of the one workgroup a file's wavefronts run in
constexpr uint32_t kVp8TilePixels = 1024u;

__device__ __forceinline__ Vp8Planes vp8_planes(const Vp8DecArgs& a, const Vp8File& f) {
    return Vp8Planes{a.block + f.y_off, a.block + f.u_off, a.block + f.v_off, f.mbw * 16u, f.mbw * 8u, f.mbw, f.mbh};
}
__device__ __forceinline__ void vp8_step_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");       // this step's pixels, before another wave's next step reads them
    __syncthreads();
}

__global__ __launch_bounds__(256) void vp8_residual_kernel(const Vp8DecArgs a) {
    const Vp8File& f = a.files[blockIdx.y];
    if (f.preset_status) return;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t m = i / 24u;
    if (m >= static_cast<uint64_t>(f.mbw) * f.mbh) return;
    const Vp8Mb& mb = reinterpret_cast<const Vp8Mb*>(a.block + f.mb_off)[m];
    vp8_residual_mb_block(reinterpret_cast<int16_t*>(a.block + f.levels_off) + m * kVp8MbLevels, mb, f.quant[mb.segment & 3u], static_cast<uint32_t>(i - m * 24u));
}

// the rows y of step s: macroblock (s - 2y, y) exists
__device__ __forceinline__ void vp8_step_rows(uint32_t s, uint32_t mbw, uint32_t mbh, uint32_t* lo, uint32_t* hi) {
    *lo = s + 1u >= mbw ? (s + 2u - mbw) / 2u : 0u;
    *hi = min(mbh - 1u, s / 2u);
}

__global__ __launch_bounds__(1024) void vp8_predict_kernel(const Vp8DecArgs a) {
    const Vp8File& f = a.files[blockIdx.x];
    if (f.preset_status) return;                                          // (uniform)
    const Vp8Planes P = vp8_planes(a, f);
    const Vp8Mb* mbs = reinterpret_cast<const Vp8Mb*>(a.block + f.mb_off);
    const int16_t* res = reinterpret_cast<const int16_t*>(a.block + f.levels_off);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t steps = f.mbw + 2u * (f.mbh - 1u);
    for (uint32_t s = 0; s < steps; ++s) {
        uint32_t lo, hi;
        vp8_step_rows(s, f.mbw, f.mbh, &lo, &hi);
        for (uint32_t y = lo + wave; y <= hi; y += kVp8WaveCount) {
            const uint32_t x = s - 2u * y;
            const size_t m = static_cast<size_t>(y) * f.mbw + x;
            vp8_predict_mb(P, mbs[m], res + m * kVp8MbLevels, x, y, lane, 64u);
        }
        vp8_step_barrier();
    }
}

__global__ __launch_bounds__(1024) void vp8_loop_filter_kernel(const Vp8DecArgs a) {
    const Vp8File& f = a.files[blockIdx.x];
    if (f.preset_status || f.filter == kVp8FilterNone) return;            // (uniform)
    const Vp8Planes P = vp8_planes(a, f);
    const Vp8Mb* mbs = reinterpret_cast<const Vp8Mb*>(a.block + f.mb_off);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t steps = f.mbw + 2u * (f.mbh - 1u);
    for (uint32_t s = 0; s < steps; ++s) {
        uint32_t lo, hi;
        vp8_step_rows(s, f.mbw, f.mbh, &lo, &hi);
        for (uint32_t pass = 0; pass < 2u; ++pass) {
            for (uint32_t y = lo + wave; y <= hi; y += kVp8WaveCount) {
                const uint32_t x = s - 2u * y;
                vp8_filter_mb_line(P, mbs[static_cast<size_t>(y) * f.mbw + x], f.filter, x, y, lane, pass != 0u);
            }
            vp8_step_barrier();
        }
    }
}

// inclusive sum over the wave's lanes, mod 256 at the caller's
__device__ __forceinline__ uint32_t vp8_wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

__global__ __launch_bounds__(64) void vp8_alpha_kernel(const Vp8DecArgs a) {
    const Vp8File& f = a.files[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint32_t status = f.preset_status;
    if (!status && f.alpha_kind == kVp8AlphaVp8l && a.alpha_status[f.alpha_index]) status = kVp8DecAlphaStream;
    if (lane == 0u) a.status[blockIdx.x] = status;
    if (status || f.alpha_kind == kVp8AlphaNone) return;                  // (uniform)
    const uint32_t w = f.w, h = f.h, filter = f.alpha_filter;
    const uint8_t* raw = a.block + f.raw_off;
    const uint32_t* argb = reinterpret_cast<const uint32_t*>(a.block + f.argb_off);
    const bool vp8l = f.alpha_kind == kVp8AlphaVp8l;
    uint8_t* out = a.block + f.alpha_off;
    auto coded = [&](size_t i) -> uint32_t { return vp8l ? (argb[i] >> 8) & 255u : raw[i]; };
    if (filter == 0u) {
        for (size_t i = lane, n = static_cast<size_t>(w) * h; i < n; i += 64u) out[i] = static_cast<uint8_t>(coded(i));
        return;
    }
    uint32_t carry = 0;
    for (uint32_t x0 = 0; x0 < w; x0 += 64u) {                            // row 0: from the left, its first pixel from 0
        const uint32_t x = x0 + lane;
        const uint32_t v = vp8_wave_scan(x < w ? coded(x) : 0u, lane) + carry;
        if (x < w) out[x] = static_cast<uint8_t>(v);
        carry = __shfl(v, 63, 64);
    }
    carry = coded(0);
    for (uint32_t y0 = 1; y0 < h; y0 += 64u) {                            // column 0: from above
        const uint32_t y = y0 + lane;
        const uint32_t v = vp8_wave_scan(y < h ? coded(static_cast<size_t>(y) * w) : 0u, lane) + carry;
        if (y < h) out[static_cast<size_t>(y) * w] = static_cast<uint8_t>(v);
        carry = __shfl(v, 63, 64);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    if (w < 2u || h < 2u) return;
    if (filter == 1u) {
        for (uint32_t y = 1u + lane; y < h; y += 64u) {
            const size_t row = static_cast<size_t>(y) * w;
            uint32_t left = out[row];
            for (uint32_t x = 1; x < w; ++x) { left = (coded(row + x) + left) & 255u; out[row + x] = static_cast<uint8_t>(left); }
        }
    } else if (filter == 2u) {
        for (uint32_t x = 1u + lane; x < w; x += 64u) {
            uint32_t top = out[x];
            for (uint32_t y = 1; y < h; ++y) { const size_t i = static_cast<size_t>(y) * w + x; top = (coded(i) + top) & 255u; out[i] = static_cast<uint8_t>(top); }
        }
    } else {
        for (uint32_t y0 = 1; y0 < h; y0 += 64u) {                        // lane r: row y0 + r, one pixel behind lane r - 1
            const uint32_t y = y0 + lane;
            const bool active = y < h;
            const size_t row = static_cast<size_t>(active ? y : 1u) * w;
            uint32_t left = out[row], tl = out[row - w], prod = 0;
            for (uint32_t t = 0; t < w - 1u + 63u; ++t) {
                const uint32_t up = __shfl_up(prod, 1, 64);               // every lane, every step
                const uint32_t px = 1u + t - lane;
                const bool on = active && t >= lane && px < w;
                uint32_t top = up;
                if (lane == 0u) top = on ? out[row - w + px] : 0u;
                if (on) {
                    const uint32_t v = (coded(row + px) + vp8_alpha_predict(3u, px, y, left, top, tl)) & 255u;
                    out[row + px] = static_cast<uint8_t>(v);
                    left = v; prod = v; tl = top;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");        // the band's last row, before the next band's first lane reads it
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void vp8_to_bgra_kernel(const Vp8DecArgs a) {
    const Vp8File& f = a.files[blockIdx.y];
    if (a.status[blockIdx.y] != kVp8DecOk) return;                        // (uniform: a damaged file leaves its frame untouched)
    const uint64_t n = static_cast<uint64_t>(f.w) * f.h, i0 = static_cast<uint64_t>(blockIdx.x) * kVp8TilePixels;
    if (i0 >= n) return;
    const Vp8Planes P = vp8_planes(a, f);
    const uint8_t* alpha = f.alpha_kind == kVp8AlphaNone ? nullptr : a.block + f.alpha_off;
    for (uint32_t j = threadIdx.x; j < kVp8TilePixels; j += 256u) {
        const uint64_t i = i0 + j;
        if (i >= n) break;
        const uint32_t y = static_cast<uint32_t>(i / f.w), x = static_cast<uint32_t>(i - static_cast<uint64_t>(y) * f.w);
        reinterpret_cast<uint32_t*>(f.frame + static_cast<size_t>(y) * f.stride)[x] = vp8_bgra_pixel(P, alpha, f.w, f.h, x, y);
    }
}

void vp8_prepare_job(const WebpParsed& parsed, Vp8Job* job) {
    job->parsed = parsed;
    job->frame = Vp8Frame();
    if (vp8_read_frame(parsed.vp8, parsed.vp8_len, &job->frame)) return;
    if (parsed.alph) (void)vp8_read_alpha(parsed.alph, parsed.alph_len, &job->frame);
}

// The device part of a batch whose files the host has walked and read: jobs[i] == nullptr is a file whose container did not
// parse.  What depends on the FILE is that file's status word; what depends on the CALLER's arguments -- the frames -- fails the call.
int vp8_decode_prepared_device(const Vp8Job* const* jobs, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                               const uint32_t* strides, uint32_t* d_status, void* hip_stream) {
    std::vector<Vp8File> desc(n_files);
    const size_t desc_bytes = pad16(sizeof(Vp8File) * n_files);
    size_t blob = desc_bytes;
    auto take = [&](size_t bytes) { const size_t at = blob; blob += pad16(bytes); return at; };
    uint64_t max_blocks = 1, max_pixels = 1;
    uint32_t n_alpha = 0;
    for (uint32_t i = 0; i < n_files; ++i) {
        Vp8File& f = desc[i];
        std::memset(&f, 0, sizeof f);
        if (!jobs[i]) { f.preset_status = IFHIP_VP8_DEC_CONTAINER; continue; }
        const Vp8Job& J = *jobs[i];
        if (J.frame.status == kVp8DecNotLossy) { f.preset_status = kVp8DecNotLossy; continue; }     // (the file gets no frame)
        if (int rc = check_frames(d_frames[i], frame_bytes[i], J.parsed.w, J.parsed.h, strides[i], "frame")) return rc;
        if (J.frame.status) { f.preset_status = J.frame.status; continue; }
        const Vp8Frame& F = J.frame;
        f.frame = d_frames[i]; f.w = F.w; f.h = F.h; f.stride = strides[i]; f.mbw = F.mbw; f.mbh = F.mbh;
        f.filter = F.filter; f.alpha_kind = F.alpha_kind; f.alpha_filter = F.alpha_filter;
        std::memcpy(f.quant, F.quant, sizeof f.quant);
        f.mb_off = take(F.mbs.size() * sizeof(Vp8Mb));
        f.levels_off = take(F.levels.size() * sizeof(int16_t));
        if (F.alpha_kind == kVp8AlphaRaw) f.raw_off = take(static_cast<size_t>(F.w) * F.h);
        if (F.alpha_kind == kVp8AlphaVp8l) f.alpha_index = n_alpha++;
        max_blocks = std::max<uint64_t>(max_blocks, static_cast<uint64_t>(F.mbs.size()) * 24u);
        max_pixels = std::max<uint64_t>(max_pixels, static_cast<uint64_t>(F.w) * F.h);
    }
    // behind what is uploaded: the three planes of whole macroblocks, the alpha plane, the VP8L reader's ARGB plane and its status words
    size_t total = blob;
    auto more = [&](size_t bytes) { const size_t at = total; total += pad16(bytes); return at; };
    for (uint32_t i = 0; i < n_files; ++i) {
        Vp8File& f = desc[i];
        if (f.preset_status) continue;
        const size_t mbs = static_cast<size_t>(f.mbw) * f.mbh;
        f.y_off = more(mbs * 256u); f.u_off = more(mbs * 64u); f.v_off = more(mbs * 64u);
        if (f.alpha_kind != kVp8AlphaNone) f.alpha_off = more(static_cast<size_t>(f.w) * f.h);
        if (f.alpha_kind == kVp8AlphaVp8l) f.argb_off = more(static_cast<size_t>(f.w) * f.h * 4u);
    }
    const size_t alpha_status_off = more(static_cast<size_t>(n_alpha) * 4u);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StagedBlock staged(st);
    if (int rc = staged.alloc(total, blob)) return rc;
    uint8_t* const block = staged.block;
    uint8_t* const host = staged.host;
    std::memset(host, 0, desc_bytes);
    std::memcpy(host, desc.data(), sizeof(Vp8File) * n_files);
    auto put = [&](size_t at, const void* p, size_t bytes) { if (bytes) std::memcpy(host + at, p, bytes); std::memset(host + at + bytes, 0, (0u - bytes) & 15u); };
    for (uint32_t i = 0; i < n_files; ++i) {
        if (desc[i].preset_status) continue;
        const Vp8Frame& F = jobs[i]->frame;
        put(desc[i].mb_off, F.mbs.data(), F.mbs.size() * sizeof(Vp8Mb));
        put(desc[i].levels_off, F.levels.data(), F.levels.size() * sizeof(int16_t));
        if (F.alpha_kind == kVp8AlphaRaw) put(desc[i].raw_off, F.alpha_data, static_cast<size_t>(F.w) * F.h);
    }
    if (int rc = staged.send()) return rc;
    if (n_alpha) {                                                        // the VP8L-coded alpha planes: the lossless reader's batch, into this block
        std::vector<WebpJob> alpha(n_alpha);
        std::vector<const WebpJob*> alpha_jobs(n_alpha);
        std::vector<uint8_t*> planes(n_alpha);
        std::vector<size_t> bytes(n_alpha);
        std::vector<uint32_t> pitch(n_alpha);
        for (uint32_t i = 0; i < n_files; ++i) {
            const Vp8File& f = desc[i];
            if (f.preset_status || f.alpha_kind != kVp8AlphaVp8l) continue;
            WebpJob& A = alpha[f.alpha_index];
            A.parsed.w = f.w; A.parsed.h = f.h; A.parsed.lossless = true; A.parsed.payload_len = jobs[i]->frame.alpha_len;
            A.prepared = jobs[i]->frame.alpha_prepared;
            A.status = 0;
            alpha_jobs[f.alpha_index] = &A;
            planes[f.alpha_index] = block + f.argb_off; bytes[f.alpha_index] = static_cast<size_t>(f.w) * f.h * 4u; pitch[f.alpha_index] = f.w * 4u;
        }
        if (int rc = webp_decode_prepared_device(alpha_jobs.data(), n_alpha, planes.data(), bytes.data(), pitch.data(), reinterpret_cast<uint32_t*>(block + alpha_status_off), hip_stream))
            return rc;
    }
    Vp8DecArgs a;
    a.files = reinterpret_cast<const Vp8File*>(block); a.block = block; a.status = d_status;
    a.alpha_status = reinterpret_cast<const uint32_t*>(block + alpha_status_off); a.n_files = n_files;
    const char* stop = debug_switch("vp8_decode_stop_after");     // tools/bench_webp_lossy_decode.py: the stages' times by difference
    auto stops = [&](const char* stage) { return stop && std::strcmp(stop, stage) == 0; };
    hipLaunchKernelGGL(vp8_residual_kernel, dim3(static_cast<uint32_t>((max_blocks + 255u) / 256u), n_files), dim3(256), 0, st, a);
    if (!stops("residual")) {
        hipLaunchKernelGGL(vp8_predict_kernel, dim3(n_files), dim3(64u * kVp8WaveCount), 0, st, a);
        if (!stops("predict")) {
            hipLaunchKernelGGL(vp8_loop_filter_kernel, dim3(n_files), dim3(64u * kVp8WaveCount), 0, st, a);
            if (!stops("filter")) {
                hipLaunchKernelGGL(vp8_alpha_kernel, dim3(n_files), dim3(64), 0, st, a);
                hipLaunchKernelGGL(vp8_to_bgra_kernel, dim3(static_cast<uint32_t>((max_pixels + kVp8TilePixels - 1u) / kVp8TilePixels), n_files), dim3(256), 0, st, a);
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_webp_lossy_decode_batch_device(const uint8_t* const* files, const size_t* lens, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                                         const uint32_t* strides, uint32_t* d_status, void* hip_stream) {
    if (n_files == 0) return IFHIP_OK;
    std::vector<Vp8Job> jobs;
    std::vector<const Vp8Job*> ok;
    auto parse = [](const uint8_t* file, size_t len, uint32_t, Vp8Job* J) {
        WebpParsed P;
        if (parse_webp(file, len, &P) != IFHIP_OK || P.animated) return false;
        if (P.lossless) { J->parsed = P; J->frame.status = kVp8DecNotLossy; return true; }
        if (parse_webp_lossy_for_decode(file, len, &P) != IFHIP_OK) return false;
        vp8_prepare_job(P, J);
        return true;
    };
    if (int rc = walk_decode_batch(files, lens, n_files, d_frames, frame_bytes, strides, d_status, &jobs, &ok, parse)) return rc;
    return vp8_decode_prepared_device(ok.data(), n_files, d_frames, frame_bytes, strides, d_status, hip_stream);
}

int ifhip_webp_lossy_decode(const uint8_t* webp, size_t len, uint8_t* bgra, uint32_t stride, size_t capacity, uint32_t* status) {
    uint32_t word = 0;
    if (!status) status = &word;
    *status = 0;
    if (!webp) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    WebpParsed P;
    if (int rc = parse_webp_lossy_for_decode(webp, len, &P)) return rc;
    if (int rc = check_decode_destination(bgra, P.w, P.h, stride, capacity)) return rc;
    Vp8Job J;
    vp8_prepare_job(P, &J);
    const Vp8Job* job = &J;
    auto device = [&](uint8_t* frame, size_t bytes, uint32_t at_stride, uint32_t* d_status) { return vp8_decode_prepared_device(&job, 1, &frame, &bytes, &at_stride, d_status, nullptr); };
    *status = J.frame.status;                                     // what the host stage finds needs no device
    if (!*status)
        if (int rc = decode_to_host_frame(P.w, P.h, bgra, stride, device, status)) return rc;
    if (*status) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: libwebp decoding error %s", vp8_status_text(*status));
    return IFHIP_OK;
}

}  // extern "C"
