// webp_decode.hip -- gfx950 kernels + C ABI of the device WebP decoder: lossless WebP files (host) -> BGRA frames in HBM.
//
// Replaces what WebPDecoder runs on the host for a VP8L file (imageflow_core/src/codecs/webp.rs:20-248 -> WebPDecode).  The
// host keeps the RIFF walk and the PREPARE of a stream (csrc/webp_read.cpp: header, transforms with their sub-images, the
// entropy image, every group's five codes as decode records -- a few percent of a file's bits, and with them the number
// of groups is known before anything is allocated); the payload, the records, the sub-images and the bit where the main
// image starts go to the device.  A batch runs 1 + (1..4) launches, every file in each; files may differ in everything.
//
//   webp_pixels_kernel     ONE WAVE PER FILE: the main image's token loop into ARGB dwords in HBM.  Wave-uniform code, like
//                          png_inflate_kernel; wave-wide are the staging of input and of a group's records into LDS, the
//                          colour cache's inserts and the copies (64 pixels a step).  The VP8L window is the whole image,
//                          so a copy reads what EARLIER TOKENS of the same wave stored to HBM: every source of a copy lies
//                          below the token's first pixel (out[p + j] = out[p - dist + (j mod dist)]), and a workgroup-scope
//                          fence stands between the earlier tokens' stores and the token's loads.  The wave is the whole
//                          workgroup, so that fence is the one the memory model asks for: the stores have left the wave
//                          (vmcnt 0) before a load is issued, and both go through the one L1 of the wave's CU.
//   webp_transform_kernel  step k applies each file's k-th inverse transform counted from the LAST, between two planes of
//                          dwords; a file's final step writes BGRA rows into the caller's frame (the ARGB dword IS the four
//                          BGRA bytes), 4 * w bytes a row, the padding untouched.  Predictor: a skewed wavefront over bands
//                          of 64 rows by block 0 of the file -- lane r takes row y0 + r and runs TWO pixels behind lane r - 1
//                          (modes 3, 5, 9, 10 read the top-right), the three upper neighbours come down by a lane shift,
//                          the band's first row reads the previous band's last row from HBM behind a fence, as the PNG
//                          un-filter does.  Cross-colour, add-green and colour indexing are element-wise and grid-wide.
// Every rule with a bit in it lives in webp_decode_core.hpp, shared with the host prepare and the CPU emulation of the
// tests (tests/webp_decode_emulate.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "decode_handoff.hpp"
#include "webp_decode_core.hpp"
#include "webp_read.hpp"

namespace ifhip {

struct WebpStep {
    uint32_t kind, bits, xsize, n;       // n: palette entries
    uint64_t data_off;                   // the tiles / the palette in the batch's block (bytes, a multiple of 16)
};
struct WebpFile {
    uint64_t stream_off, entropy_off, group_off, tables_off, plane_off[2];   // into the batch's block, multiples of 16
    uint64_t start_bit;
    uint8_t* frame;
    uint32_t stream_len;
    uint32_t w, h, stride, xsize;
    uint32_t cache_bits, prefix_bits, ent_x, has_entropy;
    uint32_t n_steps;                    // max(1, transforms): a file without transforms has one copying step
    uint32_t preset_status;              // non-zero: the host refused the file; nothing runs for it
    WebpStep step[4];                    // in the order they are applied (the file's last transform first); kind 4: copy
};
struct WebpDecArgs {
    const WebpFile* files;
    uint8_t* block;
    uint32_t* status;
    uint32_t n_files;
};
constexpr uint32_t kWebpCopyStep = 4u;
constexpr uint32_t kWebpTilePixels = 1024u;   // pixels of an element-wise step one block of 64 lanes takes

struct WebpWaveExec {
    uint32_t lane;
    template <typename F> __device__ __forceinline__ void lanes(F f) { __syncthreads(); f(lane); __syncthreads(); }
    template <typename F> __device__ __forceinline__ void one(F f) { if (lane == 0u) f(); }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __syncthreads(); }
    __device__ __forceinline__ void max64(uint64_t* p, uint64_t v) { atomicMax(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v)); }
};

// ---- the token loop: one wave per file -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void webp_pixels_kernel(const WebpDecArgs a) {
    __shared__ WebpLds S;
    const WebpFile& f = a.files[blockIdx.x];
    WebpWaveExec x{threadIdx.x};
    uint32_t status = f.preset_status;
    if (status == kWebpDecOk) {
        const WebpImage im = {f.xsize, f.h, f.cache_bits, f.prefix_bits, f.ent_x,
                              f.has_entropy ? reinterpret_cast<const uint32_t*>(a.block + f.entropy_off) : nullptr,
                              reinterpret_cast<const uint32_t*>(a.block + f.group_off), reinterpret_cast<const uint32_t*>(a.block + f.tables_off)};
        status = webp_pixels(x, S, a.block + f.stream_off, f.stream_len, f.start_bit, im, reinterpret_cast<uint32_t*>(a.block + f.plane_off[0]), nullptr);
    }
    if (threadIdx.x == 0u) a.status[blockIdx.x] = status;
}

// ---- the inverse transforms ------------------------------------------------------------------------------------------------------------
// dst: rows of `pitch` dwords (a plane: the image's width; the frame: its stride)
__device__ __forceinline__ void webp_inverse_predictor(const uint32_t* src, uint32_t* dst, size_t pitch, uint32_t w, uint32_t h, uint32_t bits, const uint32_t* tiles, uint32_t lane) {
    const uint32_t tiles_x = webp_subsample(w, bits), mask = (1u << bits) - 1u;
    for (uint32_t y0 = 0; y0 < h; y0 += 64u) {
        const uint32_t y = y0 + lane;
        const bool active = y < h;
        const uint32_t* in = src + static_cast<size_t>(active ? y : 0u) * w;
        uint32_t* out = dst + static_cast<size_t>(active ? y : 0u) * pitch;
        const uint32_t* above = out - pitch;                               // (read by lane 0 of a band behind the first only)
        const uint32_t* modes = tiles + static_cast<size_t>((active ? y : 0u) >> bits) * tiles_x;
        uint32_t prod = 0, tr = 0, tt = 0, tl = 0, left = 0, first = 0, mode = 0;
        if (lane == 0u && y0) tr = above[0];
        uint32_t raw = active && lane == 0u ? in[0] : 0u;                  // the residual of the lane's next step, loaded a step ahead
        for (uint32_t t = 0; t < w + 126u; ++t) {
            const uint32_t up = __shfl_up(prod, 1, 64);                    // every lane, every step
            const uint32_t px = t - 2u * lane;
            const bool on = active && t >= 2u * lane && px < w;
            const bool next_on = active && t + 1u >= 2u * lane && px + 1u < w;
            uint32_t next = 0, coming = up;
            if (next_on) next = in[px + 1u];
            if (lane == 0u) coming = on && y && px + 1u < w ? above[px + 1u] : 0u;
            tl = tt; tt = tr; tr = coming;
            if (on) {
                if ((px & mask) == 0u) mode = webp_tile_mode(modes[px >> bits]);
                const uint32_t v = webp_add(raw, webp_predict_at(mode, px, y, left, tt, tl, px + 1u < w ? tr : first));
                out[px] = v;
                left = v; prod = v;
                if (px == 0u) first = v;
            }
            raw = next;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // the band's last row, before the next band's first lane reads it
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void webp_transform_kernel(const WebpDecArgs a, const uint32_t k) {
    const WebpFile& f = a.files[blockIdx.y];
    if (a.status[blockIdx.y] != kWebpDecOk || k >= f.n_steps) return;     // (uniform: a damaged file leaves its frame untouched)
    const WebpStep& s = f.step[k];
    const bool last = k + 1u == f.n_steps;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.block + f.plane_off[k & 1u]);
    uint32_t* dst = last ? reinterpret_cast<uint32_t*>(f.frame) : reinterpret_cast<uint32_t*>(a.block + f.plane_off[(k + 1u) & 1u]);
    const size_t pitch = last ? f.stride / 4u : s.xsize;
    const uint32_t* data = reinterpret_cast<const uint32_t*>(a.block + s.data_off);
    if (s.kind == 0u) {
        if (blockIdx.x == 0u) webp_inverse_predictor(src, dst, pitch, s.xsize, f.h, s.bits, data, threadIdx.x);
        return;
    }
    const uint64_t n = static_cast<uint64_t>(s.xsize) * f.h, i0 = static_cast<uint64_t>(blockIdx.x) * kWebpTilePixels;
    if (i0 >= n) return;
    const uint32_t src_w = s.kind == 3u ? webp_subsample(s.xsize, s.bits) : s.xsize, tiles_x = webp_subsample(s.xsize, s.bits);
    for (uint32_t j = threadIdx.x; j < kWebpTilePixels; j += 64u) {
        const uint64_t i = i0 + j;
        if (i >= n) break;
        const uint32_t y = static_cast<uint32_t>(i / s.xsize), x = static_cast<uint32_t>(i - static_cast<uint64_t>(y) * s.xsize);
        uint32_t v;
        if (s.kind == 3u) v = webp_index_pixel(src + static_cast<size_t>(y) * src_w, x, s.bits, data, s.n);
        else {
            v = src[i];
            if (s.kind == 1u) v = webp_cross_color(v, data[static_cast<size_t>(y >> s.bits) * tiles_x + (x >> s.bits)]);
            else if (s.kind == 2u) v = webp_add_green(v);
        }
        dst[static_cast<size_t>(y) * pitch + x] = v;
    }
}

// The device part of a batch whose files the host has walked and prepared: jobs[i] == nullptr is a file whose container did
// not parse.  What depends on the FILE is that file's status word; what depends on the CALLER's arguments -- the frames --
// fails the call.
int webp_decode_prepared_device(const WebpJob* const* jobs, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                                const uint32_t* strides, uint32_t* d_status, void* hip_stream) {
    std::vector<WebpFile> desc(n_files);
    uint64_t max_pixels = 1;
    uint32_t max_steps = 1;
    const size_t desc_bytes = pad16(sizeof(WebpFile) * n_files);
    size_t blob = desc_bytes;
    auto take = [&](size_t bytes) { const size_t at = blob; blob += pad16(bytes); return at; };
    for (uint32_t i = 0; i < n_files; ++i) {
        WebpFile& f = desc[i];
        std::memset(&f, 0, sizeof f);
        if (!jobs[i]) { f.preset_status = IFHIP_WEBP_DEC_CONTAINER; continue; }
        const WebpJob& J = *jobs[i];
        if (int rc = check_frames(d_frames[i], frame_bytes[i], J.parsed.w, J.parsed.h, strides[i], "frame")) return rc;
        if (J.status) { f.preset_status = J.status; continue; }
        const WebpPrepared& P = *J.prepared;
        f.frame = d_frames[i]; f.stream_len = static_cast<uint32_t>(J.parsed.payload_len); f.start_bit = P.start_bit;
        f.w = P.w; f.h = P.h; f.stride = strides[i]; f.xsize = P.xsize;
        f.cache_bits = P.cache_bits; f.prefix_bits = P.prefix_bits; f.ent_x = P.ent_x; f.has_entropy = P.entropy.empty() ? 0u : 1u;
        f.n_steps = std::max(1u, P.n_transforms);
        f.step[0].kind = kWebpCopyStep; f.step[0].xsize = P.w;
        f.stream_off = take(J.parsed.payload_len);
        f.entropy_off = take(P.entropy.size() * 4u); f.group_off = take(P.group_off.size() * 4u); f.tables_off = take(P.tables.size() * 4u);
        for (uint32_t k = 0; k < P.n_transforms; ++k) {
            const WebpTransform& T = P.t[P.n_transforms - 1u - k];
            f.step[k].kind = T.kind; f.step[k].bits = T.bits; f.step[k].xsize = T.xsize; f.step[k].n = static_cast<uint32_t>(T.data.size());
            f.step[k].data_off = take(T.data.size() * 4u);
        }
        max_pixels = std::max<uint64_t>(max_pixels, static_cast<uint64_t>(P.w) * P.h);
        max_steps = std::max(max_steps, f.n_steps);
    }
    // behind what is uploaded: two planes of w * h dwords per file (the coded image and every intermediate one are no larger)
    size_t total = blob;
    for (uint32_t i = 0; i < n_files; ++i)
        if (!desc[i].preset_status)
            for (int p = 0; p < 2; ++p) { desc[i].plane_off[p] = total; total += pad16(static_cast<size_t>(desc[i].w) * desc[i].h * 4u); }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StagedBlock staged(st);
    if (int rc = staged.alloc(total, blob)) return rc;
    uint8_t* const block = staged.block;
    uint8_t* const host = staged.host;
    std::memset(host, 0, desc_bytes);
    std::memcpy(host, desc.data(), sizeof(WebpFile) * n_files);
    auto put = [&](size_t at, const void* p, size_t bytes) { if (bytes) std::memcpy(host + at, p, bytes); std::memset(host + at + bytes, 0, (0u - bytes) & 15u); };
    for (uint32_t i = 0; i < n_files; ++i) {
        if (desc[i].preset_status) continue;
        const WebpPrepared& P = *jobs[i]->prepared;
        put(desc[i].stream_off, P.payload.data(), jobs[i]->parsed.payload_len);
        put(desc[i].entropy_off, P.entropy.data(), P.entropy.size() * 4u);
        put(desc[i].group_off, P.group_off.data(), P.group_off.size() * 4u);
        put(desc[i].tables_off, P.tables.data(), P.tables.size() * 4u);
        for (uint32_t k = 0; k < P.n_transforms; ++k) { const WebpTransform& T = P.t[P.n_transforms - 1u - k]; put(desc[i].step[k].data_off, T.data.data(), T.data.size() * 4u); }
    }
    if (int rc = staged.send()) return rc;
    WebpDecArgs a;
    a.files = reinterpret_cast<const WebpFile*>(block); a.block = block; a.status = d_status; a.n_files = n_files;
    const char* stop = debug_switch("webp_decode_stop_after");    // tools/bench_webp_decode.py: the stages' times by difference
    hipLaunchKernelGGL(webp_pixels_kernel, dim3(n_files), dim3(64), 0, st, a);
    if (!stop || std::strcmp(stop, "pixels") != 0)
        for (uint32_t k = 0; k < max_steps; ++k)
            hipLaunchKernelGGL(webp_transform_kernel, dim3(static_cast<uint32_t>((max_pixels + kWebpTilePixels - 1u) / kWebpTilePixels), n_files), dim3(64), 0, st, a, k);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_webp_decode_batch_device(const uint8_t* const* files, const size_t* lens, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                                   const uint32_t* strides, uint32_t* d_status, void* hip_stream) {
    if (n_files == 0) return IFHIP_OK;
    std::vector<WebpJob> jobs;
    std::vector<const WebpJob*> ok;
    auto parse = [](const uint8_t* file, size_t len, uint32_t, WebpJob* J) {
        WebpParsed P;
        if (parse_webp_for_decode(file, len, &P) != IFHIP_OK) return false;
        webp_prepare_job(P, J);
        return true;
    };
    if (int rc = walk_decode_batch(files, lens, n_files, d_frames, frame_bytes, strides, d_status, &jobs, &ok, parse)) return rc;
    return webp_decode_prepared_device(ok.data(), n_files, d_frames, frame_bytes, strides, d_status, hip_stream);
}

int ifhip_webp_decode(const uint8_t* webp, size_t len, uint8_t* bgra, uint32_t stride, size_t capacity, uint32_t* status) {
    uint32_t word = 0;
    if (!status) status = &word;
    *status = 0;
    if (!webp) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    WebpJob J;
    if (int rc = parse_webp_for_decode(webp, len, &J.parsed)) return rc;
    const WebpParsed P = J.parsed;
    if (int rc = check_decode_destination(bgra, P.w, P.h, stride, capacity)) return rc;
    webp_prepare_job(P, &J);
    const WebpJob* job = &J;
    auto device = [&](uint8_t* frame, size_t bytes, uint32_t at_stride, uint32_t* d_status) { return webp_decode_prepared_device(&job, 1, &frame, &bytes, &at_stride, d_status, nullptr); };
    *status = J.status;                                           // what the host prepare finds needs no device
    if (!*status)
        if (int rc = decode_to_host_frame(P.w, P.h, bgra, stride, device, status)) return rc;
    if (*status) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: libwebp decoding error %s", webp_status_text(*status));
    return IFHIP_OK;
}

}  // extern "C"
