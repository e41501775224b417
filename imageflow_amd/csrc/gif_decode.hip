// gif_decode.hip -- gfx950 kernels + C ABI of the device GIF decoder: GIF files (host) -> the logical screen after the wanted
// frame, BGRA in HBM.
//
// Replaces what GifDecoder::read_frame runs on the host (imageflow_core/src/codecs/gif/mod.rs:207-298: the gif crate's LZW
// reader into an index buffer, then Screen::blit with Disposal, gif/screen.rs:52-94, gif/disposal.rs:29-77).  The host keeps
// the container walk (csrc/gif_read.cpp); the LZW streams, the palettes and the frames' descriptors go to the device.  A
// batch runs FIVE launches, every frame of every file in each; nothing is one serial wave per file but the hunt for clear codes:
//
//   gif_scan_kernel      ONE WAVE PER FRAME.  Between two clear codes every code's bit offset is closed-form, so 64 lanes read
//                        256 codes a step and a ballot finds the next clear or end code: segment records (start bit, codes).
//   gif_lengths_kernel   ONE WORKGROUP PER SEGMENT RECORD (grid x strides over a frame's records, grid y is the frame): the
//                        codes into LDS, every table code checked (j < k), outlen by pointer jumping, the segment's size.
//   gif_place_kernel     one workgroup per frame: the exclusive sum of its segments' sizes -- each segment's place in the
//                        frame's index buffer -- and TOO_LITTLE where the sum is below width x height.
//   gif_resolve_kernel   as the lengths kernel, then off = the workgroup scan (block_scan.hpp) of outlen and one lane per CODE
//                        writing its string from the end along the prefix chain in LDS.  A deferred clear's tail stays in
//                        its segment's own workgroup, 1024 codes a chunk against the first chunk's arrays.
//   gif_compose_kernel   one lane per SCREEN PIXEL replays dispose and blit over the frame list; BGRA rows at the caller's stride.
//   gif_compose_all_kernel   in its place where EVERY screen of a file is wanted (ifhip_gif_decode_frames_device): the same
//                        replay, once, the pixel stored into screen k behind frame k's blit -- consecutive dwords across
//                        the lanes for every k.  N screens cost one pass over the frame list, not N.
//
// Bounds: a record store is below gif_max_segments (arithmetic from the stream's length); a code read is below the
// stream's length (the scan counted only whole codes) and the staged stream carries 16 zero bytes behind it; an index store
// is below the frame's width x height (gif_write_string's cap); LDS indices are code numbers below 4096; compose reads
// index row * w + x of an inside pixel.  Every rule lives in gif_decode_core.hpp, shared with the CPU emulation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "block_scan.hpp"
#include "decode_handoff.hpp"
#include "gif_decode_core.hpp"
#include "gif_read.hpp"

namespace ifhip {

struct GifDecArgs {
    uint8_t* block;
    const GifFileDesc* files;
    const GifFrameDesc* frames;
    GifFrameState* state;
    uint32_t* status;
    uint32_t n_files, n_frames;
};

struct GifWaveExec {
    template <typename F> __device__ __forceinline__ uint64_t ballot(F f) { return __ballot(f(threadIdx.x)); }
    template <typename F> __device__ __forceinline__ void one(F f) { if (threadIdx.x == 0u) f(); }
};
struct GifBlockExec {
    uint32_t* scratch;
    template <typename F> __device__ __forceinline__ void threads(F f) { __syncthreads(); f(threadIdx.x); __syncthreads(); }
    __device__ __forceinline__ void scan(uint32_t* a, uint32_t* total) {
        const uint32_t e = block_exclusive_scan<kGifThreads>(a[threadIdx.x], scratch, total);
        __syncthreads();
        a[threadIdx.x] = e;
        __syncthreads();
    }
};

__global__ __launch_bounds__(64) void gif_scan_kernel(const GifDecArgs a) {
    const GifFrameDesc& f = a.frames[blockIdx.x];
    GifWaveExec x;
    const uint32_t n = gif_scan_frame(x, a.block + f.stream_off, f.stream_len, f.min_code, reinterpret_cast<GifSegment*>(a.block + f.seg_off), f.max_segments);
    if (threadIdx.x == 0u) a.state[blockIdx.x].n_segments = n;
}

__global__ __launch_bounds__(kGifThreads) void gif_lengths_kernel(const GifDecArgs a) {
    __shared__ GifLds S;
    const GifFrameDesc& f = a.frames[blockIdx.y];
    GifBlockExec x{S.scan_scratch};
    GifSegment* recs = reinterpret_cast<GifSegment*>(a.block + f.seg_off);
    const uint32_t n = a.state[blockIdx.y].n_segments;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        uint32_t st = 0;
        const uint32_t size = gif_segment(x, S, a.block + f.stream_off, f.min_code, recs[r], nullptr, f.n_pix, &st);
        if (threadIdx.x == 0u) {
            recs[r].size = size;
            if (st) atomicMax(&a.state[blockIdx.y].status, st);
        }
    }
}

__global__ __launch_bounds__(kGifThreads) void gif_place_kernel(const GifDecArgs a) {
    __shared__ uint32_t part[kGifThreads];
    __shared__ uint32_t scratch[kGifThreads / 64u];
    const GifFrameDesc& f = a.frames[blockIdx.x];
    if (a.state[blockIdx.x].status) return;                          // (uniform)
    struct Part { uint32_t* part; } S{part};
    GifBlockExec x{scratch};
    const uint32_t got = gif_place_segments(x, S, reinterpret_cast<const GifSegment*>(a.block + f.seg_off), a.state[blockIdx.x].n_segments,
                                            reinterpret_cast<uint32_t*>(a.block + f.place_off), f.n_pix);
    if (threadIdx.x == 0u && got < f.n_pix) a.state[blockIdx.x].status = kGifDecTooLittle;
}

__global__ __launch_bounds__(kGifThreads) void gif_resolve_kernel(const GifDecArgs a) {
    __shared__ GifLds S;
    const GifFrameDesc& f = a.frames[blockIdx.y];
    if (a.state[blockIdx.y].status) return;                          // (uniform: a damaged frame writes nothing)
    GifBlockExec x{S.scan_scratch};
    const GifSegment* recs = reinterpret_cast<const GifSegment*>(a.block + f.seg_off);
    const uint32_t* place = reinterpret_cast<const uint32_t*>(a.block + f.place_off);
    const uint32_t n = a.state[blockIdx.y].n_segments;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint32_t at = place[r];
        if (at >= f.n_pix) break;                                    // (places grow with r: nothing behind it is needed either)
        uint32_t st = 0;
        (void)gif_segment(x, S, a.block + f.stream_off, f.min_code, recs[r], a.block + f.index_off + at, f.n_pix - at, &st);
    }
}

__global__ __launch_bounds__(kGifThreads) void gif_compose_kernel(const GifDecArgs a) {
    const GifFileDesc& f = a.files[blockIdx.y];
    const uint32_t status = gif_file_status(f, a.state);
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.status[blockIdx.y] = status;
    if (status) return;                                              // (uniform: a damaged file leaves its frame untouched)
    const uint64_t n = static_cast<uint64_t>(f.w) * f.h;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kGifThreads + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * kGifThreads) {
        const uint32_t y = static_cast<uint32_t>(i / f.w), px = static_cast<uint32_t>(i - static_cast<uint64_t>(y) * f.w);
        reinterpret_cast<uint32_t*>(f.frame + static_cast<size_t>(y) * f.stride)[px] = gif_compose_pixel(f, a.frames, a.block, px, y);
    }
}

__global__ __launch_bounds__(kGifThreads) void gif_compose_all_kernel(const GifDecArgs a, const size_t screen_pitch) {
    const GifFileDesc& f = a.files[blockIdx.y];
    const uint32_t status = gif_file_status(f, a.state);
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.status[blockIdx.y] = status;
    if (status) return;                                              // (uniform: a damaged frame anywhere, and no screen is written)
    const uint64_t n = static_cast<uint64_t>(f.w) * f.h;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kGifThreads + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * kGifThreads) {
        const uint32_t y = static_cast<uint32_t>(i / f.w), px = static_cast<uint32_t>(i - static_cast<uint64_t>(y) * f.w);
        gif_compose_all_pixel(f, a.frames, a.block, px, y, screen_pitch);
    }
}

// The device part of a batch whose files the host has walked: files[i] == nullptr is a file whose header did not parse.  What
// depends on the FILE is that file's status word; what depends on the CALLER's arguments -- the frames -- fails the call.
// all_screens_pitch != 0: d_frames[i] holds every screen of file i, that far apart (the caller has checked the block).
static int gif_decode_launch(const GifParsed* const* files, uint32_t n_files, uint8_t* const* d_frames, const uint32_t* strides, uint32_t* d_status,
                             void* hip_stream, size_t all_screens_pitch) {
    GifLayout L;
    gif_layout_batch(files, n_files, d_frames, strides, &L);
    if (L.n_frames > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 65535 frames per batch at the most");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StagedBlock staged(st);
    if (int rc = staged.alloc(L.total, L.blob.size())) return rc;
    uint8_t* const block = staged.block;
    std::memcpy(staged.host, L.blob.data(), L.blob.size());           // (gif_layout_batch fills L.blob for the CPU emulation as well)
    if (int rc = staged.send()) return rc;
    GifDecArgs a;
    a.block = block; a.files = reinterpret_cast<const GifFileDesc*>(block + L.files_off); a.frames = reinterpret_cast<const GifFrameDesc*>(block + L.frames_off);
    a.state = reinterpret_cast<GifFrameState*>(block + L.state_off); a.status = d_status; a.n_files = n_files; a.n_frames = L.n_frames;
    const char* stop = debug_switch("gif_decode_stop_after");     // tools/bench_gif_decode.py: the stages' times by difference
    const bool after_scan = stop && std::strcmp(stop, "scan") == 0, after_resolve = stop && std::strcmp(stop, "resolve") == 0;
    if (L.n_frames) {
        const uint32_t seg_blocks = std::min(L.max_segments, 1024u);
        hipLaunchKernelGGL(gif_scan_kernel, dim3(L.n_frames), dim3(64), 0, st, a);
        if (!after_scan) {
            hipLaunchKernelGGL(gif_lengths_kernel, dim3(seg_blocks, L.n_frames), dim3(kGifThreads), 0, st, a);
            hipLaunchKernelGGL(gif_place_kernel, dim3(L.n_frames), dim3(kGifThreads), 0, st, a);
            hipLaunchKernelGGL(gif_resolve_kernel, dim3(seg_blocks, L.n_frames), dim3(kGifThreads), 0, st, a);
        }
    }
    if ((!after_scan && !after_resolve) || !L.n_frames) {
        const dim3 grid(std::min<uint32_t>((L.max_pixels + kGifThreads - 1u) / kGifThreads, 4096u), n_files);
        if (all_screens_pitch) hipLaunchKernelGGL(gif_compose_all_kernel, grid, dim3(kGifThreads), 0, st, a, all_screens_pitch);
        else hipLaunchKernelGGL(gif_compose_kernel, grid, dim3(kGifThreads), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int gif_decode_parsed_device(const GifParsed* const* files, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                             const uint32_t* strides, uint32_t* d_status, void* hip_stream) {
    for (uint32_t i = 0; i < n_files; ++i)
        if (files[i])
            if (int rc = check_frames(d_frames[i], frame_bytes[i], files[i]->w, files[i]->h, strides[i], "frame")) return rc;
    return gif_decode_launch(files, n_files, d_frames, strides, d_status, hip_stream, 0);
}

int gif_decode_all_parsed_device(const GifParsed& file, uint8_t* d_screens, size_t screen_pitch, uint32_t stride, uint32_t* d_status, void* hip_stream) {
    if (int rc = check_frames(d_screens, screen_pitch, file.w, file.h, stride, "screen")) return rc;
    if (!d_status) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    const GifParsed* parsed = &file;
    return gif_decode_launch(&parsed, 1, &d_screens, &stride, d_status, hip_stream, screen_pitch);
}

namespace {
int refuse(uint32_t status, uint32_t frame_index, size_t frames_seen) {
    if (status == IFHIP_GIF_DEC_NO_SUCH_FRAME)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: frame=%u requested but GIF only has %zu frames", frame_index, frames_seen);
    return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: GIF decoding error: %s", gif_status_text(status));
}
}  // namespace

}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_gif_decode_batch_device(const uint8_t* const* files, const size_t* lens, uint32_t n_files, const uint32_t* frame_index, uint8_t* const* d_frames,
                                  const size_t* frame_bytes, const uint32_t* strides, uint32_t* d_status, void* hip_stream) {
    if (n_files == 0) return IFHIP_OK;
    std::vector<GifParsed> parsed;
    std::vector<const GifParsed*> ok;
    auto parse = [&](const uint8_t* file, size_t len, uint32_t i, GifParsed* P) { return parse_gif(file, len, frame_index ? frame_index[i] : 0u, P) == IFHIP_OK && P->w && P->h; };
    if (int rc = walk_decode_batch(files, lens, n_files, d_frames, frame_bytes, strides, d_status, &parsed, &ok, parse)) return rc;
    return gif_decode_parsed_device(ok.data(), n_files, d_frames, frame_bytes, strides, d_status, hip_stream);
}

int ifhip_gif_decode_frames_device(const uint8_t* gif, size_t len, uint8_t* d_screens, size_t screen_pitch, uint32_t stride, uint32_t max_frames,
                                   uint32_t* d_status, uint32_t* n_frames_out, void* hip_stream) {
    if (!n_frames_out) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *n_frames_out = 0;
    if (!gif) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    GifParsed P;
    if (int rc = parse_gif_all(gif, len, &P)) return rc;
    if (!P.w || !P.h) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: GIF decoding error (a logical screen without pixels)");
    if (P.status) return refuse(P.status, 0u, P.frames.size());   // what the host walk finds needs no device
    if (P.frames.size() > max_frames) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: the file has %zu frames, the block holds %u screens", P.frames.size(), max_frames);
    if (int rc = gif_decode_all_parsed_device(P, d_screens, screen_pitch, stride, d_status, hip_stream)) return rc;
    // the count is promised only with the file's status: the one wait and the one word this call reads back
    uint32_t word = 0;
    HIP_TRY(hipMemcpyAsync(&word, d_status, sizeof word, hipMemcpyDeviceToHost, static_cast<hipStream_t>(hip_stream)));
    HIP_TRY(static_cast<hipError_t>(wait_stream(hip_stream)));
    if (!word) *n_frames_out = static_cast<uint32_t>(P.frames.size());
    return IFHIP_OK;
}

int ifhip_gif_decode(const uint8_t* gif, size_t len, uint32_t frame_index, uint8_t* bgra, uint32_t stride, size_t capacity, uint32_t* status) {
    uint32_t word = 0;
    if (!status) status = &word;
    *status = 0;
    if (!gif) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    GifParsed P;
    if (int rc = parse_gif(gif, len, frame_index, &P)) return rc;
    if (!P.w || !P.h) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: GIF decoding error (a logical screen without pixels)");
    if (int rc = check_decode_destination(bgra, P.w, P.h, stride, capacity)) return rc;
    const GifParsed* parsed = &P;
    auto device = [&](uint8_t* frame, size_t bytes, uint32_t at_stride, uint32_t* d_status) { return gif_decode_parsed_device(&parsed, 1, &frame, &bytes, &at_stride, d_status, nullptr); };
    *status = P.status;                                           // what the host walk finds needs no device
    if (!*status)
        if (int rc = decode_to_host_frame(P.w, P.h, bgra, stride, device, status)) return rc;
    if (*status) return refuse(*status, frame_index, P.frames.size());
    return IFHIP_OK;
}

}  // extern "C"
