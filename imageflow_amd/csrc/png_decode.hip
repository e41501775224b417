// png_decode.hip -- gfx950 kernels + C ABI of the device PNG decoder: PNG files (host) -> BGRA frames in HBM.
//
// Replaces what LibPngDecoder runs on the host (codecs/libpng_decoder.rs:82-104,297-299 -> c_components/lib/
// codec_png_wrapper.c:131-246): zlib's inflate, libpng's row un-filtering, its transforms and the Adam7 scatter.  The host
// keeps the chunk walk (csrc/png_read.cpp); the gathered IDAT stream and a small descriptor per file go to the device.
// Three launches per batch, every file of the batch in each; files of one batch may differ in size, type and depth.
//
//   png_inflate_kernel   ONE WAVE PER STREAM.  Standard deflate is serial per stream: every code's position depends on all
//                        codes before it.  The parallelism of this stage is across the files of a batch (the chip has more than a
//                        thousand wave slots); inside a stream only the table build, the input staging, the copies
//                        (matches, stored blocks) and the flush with its checksum sums are wave-wide.  Everything else is
//                        wave-uniform code.  The 32 KiB window is an LDS ring: a wave's LDS accesses are performed in
//                        program order, so a byte a lane wrote is what another lane's later load sees, and no memory scope
//                        beyond the workgroup's barrier is involved; the ring's new bytes go to HBM in 16-byte stores.
//   png_unfilter_kernel  a skewed wavefront: lane r takes row y0 + r of a 64-row band and runs one pixel behind lane r - 1;
//                        `b` is what the upper lane produced in the previous step (a lane shift), `c` the lane's previous
//                        `b`, `a` its own previous result.  Only the band's first row reads the row above from HBM (the
//                        previous band's last row: the same wave wrote it, a workgroup-scope fence stands between).  A band
//                        costs w + 63 steps instead of 64 * w; every filter type goes through the same schedule.  For Adam7
//                        the schedule runs per pass on that pass's sub-image.  One wave per image, looping over the bands.
//   png_expand_kernel    un-filtered samples -> BGRA rows of the frame: element-wise, a thread per destination pixel
//                        (coalesced dword stores, the stride honoured, padding untouched), the palette and tRNS from a
//                        per-file table, the Adam7 scatter by the destination pixel's pass coordinates.  Kept apart from
//                        the un-filter: that one is latency-bound on one wave, this one is bandwidth-bound on the chip.
// Every rule with a bit in it lives in png_decode_core.hpp, shared with the CPU emulation of the tests
// (tests/png_decode_emulate.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include "decode_handoff.hpp"
#include "png_decode_core.hpp"
#include "png_read.hpp"

namespace ifhip {

struct PngFile {
    uint64_t stream_off, inflated_off;   // into the batch's block, multiples of 16
    uint8_t* frame;
    uint32_t stream_len, inflated;
    uint32_t w, h, stride;
    uint32_t color_type, depth, interlace, has_trns, key[3];
    uint32_t palette;                    // index of the file's 256-entry table (palette files), else 0
    uint32_t preset_status;              // non-zero: the host refused the file; nothing runs for it
};
struct PngDecArgs {
    const PngFile* files;
    const uint32_t* palettes;
    uint8_t* block;
    uint32_t* status;
    uint32_t n_files;
};

struct WaveExec {
    uint32_t lane;
    template <typename F> __device__ __forceinline__ void lanes(F f) { __syncthreads(); f(lane); __syncthreads(); }
    template <typename F> __device__ __forceinline__ void one(F f) { if (lane == 0u) f(); }
    __device__ __forceinline__ void sync() { __syncthreads(); }
};

// ---- inflate: one wave per stream ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void png_inflate_kernel(const PngDecArgs a) {
    __shared__ PngInflateLds S;
    const PngFile& f = a.files[blockIdx.x];
    WaveExec x{threadIdx.x};
    uint32_t status = f.preset_status;
    if (status == kPngDecOk) status = png_inflate(x, S, a.block + f.stream_off, f.stream_len, a.block + f.inflated_off, f.inflated).status;
    if (threadIdx.x == 0u) a.status[blockIdx.x] = status;
}

// ---- un-filter: a skewed wavefront over bands of 64 rows, one wave per image ------------------------------------------------------
__device__ __forceinline__ uint64_t lane_shift_up(uint64_t v) {
    const uint32_t lo = __shfl_up(static_cast<uint32_t>(v), 1, 64), hi = __shfl_up(static_cast<uint32_t>(v >> 32), 1, 64);
    return static_cast<uint64_t>(hi) << 32 | lo;
}
// one (sub-)image in place; returns true when a row's filter type is above 4 (on the lanes that met it)
__device__ __forceinline__ bool png_unfilter_image(uint8_t* base, uint32_t w, uint32_t h, uint32_t ct, uint32_t depth, uint32_t lane) {
    const uint32_t bpp = png_filter_bpp(ct, depth), rb = static_cast<uint32_t>(png_row_bytes(w, ct, depth)), pitch = rb + 1u, units = rb / bpp;
    bool bad = false;
    for (uint32_t y0 = 0; y0 < h; y0 += 64u) {
        const uint32_t y = y0 + lane;
        const bool active = y < h;
        uint8_t* row = base + static_cast<size_t>(active ? y : 0u) * pitch + 1u;
        uint32_t ft = active ? row[-1] : 0u;
        if (ft > 4u) { bad = true; ft = 0u; }
        uint64_t pa = 0, pc = 0, prod = 0;
        uint64_t raw = active && lane == 0u ? png_load_pixel(row, bpp) : 0u;              // the pixel of the lane's next step, loaded a step ahead
        for (uint32_t t = 0; t < units + 63u; ++t) {
            const uint64_t up = lane_shift_up(prod);                                       // every lane, every step
            const uint32_t px = t - lane;
            const bool on = active && t >= lane && px < units;
            const bool next_on = active && t + 1u >= lane && px + 1u < units;
            uint64_t next = 0;
            if (next_on) next = png_load_pixel(row + static_cast<size_t>(px + 1u) * bpp, bpp);   // (never written before its owner reads it)
            if (on) {
                const uint64_t pb = lane ? up : y ? png_load_pixel(row - pitch + static_cast<size_t>(px) * bpp, bpp) : 0u;
                const uint64_t v = png_unfilter_pixel(ft, raw, pa, pb, pc, bpp);
                png_store_pixel(row + static_cast<size_t>(px) * bpp, v, bpp);
                pa = v; pc = pb; prod = v;
            }
            raw = next;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // the band's last row, before the next band's first lane reads it
        __syncthreads();
    }
    return bad;
}
__global__ __launch_bounds__(64) void png_unfilter_kernel(const PngDecArgs a) {
    const PngFile& f = a.files[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    if (a.status[blockIdx.x] != kPngDecOk) return;               // (uniform)
    uint8_t* data = a.block + f.inflated_off;
    bool bad = false;
    if (!f.interlace) {
        bad = png_unfilter_image(data, f.w, f.h, f.color_type, f.depth, lane);
    } else {
        size_t off = 0;
        for (uint32_t p = 0; p < 7u; ++p) {
            const uint32_t pw = png_pass_width(f.w, p), ph = png_pass_height(f.h, p);
            if (!pw || !ph) continue;
            bad |= png_unfilter_image(data + off, pw, ph, f.color_type, f.depth, lane);
            off += png_image_bytes(pw, ph, f.color_type, f.depth);
        }
    }
    if (bad) a.status[blockIdx.x] = kPngDecFilter;               // (every lane that met one stores the same word)
}

// ---- expand: a thread per destination pixel ---------------------------------------------------------------------------------------------
// (The grid is sized by the batch's largest image: blocks past a smaller file's last pixel leave at once, every thread pays a
// 64-bit divide and an interlaced pixel re-sums its pass's offset.  All of it is noise next to the inflate in front, DESIGN 6;
// a per-file block table and per-pass offsets in the descriptor are what to do if this stage ever shows.)
__global__ __launch_bounds__(256) void png_expand_kernel(const PngDecArgs a) {
    const PngFile& f = a.files[blockIdx.y];
    if (a.status[blockIdx.y] != kPngDecOk) return;               // (uniform: a damaged file leaves its frame untouched)
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= static_cast<uint64_t>(f.w) * f.h) return;
    const uint32_t y = static_cast<uint32_t>(i / f.w), x = static_cast<uint32_t>(i - static_cast<uint64_t>(y) * f.w);
    const uint8_t* data = a.block + f.inflated_off;
    const uint8_t* row;
    uint32_t px = x;
    if (f.interlace) {
        const uint32_t p = png_pass_of(x, y);
        size_t off = 0;
        for (uint32_t q = 0; q < p; ++q) off += png_image_bytes(png_pass_width(f.w, q), png_pass_height(f.h, q), f.color_type, f.depth);
        px = (x - png_pass_x0(p)) / png_pass_dx(p);
        row = data + off + static_cast<size_t>((y - png_pass_y0(p)) / png_pass_dy(p)) * (1u + png_row_bytes(png_pass_width(f.w, p), f.color_type, f.depth)) + 1u;
    } else {
        row = data + static_cast<size_t>(y) * (1u + png_row_bytes(f.w, f.color_type, f.depth)) + 1u;
    }
    const PngExpand e = {f.color_type, f.depth, f.has_trns, {f.key[0], f.key[1], f.key[2]}};
    const uint32_t v = png_expand_pixel(e, a.palettes + static_cast<size_t>(f.palette) * 256u, row, px);
    *reinterpret_cast<uint32_t*>(f.frame + static_cast<size_t>(y) * f.stride + 4u * static_cast<size_t>(x)) = v;
}

const char* png_status_text(uint32_t s) {
    switch (s) {
    case kPngDecTruncated: return "Not enough image data (the zlib stream ends early)";
    case kPngDecBlockType: return "invalid block type";
    case kPngDecStoredLength: return "invalid stored block lengths";
    case kPngDecCodeLengths: return "invalid code lengths set";
    case kPngDecBadCode: return "invalid literal/length or distance code";
    case kPngDecDistance: return "invalid distance too far back";
    case kPngDecZlibHeader: return "incorrect header check";
    case kPngDecAdler: return "incorrect data check";
    case kPngDecTooLittle: return "Not enough image data";
    case kPngDecFilter: return "bad adaptive filter value";
    default: return "the file's chunks did not parse";
    }
}


// The device part of a batch whose files the host has walked already (parse_png with gather): parsed[i] == nullptr is a file
// whose chunks did not parse.  What depends on the FILE is that file's status word (IFHIP_PNG_DEC_CONTAINER also for an image
// that would inflate beyond 2^31 bytes); what depends on the CALLER's arguments -- the frames -- fails the call.
int png_decode_parsed_device(const PngParsed* const* parsed, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                             const uint32_t* strides, uint32_t* d_status, void* hip_stream) {
    std::vector<PngFile> desc(n_files);
    uint32_t n_palettes = 1;                                      // table 0: what files without a palette point at
    size_t blob = 0, inflated_total = 0;
    uint64_t max_pixels = 1;
    for (uint32_t i = 0; i < n_files; ++i) {
        PngFile& f = desc[i];
        std::memset(&f, 0, sizeof f);
        if (!parsed[i] || parsed[i]->inflated > 0x7FFF0000ull) { f.preset_status = IFHIP_PNG_DEC_CONTAINER; continue; }
        const PngParsed& P = *parsed[i];
        if (int rc = check_frames(d_frames[i], frame_bytes[i], P.w, P.h, strides[i], "frame")) return rc;
        f.frame = d_frames[i]; f.stream_len = static_cast<uint32_t>(P.idat_len); f.inflated = static_cast<uint32_t>(P.inflated);
        f.w = P.w; f.h = P.h; f.stride = strides[i]; f.color_type = P.color_type; f.depth = P.depth; f.interlace = P.interlace;
        f.has_trns = P.has_trns; f.key[0] = P.key[0]; f.key[1] = P.key[1]; f.key[2] = P.key[2];
        if (P.color_type == 3u) f.palette = n_palettes++;
        max_pixels = std::max<uint64_t>(max_pixels, static_cast<uint64_t>(P.w) * P.h);
    }
    if (max_pixels > 256ull * 0x7FFFFFFFull) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a frame of %llu pixels exceeds the launch grid", static_cast<unsigned long long>(max_pixels));
    // the block: descriptors, palette tables, the streams (what is uploaded), then the inflated images
    const size_t desc_bytes = pad16(sizeof(PngFile) * n_files), pal_bytes = static_cast<size_t>(n_palettes) * 1024u;
    blob = desc_bytes + pal_bytes;
    for (uint32_t i = 0; i < n_files; ++i) if (!desc[i].preset_status) { desc[i].stream_off = blob; blob += pad16(parsed[i]->idat_len); }
    for (uint32_t i = 0; i < n_files; ++i)
        if (!desc[i].preset_status) { desc[i].inflated_off = blob + inflated_total; inflated_total += pad16(desc[i].inflated); }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StagedBlock staged(st);
    if (int rc = staged.alloc(blob + inflated_total, blob)) return rc;
    uint8_t* const block = staged.block;
    uint8_t* const host = staged.host;
    std::memset(host, 0, desc_bytes + pal_bytes);
    std::memcpy(host, desc.data(), sizeof(PngFile) * n_files);
    uint32_t* pal = reinterpret_cast<uint32_t*>(host + desc_bytes);
    for (uint32_t i = 0; i < n_files; ++i) {
        if (desc[i].preset_status) continue;
        if (desc[i].palette) std::memcpy(pal + static_cast<size_t>(desc[i].palette) * 256u, parsed[i]->palette, 1024);
        uint8_t* at = host + desc[i].stream_off;                     // the IDAT payloads become one stream here, padded with zeros to 16 bytes
        for (const auto& c : parsed[i]->idat) { std::memcpy(at, c.first, c.second); at += c.second; }
        std::memset(at, 0, (0u - parsed[i]->idat_len) & 15u);
    }
    if (int rc = staged.send()) return rc;
    PngDecArgs a;
    a.files = reinterpret_cast<const PngFile*>(block); a.palettes = reinterpret_cast<const uint32_t*>(block + desc_bytes); a.block = block;
    a.status = d_status; a.n_files = n_files;
    const char* stop = debug_switch("png_decode_stop_after");     // tools/bench_png_decode.py: the stages' times by difference
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n_files), dim3(64), 0, st, a);
    if (!stop || std::strcmp(stop, "inflate") != 0) {
        hipLaunchKernelGGL(png_unfilter_kernel, dim3(n_files), dim3(64), 0, st, a);
        if (!stop || std::strcmp(stop, "unfilter") != 0)
            hipLaunchKernelGGL(png_expand_kernel, dim3(static_cast<uint32_t>((max_pixels + 255u) / 256u), n_files), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_png_decode_batch_device(const uint8_t* const* files, const size_t* lens, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                                  const uint32_t* strides, uint32_t* d_status, void* hip_stream) {
    if (n_files == 0) return IFHIP_OK;
    std::vector<PngParsed> parsed;
    std::vector<const PngParsed*> ok;
    auto parse = [](const uint8_t* file, size_t len, uint32_t, PngParsed* P) { return parse_png(file, len, P, true) == IFHIP_OK; };
    if (int rc = walk_decode_batch(files, lens, n_files, d_frames, frame_bytes, strides, d_status, &parsed, &ok, parse)) return rc;
    return png_decode_parsed_device(ok.data(), n_files, d_frames, frame_bytes, strides, d_status, hip_stream);
}

int ifhip_png_decode(const uint8_t* png, size_t len, uint8_t* bgra, uint32_t stride, size_t capacity, uint32_t* status) {
    uint32_t word = 0;
    if (!status) status = &word;
    *status = 0;
    if (!png) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    PngParsed P;
    if (int rc = parse_png(png, len, &P, true)) return rc;          // the one walk over the chunks
    if (int rc = check_decode_destination(bgra, P.w, P.h, stride, capacity)) return rc;
    const PngParsed* parsed = &P;
    auto device = [&](uint8_t* frame, size_t bytes, uint32_t at_stride, uint32_t* d_status) { return png_decode_parsed_device(&parsed, 1, &frame, &bytes, &at_stride, d_status, nullptr); };
    if (int rc = decode_to_host_frame(P.w, P.h, bgra, stride, device, status)) return rc;
    if (*status) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: LibPNG error: %s", png_status_text(*status));
    return IFHIP_OK;
}

}  // extern "C"
