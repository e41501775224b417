// png_encode.hip -- gfx950 kernels + C ABI of the device PNG coder: BGRA / BGRX frames in HBM -> complete PNG files in HBM.
//
// Replaces what EncoderPreset::Libpng runs on the host (codecs/libpng_encoder.rs:43-72,134-160 ->
// c_components/lib/codec_png_wrapper.c:349-430): libpng's row filtering with its default adaptive choice, zlib's deflate
// and the chunk framing with its CRCs.  8-bit RGB or RGBA, non-interlaced, gAMA / sRGB / cHRM in front of one IDAT.
// Launches per batch (all images in each): filter (a wave per row) into the streams of the deflate back end, its match /
// codes / layout / emit (png_deflate.hip), which write the zlib body straight into the caller's file, and finish (the
// head, and the IDAT framing of png_frame_device.hpp).  Every rule with a bit in it lives in png_encode_core.hpp (the
// construction of the prefix codes: prefix_code_core.hpp), shared with the CPU emulation of the tests (tests/png_emulate.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "encode_handoff.hpp"
#include "png_frame_device.hpp"      // (with png_deflate.hpp and png_encode_core.hpp)

namespace ifhip {

struct PngFileArgs {                    // what the coder's own two kernels take besides the deflate back end's arguments
    const uint8_t* images;
    size_t image_bytes;
    uint32_t stride, w, h, color_type, zlib_header;
    uint8_t* files;
    size_t file_pitch;
    uint32_t *lengths, *status_out;
};

// ---- filter: a wave per row ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_filter_kernel(const PngFileArgs io, const PngDeflateArgs a) {
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6), img = blockIdx.y;
    if (row >= io.h) return;                                  // (the whole wave)
    const uint8_t* frame = io.images + static_cast<size_t>(img) * io.image_bytes;
    const uint32_t* cur = reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(row) * io.stride);
    const uint32_t* prev = reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(row ? row - 1u : 0u) * io.stride);   // the row above comes from HBM / L2 again
    const bool top = row == 0u;
    uint32_t sums[5] = {0, 0, 0, 0, 0};
    for (uint32_t x = lane; x < io.w; x += 64u) {
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
    for (uint32_t x = lane; x < io.w; x += 64u) {
        const uint32_t px = cur[x], pa = x ? cur[x - 1u] : 0u, pb = top ? 0u : prev[x], pc = (top || !x) ? 0u : prev[x - 1u];
        for (uint32_t ch = 0; ch < a.bpp; ++ch)
            out[1u + x * a.bpp + ch] = static_cast<uint8_t>(png_filter_byte(f, png_channel(px, ch), png_channel(pa, ch), png_channel(pb, ch), png_channel(pc, ch)));
    }
}

// ---- finish: the head and the IDAT framing, a workgroup per image -------------------------------------------------------------
__global__ __launch_bounds__(1024) void png_finish_kernel(const PngFileArgs io, const PngDeflateArgs a) {
    __shared__ uint32_t scratch[16];
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    const uint32_t body = a.image[img], adler = a.image[a.n_images + img];
    if (a.image[2u * a.n_images + img]) {
        if (tid == 0u) { io.lengths[img] = 0u; if (io.status_out) io.status_out[img] = kPngFileOverflow; }
        return;
    }
    uint8_t* file = io.files + static_cast<size_t>(img) * io.file_pitch;
    const uint32_t zlen = png_frame_idat<1024>(file + kPngHeadBytes, body, adler, io.zlib_header, a, img, scratch);
    if (tid == 0u) {
        png_write_head(file, io.w, io.h, io.color_type);
        io.lengths[img] = kPngFraming + zlen;
        if (io.status_out) io.status_out[img] = 0u;
    }
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_png_enc_stage {
    uint32_t width = 0, height = 0, color_type = 0, max_images = 0;
    PngDeflateScratch deflate;
};

extern "C" {

int ifhip_png_enc_stage_create(ifhip_png_enc_stage** stage, uint32_t width, uint32_t height, int color_type, uint32_t max_images) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage out-pointer");
    *stage = nullptr;
    if (color_type != IFHIP_PNG_RGB && color_type != IFHIP_PNG_RGBA) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: color_type is 2 (RGB) or 6 (RGBA)");
    if (width == 0 || height == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (max_images == 0 || max_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 images per stage");
    const uint32_t bpp = color_type == IFHIP_PNG_RGB ? 3u : 4u;
    const uint64_t bytes = (1ull + static_cast<uint64_t>(width) * bpp) * height;
    if (bytes > 0x7FFF0000ull) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a filtered image of %llu bytes (one IDAT chunk holds 2^31 - 1)", static_cast<unsigned long long>(bytes));
    std::unique_ptr<ifhip_png_enc_stage> s(new ifhip_png_enc_stage);
    s->width = width; s->height = height; s->color_type = static_cast<uint32_t>(color_type); s->max_images = max_images;
    s->deflate.shape(width, bpp, height);
    *stage = s.release();
    return IFHIP_OK;
}

void ifhip_png_enc_stage_destroy(ifhip_png_enc_stage* stage) { delete stage; }

size_t ifhip_png_enc_stage_max_file_bytes(const ifhip_png_enc_stage* stage) { return stage ? stage->deflate.max_body_bytes() + kPngFraming : 0u; }

int ifhip_png_encode_batch_device(ifhip_png_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, uint32_t n_images,
                                  int zlib_level, uint8_t* d_files, size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status, void* hip_stream) {
    bool go = false;
    if (int rc = open_encode_batch(stage, d_images, image_bytes, stride, n_images, d_files, d_lengths, &go); rc || !go) return rc;
    if (zlib_level < -1 || zlib_level > 9) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: zlib_level is -1 or 0..9");
    if (file_pitch < kPngFraming + 6u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: file_pitch below %u bytes", kPngFraming + 6u);
    if (int rc = stage->deflate.allocate(stage->max_images)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const PngFileArgs io{d_images, image_bytes, stride, stage->width, stage->height, stage->color_type, png_zlib_header(zlib_level),
                         d_files, file_pitch, d_lengths, d_status};
    // the body goes straight into its place in the file, behind the head, IDAT's length and type and the zlib header, and
    // may take what the framing leaves of file_pitch (no body is larger than 2^32 - 1 bytes)
    const uint32_t room = static_cast<uint32_t>(std::min<size_t>(file_pitch - kPngFraming - 6u, 0xFFFFFFFFu));
    const PngDeflateArgs a = stage->deflate.args(n_images, zlib_level, d_files + kPngHeadBytes + 10u, file_pitch, room);
    hipLaunchKernelGGL(png_filter_kernel, dim3((stage->height + 3u) / 4u, n_images), dim3(256), 0, st, io, a);
    png_launch_deflate(a, st);
    hipLaunchKernelGGL(png_finish_kernel, dim3(n_images), dim3(1024), 0, st, io, a);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_png_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int color_type, int zlib_level, uint8_t* out,
                     size_t capacity, size_t* len) {
    uint32_t status = 0;
    if (int rc = encode_host_frame(
            bgra, width, height, stride, out, capacity, len, &status, [&](ifhip_png_enc_stage** s) { return ifhip_png_enc_stage_create(s, width, height, color_type, 1); },
            ifhip_png_enc_stage_destroy, ifhip_png_enc_stage_max_file_bytes, [&](ifhip_png_enc_stage* s, const HostFrame& f, size_t pitch, uint32_t* d_len) {
                return ifhip_png_encode_batch_device(s, f.d, f.image_bytes, stride, 1, zlib_level, f.side_output(), pitch, d_len, d_len + 1, nullptr);
            })) return rc;
    return refuse_unfitted_file(status, *len);
}

}  // extern "C"
