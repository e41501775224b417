// gif_encode.hip -- gfx950 kernels + C ABI of the device GIF coder: BGRA / BGRX frames in HBM -> GIF89a files in HBM.
//
// Replaces what EncoderPreset::Gif runs on the host (imageflow_core/src/codecs/gif/mod.rs:385-592: gif::Frame::from_rgba's
// quantisation and the gif crate's LZW writer).  Every rule lives in gif_encode_core.hpp, shared with the CPU emulation of
// the tests (tests/gif_encode_emulate.cpp); the palette is the quantiser's of png_quantize.hip under the key rule
// kPqKeyGif.  Launches per batch (all images in each), whatever the frames hold:
//   * the two clears, the six histogram levels and the palette of png_quantize.hip (pq_launch_palette);
//   * remap, grid-wide: the nearest palette entry of every pixel, the palette in LDS, an index byte per pixel;
//   * lzw: a wave per segment of kGifEncSegmentPixels indices, the string table an open-addressed hash in LDS; the
//     segment's bits go to its private slot, its bit length to the segment's word;
//   * scan (a workgroup per image): the segments' bit offsets and the total;
//   * gather: every dword of the frame's stream is assembled by the lane that owns it;
//   * finish: the stream into 255-byte sub-blocks, the head, the terminator and ';'.
// The palette's size -- and with it the minimum code size and the head's length -- is read on the device.
//
// N frames into ONE file (ifhip_gif_encode_animation_device): the launches above up to the gather run per chunk
// of at most max_images frames, then
//   * offsets (one workgroup): the chunk's body lengths, their exclusive sum on top of the running byte offset that lives on
//     the device, every frame's head into the stage;
//   * layout: every dword of the FILE that ends inside the chunk's bytes is assembled by the lane that owns it; the bytes
//     in front of the first such dword come from the chunk before through a carry word, so no dword is written twice.
// Nothing is read back between chunks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>

#include "block_scan.hpp"
#include "decode_handoff.hpp"      // StagedBlock
#include "encode_handoff.hpp"
#include "gif_encode_core.hpp"
#include "png_quantize.hpp"
#include "stage_scratch.hpp"

namespace ifhip {

struct GifEncArgs {
    uint32_t n_seg, slot_words, stream_words;   // per image
    size_t index_pitch;                         // bytes of an image's indices in the stage
    uint8_t* indices;                           // [n_images][index_pitch]
    uint32_t* slots;                            // [n_images][n_seg][slot_words]
    uint32_t* seg_bits;                         // [n_images][n_seg + 1]: lengths, then exclusive offsets and the total
    uint32_t* stream;                           // [n_images][stream_words]
    int32_t repeat;
    uint32_t delay, user_input;
};

// ---- remap: grid-wide, no dithering ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGifEncThreads) void gif_remap_kernel(const QuantArgs a, const GifEncArgs g) {
    __shared__ PqColor pal[kPqMaxColors];
    const uint32_t tid = threadIdx.x, img = blockIdx.y;
    const uint32_t* r = a.result + static_cast<size_t>(img) * kPqResultWords;
    const uint32_t count = r[0];
    if (tid < count) pal[tid] = pq_premultiply(r[8u + tid]);
    __syncthreads();
    const uint8_t* frame = a.images + static_cast<size_t>(img) * a.image_bytes;
    uint8_t* out = g.indices + static_cast<size_t>(img) * g.index_pitch;
    uint8_t* tap = a.indices ? a.indices + static_cast<size_t>(img) * a.w * a.h : nullptr;
    const uint32_t npix = a.w * a.h;
    for (uint32_t i = blockIdx.x * kGifEncThreads + tid; i < npix; i += gridDim.x * kGifEncThreads) {
        const uint32_t y = i / a.w, x = i - y * a.w;
        const uint32_t px = *reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(y) * a.stride + 4u * x);
        uint64_t d;
        const uint8_t idx = static_cast<uint8_t>(pq_nearest(pal, count, pq_premultiply(pq_key(px, a.alpha != 0u, kPqKeyGif)), &d));
        out[i] = idx;
        if (tap) tap[i] = idx;
    }
}

// ---- lzw: a wave per segment -------------------------------------------------------------------------------------------------------------
struct GifEncWave {
    uint32_t held = 0;
    __device__ __forceinline__ void fetch(const uint8_t* p, uint32_t base, uint32_t n) { held = base + threadIdx.x < n ? p[base + threadIdx.x] : 0u; }
    __device__ __forceinline__ uint32_t byte(uint32_t j) const { return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(held), static_cast<int>(j))); }
    __device__ __forceinline__ uint32_t uniform(uint32_t v) const { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }
    __device__ __forceinline__ void clear(uint32_t* table) {
        __syncthreads();                                         // (one wave: what the lanes wrote before is ordered before the clear)
        for (uint32_t i = threadIdx.x; i < kGifEncHashSlots; i += 64u) table[i] = 0u;
        __syncthreads();
    }
    template <typename F> __device__ __forceinline__ void one(F f) { if (threadIdx.x == 0u) f(); }
};

__global__ __launch_bounds__(64) void gif_lzw_kernel(const QuantArgs a, const GifEncArgs g) {
    __shared__ uint32_t table[kGifEncHashSlots];
    const uint32_t seg = blockIdx.x, img = blockIdx.y;
    const uint32_t npix = a.w * a.h, first_pixel = seg * kGifEncSegmentPixels;
    const uint32_t n = npix - first_pixel < kGifEncSegmentPixels ? npix - first_pixel : kGifEncSegmentPixels;
    const uint32_t count = a.result[static_cast<size_t>(img) * kPqResultWords];
    GifEncWave x;
    const uint32_t bits = gifenc_segment(x, table, g.indices + static_cast<size_t>(img) * g.index_pitch + first_pixel, n, x.uniform(gifenc_min_code(count)),
                                         seg == 0u, seg + 1u == g.n_seg, g.slots + (static_cast<size_t>(img) * g.n_seg + seg) * g.slot_words);
    if (threadIdx.x == 0u) g.seg_bits[static_cast<size_t>(img) * (g.n_seg + 1u) + seg] = bits;
}

// ---- scan: a workgroup per image -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGifEncThreads) void gif_enc_scan_kernel(const GifEncArgs g) {
    __shared__ uint32_t scratch[kGifEncThreads / 64u];
    uint32_t* bits = g.seg_bits + static_cast<size_t>(blockIdx.x) * (g.n_seg + 1u);
    uint32_t base = 0;
    for (uint32_t s0 = 0; s0 < g.n_seg; s0 += kGifEncThreads) {
        const uint32_t s = s0 + threadIdx.x, v = s < g.n_seg ? bits[s] : 0u;
        uint32_t total = 0;
        const uint32_t before = block_exclusive_scan<kGifEncThreads>(v, scratch, &total);
        if (s < g.n_seg) bits[s] = base + before;
        base += total;
    }
    if (threadIdx.x == 0u) bits[g.n_seg] = base;
}

// ---- gather: a lane per dword of the stream -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGifEncThreads) void gif_gather_kernel(const GifEncArgs g) {
    const uint32_t img = blockIdx.y;
    const uint32_t* off = g.seg_bits + static_cast<size_t>(img) * (g.n_seg + 1u);
    const uint32_t* slots = g.slots + static_cast<size_t>(img) * g.n_seg * g.slot_words;
    uint32_t* stream = g.stream + static_cast<size_t>(img) * g.stream_words;
    const uint32_t words = (off[g.n_seg] + 31u) / 32u;           // (<= stream_words: gifenc_max_data_bytes)
    for (uint32_t j = blockIdx.x * kGifEncThreads + threadIdx.x; j < words && j < g.stream_words; j += gridDim.x * kGifEncThreads)
        stream[j] = gifenc_gather_word(off, g.n_seg, slots, g.slot_words, j);
}

// ---- finish: sub-blocks, head and tail ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGifEncThreads) void gif_finish_kernel(const QuantArgs a, const GifEncArgs g) {
    const uint32_t tid = threadIdx.x, img = blockIdx.y;
    const uint32_t* r = a.result + static_cast<size_t>(img) * kPqResultWords;
    const uint32_t count = r[0], n_trans = r[1];
    const uint32_t data = (g.seg_bits[static_cast<size_t>(img) * (g.n_seg + 1u) + g.n_seg] + 7u) / 8u;
    const uint32_t head = gifenc_head_bytes(count, g.repeat);
    const uint64_t total = gifenc_file_bytes(head, data);
    if (total > a.file_pitch) {                                  // (uniform) no file: the neighbours' are not touched
        if (blockIdx.x == 0u && tid == 0u) { a.lengths[img] = 0u; if (a.status_out) a.status_out[img] = kGifEncFileOverflow; }
        return;
    }
    uint8_t* file = a.files + static_cast<size_t>(img) * a.file_pitch;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(g.stream + static_cast<size_t>(img) * g.stream_words);
    for (uint32_t i = blockIdx.x * kGifEncThreads + tid; i < data; i += gridDim.x * kGifEncThreads) {
        const uint64_t at = head + gifenc_data_position(i);
        file[at] = src[i];
        if (i % 255u == 0u) file[at - 1u] = static_cast<uint8_t>(data - i < 255u ? data - i : 255u);
    }
    if (blockIdx.x != 0u || tid != 0u) return;
    gifenc_write_head(file, a.w, a.h, r + 8, count, n_trans, g.repeat, g.delay, g.user_input);
    file[total - 2u] = 0; file[total - 1u] = 0x3B;
    a.lengths[img] = static_cast<uint32_t>(total);
    if (a.status_out) a.status_out[img] = 0u;
}

// ---- the animation: offsets and layout ------------------------------------------------------------------------------------------------------
struct GifAnimArgs {
    uint32_t* run;                  // [0] the file's bytes so far, [1] an overflow was seen, [2], [3] the carry words of even / odd chunks
    uint32_t *off, *data_bytes, *head_bytes;     // [max_images + 1], [max_images], [max_images]
    uint8_t* heads;                 // kGifEncScreenPitch + max_images * kGifEncFrameHeadPitch
    const uint32_t* meta;           // the chunk's frames: delay | user_input << 16
    uint8_t* file;
    uint32_t* length;
    uint32_t* status;
    uint32_t capacity, n, chunk, first, last, dispose;
};

__global__ __launch_bounds__(kGifEncThreads) void gif_anim_offsets_kernel(const QuantArgs a, const GifEncArgs g, const GifAnimArgs m) {
    __shared__ uint32_t scratch[kGifEncThreads / 64u];
    const uint32_t tid = threadIdx.x;
    uint32_t base = m.first ? gifenc_screen_bytes(g.repeat) : m.run[0];      // (read by every lane in front of the first barrier, written behind the last)
    for (uint32_t i0 = 0; i0 < m.n; i0 += kGifEncThreads) {
        const uint32_t i = i0 + tid;
        uint32_t body = 0, count = 0, data = 0;
        const uint32_t* r = a.result + static_cast<size_t>(i) * kPqResultWords;
        if (i < m.n) {
            count = r[0];
            data = (g.seg_bits[static_cast<size_t>(i) * (g.n_seg + 1u) + g.n_seg] + 7u) / 8u;
            body = gifenc_body_bytes(count, data);
        }
        uint32_t total = 0;
        const uint32_t before = block_exclusive_scan<kGifEncThreads>(body, scratch, &total);
        if (i < m.n) {
            m.off[i] = base + before; m.data_bytes[i] = data; m.head_bytes[i] = gifenc_frame_head_bytes(count);
            gifenc_write_frame_head(m.heads + kGifEncScreenPitch + static_cast<size_t>(i) * kGifEncFrameHeadPitch, a.w, a.h, r + 8, count, r[1], m.meta[i] & 0xFFFFu,
                                    m.meta[i] >> 16, m.dispose);
        }
        base += total;
    }
    if (tid != 0u) return;
    m.off[m.n] = base;
    const uint32_t seen = m.first ? 0u : m.run[1];
    m.run[0] = base;
    m.run[1] = (seen || static_cast<uint64_t>(base) + m.last > m.capacity) ? 1u : 0u;
    if (m.first) gifenc_write_screen(m.heads, a.w, a.h, g.repeat);
}

__global__ __launch_bounds__(kGifEncThreads) void gif_anim_layout_kernel(const GifEncArgs g, const GifAnimArgs m) {
    const uint32_t overflow = m.run[1];
    GifAnimChunk c;
    c.off = m.off; c.heads = m.heads; c.streams = reinterpret_cast<const uint8_t*>(g.stream); c.data_bytes = m.data_bytes; c.head_bytes = m.head_bytes;
    c.n = m.n; c.stream_pitch = g.stream_words * 4u; c.first = m.first; c.last = m.last;
    c.lo = m.first ? 0u : m.off[0]; c.hi = m.off[m.n] + m.last;
    const bool lane0 = blockIdx.x == 0u && threadIdx.x == 0u;
    if (m.last && lane0) { *m.length = overflow ? 0u : c.hi; if (m.status) *m.status = overflow ? kGifEncFileOverflow : 0u; }
    if (overflow) return;                                        // (uniform; c.hi <= capacity from here on)
    const uint32_t carry_in = m.first ? 0u : m.run[2u + ((m.chunk + 1u) & 1u)];
    const uint32_t j0 = c.lo / 4u, j1 = c.hi / 4u;
    uint32_t* file = reinterpret_cast<uint32_t*>(m.file);
    for (uint32_t j = j0 + blockIdx.x * kGifEncThreads + threadIdx.x; j < j1; j += gridDim.x * kGifEncThreads) file[j] = gifenc_animation_word(c, j, carry_in);
    if (!lane0) return;
    const uint32_t tail = gifenc_animation_word(c, j1, carry_in);  // the bytes behind the last whole dword
    if (!m.last) { m.run[2u + (m.chunk & 1u)] = tail; return; }
    for (uint32_t p = 4u * j1; p < c.hi; ++p) m.file[p] = static_cast<uint8_t>(tail >> (8u * (p - 4u * j1)));
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_gif_enc_stage {
    uint32_t width = 0, height = 0, max_images = 0;
    uint32_t n_seg = 0, stream_words = 0;
    size_t index_pitch = 0;
    uint8_t* d_indices = nullptr;
    uint32_t *d_slots = nullptr, *d_seg_bits = nullptr, *d_stream = nullptr;
    QuantScratch quant;
    uint32_t* d_anim = nullptr;                          // the animation's running words, offsets and lengths (GifAnimArgs)
    uint8_t* d_anim_heads = nullptr;
    StageScratch blocks{&d_indices, &d_slots, &d_seg_bits, &d_stream, &quant.d_tables, &quant.d_ekey, &quant.d_ew, &quant.d_edmin, &quant.d_result, &d_anim, &d_anim_heads};
};

namespace {
int gif_enc_stage_allocate(ifhip_gif_enc_stage* s) {
    const size_t n = s->max_images;
    return s->blocks.ensure([&]() -> int {
        HIP_TRY(DEV_MALLOC(&s->d_indices, n * s->index_pitch));
        HIP_TRY(DEV_MALLOC(&s->d_slots, n * s->n_seg * gifenc_slot_words() * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_seg_bits, n * (s->n_seg + 1u) * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_stream, n * s->stream_words * sizeof(uint32_t)));
        if (int rc = s->quant.allocate(n)) return rc;
        HIP_TRY(DEV_MALLOC(&s->d_anim, (8u + 3u * n + 1u) * sizeof(uint32_t)));
        HIP_TRY(DEV_MALLOC(&s->d_anim_heads, kGifEncScreenPitch + n * kGifEncFrameHeadPitch));
        return IFHIP_OK;
    });
}
// the arguments of one batch of `n_images` frames through the stage (the caller adds where the files go)
void gif_enc_args(ifhip_gif_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, int alpha_meaningful, uint32_t n_images, int repeat,
                  QuantArgs* qp, GifEncArgs* gp) {
    // the pngquant preset's defaults (codecs/pngquant.rs:50-57): speed 4, target 100, minimum 0
    stage->quant.fill(qp, d_images, image_bytes, stride, stage->width, stage->height, n_images, alpha_meaningful, kPqMaxColors, 4u, 100u, 0u);
    qp->key_rule = kPqKeyGif;
    GifEncArgs& g = *gp;
    std::memset(&g, 0, sizeof g);
    g.n_seg = stage->n_seg; g.slot_words = gifenc_slot_words(); g.stream_words = stage->stream_words; g.index_pitch = stage->index_pitch;
    g.indices = stage->d_indices; g.slots = stage->d_slots; g.seg_bits = stage->d_seg_bits; g.stream = stage->d_stream;
    g.repeat = repeat;
}
// palette, remap, lzw, scan and gather: every frame's LZW stream and its length in the stage
int gif_enc_launch_streams(ifhip_gif_enc_stage* stage, const QuantArgs& q, const GifEncArgs& g, hipStream_t st) {
    if (int rc = pq_launch_palette(q, st)) return rc;
    const uint32_t npix = stage->width * stage->height;
    const uint32_t pixel_blocks = std::min(1024u, (npix + kGifEncThreads - 1u) / kGifEncThreads);
    const uint32_t word_blocks = std::min(1024u, (stage->stream_words + kGifEncThreads - 1u) / kGifEncThreads);
    hipLaunchKernelGGL(gif_remap_kernel, dim3(pixel_blocks, q.n_images), dim3(kGifEncThreads), 0, st, q, g);
    hipLaunchKernelGGL(gif_lzw_kernel, dim3(stage->n_seg, q.n_images), dim3(64), 0, st, q, g);
    hipLaunchKernelGGL(gif_enc_scan_kernel, dim3(q.n_images), dim3(kGifEncThreads), 0, st, g);
    hipLaunchKernelGGL(gif_gather_kernel, dim3(word_blocks, q.n_images), dim3(kGifEncThreads), 0, st, g);
    return IFHIP_OK;
}
}  // namespace

extern "C" {

int ifhip_gif_enc_stage_create(ifhip_gif_enc_stage** stage, uint32_t width, uint32_t height, uint32_t max_images) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage out-pointer");
    *stage = nullptr;
    if (width == 0 || height == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    // size_16() (codecs/gif/mod.rs:385-592): the logical screen's sides are 16 bits wide
    if (width > 65535u || height > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: GIF dimensions must be at most 65535 (%ux%u)", width, height);
    if (max_images == 0 || max_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 images per stage");
    const uint64_t pixels = static_cast<uint64_t>(width) * height;
    if (pixels > kPqMaxPixels) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: %llu pixels (the quantiser's error sums hold 2^28)", static_cast<unsigned long long>(pixels));
    std::unique_ptr<ifhip_gif_enc_stage> s(new ifhip_gif_enc_stage);
    s->width = width; s->height = height; s->max_images = max_images;
    s->n_seg = gifenc_segments(static_cast<uint32_t>(pixels));
    s->stream_words = static_cast<uint32_t>((gifenc_max_data_bytes(pixels) + 3u) / 4u);
    s->index_pitch = (static_cast<size_t>(pixels) + 15u) & ~static_cast<size_t>(15u);
    *stage = s.release();
    return IFHIP_OK;
}

void ifhip_gif_enc_stage_destroy(ifhip_gif_enc_stage* stage) { delete stage; }

size_t ifhip_gif_enc_stage_max_file_bytes(const ifhip_gif_enc_stage* stage) {
    return stage ? static_cast<size_t>(gifenc_max_file_bytes(static_cast<uint64_t>(stage->width) * stage->height)) : 0u;
}

int ifhip_gif_encode_batch_device(ifhip_gif_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, int alpha_meaningful,
                                  uint32_t n_images, int repeat, uint32_t delay, int needs_user_input, uint8_t* d_files, size_t file_pitch,
                                  uint32_t* d_lengths, uint32_t* d_status, uint8_t* d_palettes, uint8_t* d_indices, void* hip_stream) {
    bool go = false;
    if (int rc = open_encode_batch(stage, d_images, image_bytes, stride, n_images, d_files, d_lengths, &go); rc || !go) return rc;
    if (repeat < -1 || repeat > 65535) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: repeat is -1 (none) or 0..65535");
    if (delay > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: delay is 0..65535 hundredths of a second");
    if (file_pitch < kGifEncHeadMax + 8u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: file_pitch below %u bytes", kGifEncHeadMax + 8u);
    if (int rc = gif_enc_stage_allocate(stage)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    QuantArgs q;
    GifEncArgs g;
    gif_enc_args(stage, d_images, image_bytes, stride, alpha_meaningful, n_images, repeat, &q, &g);
    q.palettes = d_palettes; q.indices = d_indices;
    q.files = d_files; q.file_pitch = file_pitch; q.lengths = d_lengths; q.status_out = d_status;
    g.delay = delay; g.user_input = needs_user_input ? 1u : 0u;
    if (int rc = gif_enc_launch_streams(stage, q, g, st)) return rc;
    const uint32_t word_blocks = std::min(1024u, (stage->stream_words + kGifEncThreads - 1u) / kGifEncThreads);
    hipLaunchKernelGGL(gif_finish_kernel, dim3(word_blocks, n_images), dim3(kGifEncThreads), 0, st, q, g);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_gif_enc_stage_max_animation_bytes(const ifhip_gif_enc_stage* stage, uint32_t n_frames, size_t* bytes) {
    if (!bytes) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *bytes = 0;
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage");
    if (n_frames == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: an animation has one frame at the least");
    // the head with NETSCAPE2.0, n times the one-frame file's bound (above a body's), ';'
    const uint64_t bound = gifenc_screen_bytes(0) + static_cast<uint64_t>(n_frames) * gifenc_max_file_bytes(static_cast<uint64_t>(stage->width) * stage->height) + 1u;
    if (bound >= (1ull << 32))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: %u frames of %ux%u may need %llu bytes (byte offsets in the file are 32 bits wide)", n_frames, stage->width,
                    stage->height, static_cast<unsigned long long>(bound));
    *bytes = static_cast<size_t>(bound);
    return IFHIP_OK;
}

int ifhip_gif_encode_animation_device(ifhip_gif_enc_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, int alpha_meaningful,
                                      uint32_t n_frames, int repeat, const uint32_t* delays, const uint8_t* user_input, uint8_t* d_file, size_t capacity,
                                      uint32_t* d_length, uint32_t* d_status, void* hip_stream) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage");
    if (n_frames == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: an animation has one frame at the least");
    if (int rc = check_frames(d_images, image_bytes, stage->width, stage->height, stride, "image")) return rc;
    if (!d_file || !d_length || !delays || !user_input) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    if (reinterpret_cast<uintptr_t>(d_file) & 3u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: the file's block must be 4-byte aligned");
    if (repeat < -1 || repeat > 65535) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: repeat is -1 (none) or 0..65535");
    for (uint32_t k = 0; k < n_frames; ++k)
        if (delays[k] > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: delay is 0..65535 hundredths of a second (frame %u)", k);
    if (capacity < gifenc_screen_bytes(0) + 1u)                  // (not even the screen part and ';': never a file, whatever the frames hold)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: capacity below %u bytes", gifenc_screen_bytes(0) + 1u);
    size_t bound = 0;
    if (int rc = ifhip_gif_enc_stage_max_animation_bytes(stage, n_frames, &bound)) return rc;
    if (int rc = gif_enc_stage_allocate(stage)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StagedBlock meta(st);                                        // delay | user_input << 16 per frame: the one upload
    if (int rc = meta.alloc(4u * static_cast<size_t>(n_frames), 4u * static_cast<size_t>(n_frames))) return rc;
    for (uint32_t k = 0; k < n_frames; ++k) {
        const uint32_t word = delays[k] | (user_input[k] ? 1u << 16 : 0u);
        std::memcpy(meta.host + 4u * static_cast<size_t>(k), &word, 4);
    }
    if (int rc = meta.send()) return rc;
    const uint32_t n = stage->max_images;
    GifAnimArgs m;
    std::memset(&m, 0, sizeof m);
    m.run = stage->d_anim; m.off = stage->d_anim + 8; m.data_bytes = m.off + n + 1u; m.head_bytes = m.data_bytes + n; m.heads = stage->d_anim_heads;
    m.file = d_file; m.length = d_length; m.status = d_status;
    m.capacity = static_cast<uint32_t>(std::min<size_t>(capacity, 0xFFFFFFFFu));
    m.dispose = gifenc_animation_dispose(n_frames, alpha_meaningful != 0);
    const uint64_t body_words = (gifenc_max_body_bytes(static_cast<uint64_t>(stage->width) * stage->height) + 3u) / 4u;
    for (uint32_t base = 0, chunk = 0; base < n_frames; base += n, ++chunk) {
        const uint32_t count = std::min(n, n_frames - base);
        QuantArgs q;
        GifEncArgs g;
        gif_enc_args(stage, d_images + static_cast<size_t>(base) * image_bytes, image_bytes, stride, alpha_meaningful, count, repeat, &q, &g);
        if (int rc = gif_enc_launch_streams(stage, q, g, st)) return rc;
        m.meta = reinterpret_cast<const uint32_t*>(meta.block) + base;
        m.n = count; m.chunk = chunk; m.first = base == 0u ? 1u : 0u; m.last = base + count == n_frames ? 1u : 0u;
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(4096u, (body_words * count + 16u + kGifEncThreads - 1u) / kGifEncThreads));
        hipLaunchKernelGGL(gif_anim_offsets_kernel, dim3(1), dim3(kGifEncThreads), 0, st, q, g, m);
        hipLaunchKernelGGL(gif_anim_layout_kernel, dim3(blocks), dim3(kGifEncThreads), 0, st, g, m);
    }
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_gif_encode(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful, int repeat, uint32_t delay,
                     int needs_user_input, uint8_t* out, size_t capacity, size_t* len) {
    uint32_t status = 0;
    if (int rc = encode_host_frame(
            bgra, width, height, stride, out, capacity, len, &status, [&](ifhip_gif_enc_stage** s) { return ifhip_gif_enc_stage_create(s, width, height, 1); },
            ifhip_gif_enc_stage_destroy, ifhip_gif_enc_stage_max_file_bytes, [&](ifhip_gif_enc_stage* s, const HostFrame& f, size_t pitch, uint32_t* d_len) {
                return ifhip_gif_encode_batch_device(s, f.d, f.image_bytes, stride, alpha_meaningful, 1, repeat, delay, needs_user_input, f.side_output(), pitch,
                                                     d_len, d_len + 1, nullptr, nullptr, nullptr);
            })) return rc;
    return refuse_unfitted_file(status, *len);
}

}  // extern "C"
