// png_quantize.hip -- gfx950 kernels + C ABI of the device palette coder: BGRA / BGRX frames in HBM -> 8-bit palette PNG
// files in HBM.
//
// Replaces what EncoderPreset::Pngquant runs on the host (codecs/pngquant.rs:35-139: libimagequant's quantisation and
// remap with dithering level 1.0, then lode::LodepngEncoder::write_png8, lode.rs:162-195).  The quantiser is this
// project's own; every rule of it lives in png_quantize_core.hpp, shared with the CPU emulation of the tests
// (tests/png_quantize_emulate.cpp).  Launches per batch (all images in each):
//   * histogram, once per posterise level: a grid-wide exact hash table by atomicCAS; a level runs only when every level
//     before it overflowed, which it reads from the device -- the host never waits;
//   * palette (a workgroup per image): the table's entries are packed, the palette grows one entry per pass over them and
//     is refined by Lloyd iterations with the palette and the 64-bit integer sums in LDS;
//   * remap (a workgroup per image): nearest entry with Floyd-Steinberg error diffusion as a skewed wavefront -- lane L
//     takes rows L, L + 1024, ..., two columns behind the lane above -- and writes the filtered stream itself;
//   * match / codes / layout / emit of the deflate back end (png_deflate.hip) on that stream with bpp = 1; the zlib body
//     lands in the stage, since the size of the head in front of it is not known before the palette is;
//   * finish: IHDR (type 3), PLTE, tRNS, the body into place and the IDAT framing around it (png_frame_device.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>

#include "encode_handoff.hpp"
#include "png_frame_device.hpp"      // (with png_deflate.hpp)
#include "png_quantize.hpp"           // (with png_quantize_core.hpp)

namespace ifhip {

constexpr uint32_t kPqLanes = 1024;          // the remap's rows in flight: a workgroup's most
constexpr uint32_t kPqLastRowCols = 16384;   // the widest frame of more than kPqLanes rows: the last lane's error row lies in LDS
constexpr uint32_t kPqCopyBlocks = 16;

__device__ __forceinline__ bool pq_level_runs(const uint32_t* state, uint32_t level) {
    for (uint32_t q = 0; q < level; ++q) if (!state[q]) return false;      // an earlier level held all colours
    return true;
}

// ---- histogram: grid-wide, one launch per level ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pngq_histogram_kernel(const QuantArgs a, const uint32_t level) {
    const uint32_t img = blockIdx.y;
    uint32_t* state = a.state + static_cast<size_t>(img) * kPqStateWords;
    if (!pq_level_runs(state, level)) return;
    uint32_t* slots = a.tables + (static_cast<size_t>(img) * kPqLevels + level) * 2u * kPqSlots;
    uint32_t* counts = slots + kPqSlots;
    const uint8_t* frame = a.images + static_cast<size_t>(img) * a.image_bytes;
    const uint32_t npix = a.w * a.h;
    auto cas = [](uint32_t* p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); };
    auto add = [](uint32_t* p, uint32_t v) { return atomicAdd(p, v); };
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < npix; i += gridDim.x * 256u) {
        const uint32_t y = i / a.w, x = i - y * a.w;
        const uint32_t px = *reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(y) * a.stride + 4u * x);
        if (!pq_insert(slots, counts, state + kPqLevels + level, a.max_entries, pq_posterize(pq_key(px, a.alpha != 0u, a.key_rule), level), cas, add)) {
            state[level] = 1u;                                       // the pass is void: the next level runs
            break;
        }
    }
}

// ---- palette: a workgroup per image ------------------------------------------------------------------------------------------------
struct PaletteLds {
    uint32_t keys[kPqMaxColors];
    PqColor pal[kPqMaxColors];
    unsigned long long sums[kPqMaxColors * 5u];
    uint64_t red_err[kPqLanes / 64u], red_score[kPqLanes / 64u];
    uint32_t red_key[kPqLanes / 64u];
    uint32_t n;
};
// the workgroup's PqGrow: errors add, the best (score, then lowest key) wins; the same in every lane
__device__ __forceinline__ void pq_block_reduce(PqGrow& g, PaletteLds& s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        g.err += __shfl_xor(static_cast<unsigned long long>(g.err), d, 64);
        const uint64_t os = __shfl_xor(static_cast<unsigned long long>(g.score), d, 64);
        const uint32_t ok = __shfl_xor(g.key, d, 64);
        pq_grow_better(&g, os, ok);
    }
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) { s.red_err[threadIdx.x >> 6] = g.err; s.red_score[threadIdx.x >> 6] = g.score; s.red_key[threadIdx.x >> 6] = g.key; }
    __syncthreads();
    g.err = 0u; g.score = 0u; g.key = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t w = 0; w < kPqLanes / 64u; ++w) { g.err += s.red_err[w]; pq_grow_better(&g, s.red_score[w], s.red_key[w]); }
}

__global__ __launch_bounds__(kPqLanes) void pngq_palette_kernel(const QuantArgs a) {
    __shared__ PaletteLds s;
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    const uint32_t* state = a.state + static_cast<size_t>(img) * kPqStateWords;
    uint32_t level = 0;
    while (level + 1u < kPqLevels && state[level]) ++level;
    const uint32_t* slots = a.tables + (static_cast<size_t>(img) * kPqLevels + level) * 2u * kPqSlots;
    const uint32_t* counts = slots + kPqSlots;
    uint32_t* ekey = a.ekey + static_cast<size_t>(img) * kPqMaxEntries;
    uint32_t* ew = a.ew + static_cast<size_t>(img) * kPqMaxEntries;
    uint64_t* edmin = a.edmin + static_cast<size_t>(img) * kPqMaxEntries;
    if (tid == 0u) s.n = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < kPqSlots; i += kPqLanes) {            // pack the entries; their order is free, nothing below depends on it
        const uint32_t held = slots[i];
        if (held) {
            const uint32_t at = atomicAdd(&s.n, 1u);
            if (at < kPqMaxEntries) { ekey[at] = held ^ kPqSlotXor; ew[at] = counts[i]; }
        }
    }
    __syncthreads();
    const uint32_t n = min(s.n, kPqMaxEntries);
    const uint64_t pixels = static_cast<uint64_t>(a.w) * a.h;
    // growth
    PqGrow g{0u, 0u, 0xFFFFFFFFu};
    for (uint32_t i = tid; i < n; i += kPqLanes) pq_grow_better(&g, ew[i], ekey[i]);
    pq_block_reduce(g, s);
    uint32_t newest = g.key, count = 1;
    for (;;) {
        g.err = 0u; g.score = 0u; g.key = 0xFFFFFFFFu;
        pq_grow_lane(ekey, ew, edmin, n, tid, kPqLanes, newest, count == 1u, &g);
        pq_block_reduce(g, s);
        if (tid == 0u) s.keys[count - 1u] = newest;
        if (g.err <= a.bound_target * pixels || count >= a.max_colors) break;
        newest = g.key;
        ++count;
    }
    __syncthreads();
    // Lloyd iterations over the histogram entries: integer sums, so the order of the atomics does not show
    for (uint32_t it = 0; it < a.iterations; ++it) {
        for (uint32_t i = tid; i < kPqMaxColors * 5u; i += kPqLanes) s.sums[i] = 0ull;
        if (tid < count) s.pal[tid] = pq_premultiply(s.keys[tid]);
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kPqLanes) {
            uint64_t d;
            const uint32_t k = ekey[i], idx = pq_nearest(s.pal, count, pq_premultiply(k), &d);
            const uint64_t wt = ew[i], wa = wt * (k >> 24);
            atomicAdd(&s.sums[idx * 5u + 0u], static_cast<unsigned long long>(wa * (k & 255u)));
            atomicAdd(&s.sums[idx * 5u + 1u], static_cast<unsigned long long>(wa * ((k >> 8) & 255u)));
            atomicAdd(&s.sums[idx * 5u + 2u], static_cast<unsigned long long>(wa * ((k >> 16) & 255u)));
            atomicAdd(&s.sums[idx * 5u + 3u], static_cast<unsigned long long>(wa));
            atomicAdd(&s.sums[idx * 5u + 4u], static_cast<unsigned long long>(wt));
        }
        __syncthreads();
        if (tid < count) {
            uint64_t sums[5];
            for (int k = 0; k < 5; ++k) sums[k] = s.sums[tid * 5u + k];
            s.keys[tid] = pq_centroid(sums, s.keys[tid]);
        }
        __syncthreads();
    }
    if (tid < count) s.pal[tid] = pq_premultiply(s.keys[tid]);
    __syncthreads();
    g.err = 0u; g.score = 0u; g.key = 0xFFFFFFFFu;
    for (uint32_t i = tid; i < n; i += kPqLanes) { uint64_t d; pq_nearest(s.pal, count, pq_premultiply(ekey[i]), &d); g.err += d * ew[i]; }
    pq_block_reduce(g, s);
    if (tid == 0u) {
        uint32_t* r = a.result + static_cast<size_t>(img) * kPqResultWords;
        const uint32_t n_trans = pq_order_palette(s.keys, count, r + 8);
        r[0] = count; r[1] = n_trans; r[2] = g.err > a.bound_min * pixels ? 1u : 0u; r[3] = level; r[4] = n; r[5] = 0u;
        r[6] = static_cast<uint32_t>(g.err); r[7] = static_cast<uint32_t>(g.err >> 32);
        if (a.mse) a.mse[img] = static_cast<double>(g.err) / (static_cast<double>(pixels) * static_cast<double>(kPqDistanceUnit));
        if (a.palettes) {
            uint8_t* p = a.palettes + static_cast<size_t>(img) * kPqPaletteTap;
            for (uint32_t i = 0; i < kPqMaxColors; ++i) {
                const uint32_t k = i < count ? r[8u + i] : 0u;
                p[4u * i] = static_cast<uint8_t>(k >> 16); p[4u * i + 1u] = static_cast<uint8_t>(k >> 8); p[4u * i + 2u] = static_cast<uint8_t>(k); p[4u * i + 3u] = static_cast<uint8_t>(k >> 24);
            }
            p[4u * kPqMaxColors] = static_cast<uint8_t>(count); p[4u * kPqMaxColors + 1u] = static_cast<uint8_t>(count >> 8);
            p[4u * kPqMaxColors + 2u] = 0; p[4u * kPqMaxColors + 3u] = 0;
        }
    }
}

// ---- remap: a workgroup per image, a skewed wavefront over the rows ----------------------------------------------------------------
// Row y at column x needs the errors of row y - 1 up to column x + 1, so lane L works two columns behind lane L - 1 and a
// step is one pixel per lane.  A lane that finishes row r goes on with row r + kPqLanes, `period` steps after it began r:
// period = max(w, 2 * kPqLanes) keeps lane 0 two columns behind the last lane's row above it.  What a lane hands down goes
// through a two-slot ring per lane (the reader is exactly two columns behind); the last lane's row, which lane 0 reads up
// to a whole row later, lies in LDS in full.
struct RemapLds {
    PqColor pal[kPqMaxColors];
    uint32_t keys[kPqMaxColors];
    short4 ring[kPqLanes][2];
    short4 last[kPqLastRowCols];
};
static_assert(sizeof(RemapLds) <= 160u * 1024u, "the remap's palette, rings and last row fit a workgroup's LDS");

__global__ __launch_bounds__(kPqLanes) void pngq_remap_kernel(const QuantArgs a, const PngDeflateArgs png) {
    __shared__ RemapLds s;
    const uint32_t tid = threadIdx.x, img = blockIdx.x;
    const uint32_t* r = a.result + static_cast<size_t>(img) * kPqResultWords;
    const uint32_t count = r[0];
    if (tid < count) { s.keys[tid] = r[8u + tid]; s.pal[tid] = pq_premultiply(r[8u + tid]); }
    __syncthreads();
    const uint8_t* frame = a.images + static_cast<size_t>(img) * a.image_bytes;
    uint8_t* stream = png.streams + static_cast<size_t>(img) * png.stream_pitch;
    uint8_t* tap = a.indices ? a.indices + static_cast<size_t>(img) * a.w * a.h : nullptr;
    const uint32_t w = a.w, h = a.h, period = max(w, 2u * kPqLanes);
    const uint32_t steps = 2u * ((h - 1u) % kPqLanes) + ((h - 1u) / kPqLanes) * period + w;
    const bool dither = a.dither != 0u, alpha = a.alpha != 0u;
    int32_t right[4] = {0, 0, 0, 0}, acc_prev[4] = {0, 0, 0, 0}, acc_cur[4] = {0, 0, 0, 0};
    for (uint32_t t = 0; t < steps; ++t) {
        const uint32_t rel = t - 2u * tid;                          // (wraps while the lane has not started)
        const uint32_t pass = t >= 2u * tid ? rel / period : 0u, x = rel - pass * period, y = pass * kPqLanes + tid;
        const bool active = t >= 2u * tid && x < w && y < h;
        short4 above = make_short4(0, 0, 0, 0);
        uint32_t px = 0;
        if (active) {
            if (y > 0u && dither) above = tid == 0u ? s.last[x] : s.ring[tid - 1u][x & 1u];
            px = *reinterpret_cast<const uint32_t*>(frame + static_cast<size_t>(y) * a.stride + 4u * x);
        }
        __syncthreads();                                             // every lane has read what the step before handed down
        if (active) {
            if (x == 0u) for (int k = 0; k < 4; ++k) { right[k] = 0; acc_prev[k] = 0; acc_cur[k] = 0; }
            const int32_t in[4] = {right[0] + above.x, right[1] + above.y, right[2] + above.z, right[3] + above.w};
            int32_t e[4], out[4];
            const uint32_t idx = pq_remap_pixel(s.pal, s.keys, count, pq_normalize(px, alpha), in, dither, e);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int32_t bl, b, br;
                pq_split_error(e[k], &right[k], &bl, &b, &br);
                out[k] = acc_prev[k] + bl; acc_prev[k] = acc_cur[k] + b; acc_cur[k] = br;
            }
            if (dither) {
                short4* row = tid == kPqLanes - 1u ? s.last : nullptr;
                if (x > 0u) {
                    const short4 v = make_short4(static_cast<short>(out[0]), static_cast<short>(out[1]), static_cast<short>(out[2]), static_cast<short>(out[3]));
                    if (row) row[x - 1u] = v; else s.ring[tid][(x - 1u) & 1u] = v;
                }
                if (x == w - 1u) {
                    const short4 v = make_short4(static_cast<short>(acc_prev[0]), static_cast<short>(acc_prev[1]), static_cast<short>(acc_prev[2]), static_cast<short>(acc_prev[3]));
                    if (row) row[x] = v; else s.ring[tid][x & 1u] = v;
                }
            }
            if (x == 0u) stream[static_cast<size_t>(y) * png.pitch] = 0;     // filter type 0 on every row (lode.rs:162-195)
            stream[static_cast<size_t>(y) * png.pitch + 1u + x] = static_cast<uint8_t>(idx);
            if (tap) tap[static_cast<size_t>(y) * w + x] = static_cast<uint8_t>(idx);
        }
        __syncthreads();
    }
}

// ---- finish: the palette framing, the IDAT chunk's CRC and the body into place -----------------------------------------------------
__global__ __launch_bounds__(256) void pngq_finish_kernel(const QuantArgs a, const PngDeflateArgs png) {
    __shared__ uint32_t scratch[4];
    const uint32_t tid = threadIdx.x, img = blockIdx.y;
    const uint32_t* r = a.result + static_cast<size_t>(img) * kPqResultWords;
    const uint32_t count = r[0], n_trans = r[1];
    const uint32_t body = png.image[img], adler = png.image[png.n_images + img];
    const uint32_t head = pq_head_bytes(count, n_trans), zlen = 2u + body + 4u;
    const uint64_t total = static_cast<uint64_t>(head) + 12u + zlen + 12u;
    const uint32_t status = r[2] ? kPqQualityTooLow : total > a.file_pitch ? kPngFileOverflow : 0u;
    if (status) {                                                // (uniform) no file: the neighbours' are not touched
        if (blockIdx.x == 0u && tid == 0u) { a.lengths[img] = 0u; if (a.status_out) a.status_out[img] = status; }
        return;
    }
    uint8_t* file = a.files + static_cast<size_t>(img) * a.file_pitch;
    uint8_t* idat = file + head;
    const uint8_t* src = png.body + static_cast<size_t>(img) * png.body_pitch;
    for (uint32_t i = blockIdx.x * 256u + tid; i < body; i += gridDim.x * 256u) idat[10u + i] = src[i];
    if (blockIdx.x != 0u) return;
    png_frame_idat<256>(idat, body, adler, a.zlib_header, png, img, scratch);
    if (tid == 0u) {
        pq_write_head(file, a.w, a.h, r + 8, count, n_trans);
        a.lengths[img] = static_cast<uint32_t>(total);
        if (a.status_out) a.status_out[img] = 0u;
    }
}

int pq_launch_palette(const QuantArgs& q, hipStream_t st) {
    // the tables of the images in use and all state words: one clear (an empty slot is 0)
    HIP_TRY(hipMemsetAsync(q.tables, 0, quant_table_words(q.n_images) * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(q.state, 0, static_cast<size_t>(q.n_images) * kPqStateWords * sizeof(uint32_t), st));
    const uint32_t npix = q.w * q.h, hist_blocks = std::min(256u, (npix + 1023u) / 1024u);
    for (uint32_t level = 0; level < kPqLevels; ++level)
        hipLaunchKernelGGL(pngq_histogram_kernel, dim3(hist_blocks, q.n_images), dim3(256), 0, st, q, level);
    hipLaunchKernelGGL(pngq_palette_kernel, dim3(q.n_images), dim3(kPqLanes), 0, st, q);
    return IFHIP_OK;
}

int QuantScratch::allocate(size_t n) {
    max_images = n;
    HIP_TRY(DEV_MALLOC(&d_tables, (quant_table_words(n) + n * kPqStateWords) * sizeof(uint32_t)));
    HIP_TRY(DEV_MALLOC(&d_ekey, n * kPqMaxEntries * sizeof(uint32_t)));
    HIP_TRY(DEV_MALLOC(&d_ew, n * kPqMaxEntries * sizeof(uint32_t)));
    HIP_TRY(DEV_MALLOC(&d_edmin, n * kPqMaxEntries * sizeof(uint64_t)));
    HIP_TRY(DEV_MALLOC(&d_result, n * kPqResultWords * sizeof(uint32_t)));
    return IFHIP_OK;
}

void QuantScratch::fill(QuantArgs* qp, const uint8_t* images, size_t image_bytes, uint32_t stride, uint32_t w, uint32_t h, uint32_t n_images,
                        int alpha_meaningful, uint32_t max_colors, uint32_t speed, uint32_t target, uint32_t minimum) const {
    QuantArgs& q = *qp;
    std::memset(&q, 0, sizeof q);
    q.images = images; q.image_bytes = image_bytes; q.stride = stride; q.w = w; q.h = h; q.n_images = n_images;
    q.alpha = alpha_meaningful ? 1u : 0u; q.max_colors = max_colors;
    q.iterations = pq_speed_iterations(speed); q.max_entries = pq_speed_max_entries(speed);
    q.bound_target = pq_quality_bound(target); q.bound_min = pq_quality_bound(minimum);
    q.tables = d_tables; q.state = d_tables + quant_table_words(max_images);
    q.ekey = d_ekey; q.ew = d_ew; q.edmin = d_edmin; q.result = d_result;
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_png_quant_stage {
    uint32_t width = 0, height = 0, max_images = 0;
    PngDeflateScratch deflate;
    size_t body_pitch = 0;
    uint8_t* d_body = nullptr;          // the zlib bodies, until finish knows where in the file they go
    QuantScratch quant;
    StageScratch blocks{&d_body, &quant.d_tables, &quant.d_ekey, &quant.d_ew, &quant.d_edmin, &quant.d_result};
};

namespace {
int quant_stage_allocate(ifhip_png_quant_stage* s) {
    if (int rc = s->deflate.allocate(s->max_images)) return rc;
    const size_t n = s->max_images;
    return s->blocks.ensure([&]() -> int {                       // the stage's own buffers, on the same device
        HIP_TRY(DEV_MALLOC(&s->d_body, n * s->body_pitch));
        return s->quant.allocate(n);
    });
}
int clamp_int(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
}  // namespace

extern "C" {

int ifhip_png_quant_stage_create(ifhip_png_quant_stage** stage, uint32_t width, uint32_t height, uint32_t max_images) {
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage out-pointer");
    *stage = nullptr;
    if (width == 0 || height == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (max_images == 0 || max_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 images per stage");
    const uint64_t pixels = static_cast<uint64_t>(width) * height;
    if (pixels > kPqMaxPixels) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: %llu pixels (the quantiser's error sums hold 2^28)", static_cast<unsigned long long>(pixels));
    if (height >= kPqLanes && width > kPqLastRowCols)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a frame of %u rows or more is at most %u pixels wide (the remap's error row lies in LDS)", kPqLanes, kPqLastRowCols);
    std::unique_ptr<ifhip_png_quant_stage> s(new ifhip_png_quant_stage);
    s->width = width; s->height = height; s->max_images = max_images;
    s->deflate.shape(width, 1u, height);
    s->body_pitch = (s->deflate.max_body_bytes() + 15u) & ~static_cast<size_t>(15u);
    *stage = s.release();
    return IFHIP_OK;
}

void ifhip_png_quant_stage_destroy(ifhip_png_quant_stage* stage) { delete stage; }

size_t ifhip_png_quant_stage_max_file_bytes(const ifhip_png_quant_stage* stage) {
    return stage ? stage->deflate.max_body_bytes() + kPqFramingMax : 0u;     // (the framing with a full PLTE and tRNS)
}

int ifhip_png_quantize_batch_device(ifhip_png_quant_stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, int alpha_meaningful,
                                    uint32_t n_images, int quality, int min_quality, int speed, uint32_t max_colors, int dither, int zlib_level,
                                    uint8_t* d_files, size_t file_pitch, uint32_t* d_lengths, uint32_t* d_status, uint8_t* d_palettes, uint8_t* d_indices,
                                    double* d_mse, void* hip_stream) {
    bool go = false;
    if (int rc = open_encode_batch(stage, d_images, image_bytes, stride, n_images, d_files, d_lengths, &go); rc || !go) return rc;
    if (max_colors < 2u || max_colors > kPqMaxColors) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: max_colors is 2..256");
    if (dither != 0 && dither != 1) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: dither is 0 or 1");
    if (zlib_level < -1 || zlib_level > 9) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: zlib_level is -1 or 0..9");
    if (file_pitch < kPqFramingMax + 6u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: file_pitch below %u bytes", kPqFramingMax + 6u);
    if (d_mse && (reinterpret_cast<uintptr_t>(d_mse) & 7u)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: d_mse must be 8-byte aligned");
    if (int rc = quant_stage_allocate(stage)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // PngquantEncoder::create (codecs/pngquant.rs:50-57): speed 1..10 (absent: libimagequant's 4), target 0..100 (absent: 100),
    // minimum 0..target (absent: 0)
    const uint32_t sp = static_cast<uint32_t>(clamp_int(speed < 0 ? 4 : speed, 1, 10));
    const int target = clamp_int(quality < 0 ? 100 : quality, 0, 100), minimum = clamp_int(min_quality < 0 ? 0 : min_quality, 0, target);
    QuantArgs q;
    stage->quant.fill(&q, d_images, image_bytes, stride, stage->width, stage->height, n_images, alpha_meaningful, max_colors, sp,
                      static_cast<uint32_t>(target), static_cast<uint32_t>(minimum));
    q.dither = static_cast<uint32_t>(dither); q.zlib_header = png_zlib_header(zlib_level);
    q.palettes = d_palettes; q.indices = d_indices; q.mse = d_mse;
    q.files = d_files; q.file_pitch = file_pitch; q.lengths = d_lengths; q.status_out = d_status;
    // the zlib body first lands in the stage, which has room for its worst case; finish copies it into its frame
    const PngDeflateArgs a = stage->deflate.args(n_images, zlib_level, stage->d_body, stage->body_pitch, static_cast<uint32_t>(stage->deflate.max_body_bytes() - 6u));
    if (int rc = pq_launch_palette(q, st)) return rc;
    hipLaunchKernelGGL(pngq_remap_kernel, dim3(n_images), dim3(kPqLanes), 0, st, q, a);
    png_launch_deflate(a, st);
    hipLaunchKernelGGL(pngq_finish_kernel, dim3(kPqCopyBlocks, n_images), dim3(256), 0, st, q, a);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_png_quantize(const uint8_t* bgra, uint32_t width, uint32_t height, uint32_t stride, int alpha_meaningful, int quality, int min_quality, int speed,
                       uint8_t* out, size_t capacity, size_t* len, uint32_t* status) {
    if (len && status) *status = 0;                                        // (a null `len` is refused below with nothing written)
    uint32_t word = 0;
    if (int rc = encode_host_frame(
            bgra, width, height, stride, out, capacity, len, &word, [&](ifhip_png_quant_stage** s) { return ifhip_png_quant_stage_create(s, width, height, 1); },
            ifhip_png_quant_stage_destroy, ifhip_png_quant_stage_max_file_bytes, [&](ifhip_png_quant_stage* s, const HostFrame& f, size_t pitch, uint32_t* d_len) {
                return ifhip_png_quantize_batch_device(s, f.d, f.image_bytes, stride, alpha_meaningful, 1, quality, min_quality, speed, kPqMaxColors, 1, 6,
                                                       f.side_output(), pitch, d_len, d_len + 1, nullptr, nullptr, nullptr, nullptr);
            })) return rc;
    if (status) *status = word;
    if (word == kPqQualityTooLow) return IFHIP_OK;                         // no file: the caller writes a lossless one (pngquant.rs:105-139)
    return refuse_unfitted_file(word, *len);
}

}  // extern "C"
