// white_balance.hip -- gfx950 kernels + C ABI for flow/nodes/white_balance.rs (:13-93, WhiteBalanceSrgbMutDef) with
// graphics/histogram.rs::populate_histogram_from_window: the white_balance_histogram_area_threshold_srgb node and the
// querystring's a.balancewhite key.
//
// Two launches per batch, both grid-wide with 16-byte loads:
//   histogram  each workgroup counts R, G and B of its rows into LDS -- one sub-histogram per wave, so that waves never
//              meet on an LDS address; inside a wave a lane adds a run of four equal values once, and a wave whose 256
//              pixels share one colour (a flat frame, a flat background) adds once for the wave -- then flushes them once
//              into the frame's 3 x 256 u64 counts with device-scope atomics.  Integer counts: order does not matter.
//   apply      each workgroup rebuilds the three byte maps in LDS from its frame's counts (one wave per channel: a
//              wave-wide scan of the counts, the threshold tests of area_threshold in f64, create_byte_mapping in f64),
//              then maps R, G and B; alpha keeps its value.
// f64 as the reference: `area as f64 / total as f64 > t` with t the f32 threshold widened; `high` searched with the LOW
// threshold (:33, sic); `(high - low)` a wrapping usize subtraction (release build: high < low gives a scale of about
// 1.4e-17 and maps everything to 0); high == low a scale of +inf (0 * inf = NaN, and `NaN.min(255)` is 255).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "hip_entry.hpp"

namespace ifhip {
namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kTargetBlocks = 2048;               // 256 CUs x 8 workgroups

struct Geometry {
    uint8_t* bgra;
    size_t image_bytes;
    uint32_t w, h, stride;
    uint32_t rows_per_block;                            // rows [blockIdx.x * rows_per_block, ..) of frame blockIdx.y
    uint32_t vec16;                                     // base, image_bytes and stride are multiples of 16
    unsigned long long* hist;                           // [n][3][256] R, G, B
};

// the four-pixel groups of the workgroup's rows: gpr >= 256 -> the lanes walk along each row; narrower rows -> each lane
// keeps one group column and the workgroup takes 256 / gpr rows per step
template <typename F>
__device__ __forceinline__ void for_groups(const Geometry& g, F&& body) {
    const uint32_t gpr = (g.w + 3u) >> 2;
    const uint32_t r0 = blockIdx.x * g.rows_per_block, r1 = min(g.h, r0 + g.rows_per_block);
    uint8_t* frame = g.bgra + static_cast<size_t>(blockIdx.y) * g.image_bytes;
    if (gpr >= kThreads) {
        for (uint32_t y = r0; y < r1; ++y)
            for (uint32_t c = threadIdx.x; c < gpr; c += kThreads) body(reinterpret_cast<uint32_t*>(frame + static_cast<size_t>(y) * g.stride) + 4u * c, min(4u, g.w - 4u * c));
    } else {
        const uint32_t per = kThreads / gpr, ro = threadIdx.x / gpr, c = threadIdx.x - ro * gpr;
        if (ro < per)
            for (uint32_t y = r0 + ro; y < r1; y += per) body(reinterpret_cast<uint32_t*>(frame + static_cast<size_t>(y) * g.stride) + 4u * c, min(4u, g.w - 4u * c));
    }
}

__device__ __forceinline__ uint4 load4(const Geometry& g, const uint32_t* p, uint32_t n) {
    if (g.vec16 && n == 4u) return *reinterpret_cast<const uint4*>(p);
    uint4 v{p[0], 0u, 0u, 0u};
    if (n > 1u) v.y = p[1];
    if (n > 2u) v.z = p[2];
    if (n > 3u) v.w = p[3];
    return v;
}

__global__ void __launch_bounds__(kThreads) histogram_kernel(const Geometry g) {
    __shared__ uint32_t lds[kWaves][3][256];
    for (uint32_t i = threadIdx.x; i < kWaves * 3u * 256u; i += kThreads) (&lds[0][0][0])[i] = 0u;
    __syncthreads();
    uint32_t (*mine)[256] = lds[threadIdx.x >> 6];
    for_groups(g, [&](const uint32_t* p, uint32_t n) {
        const uint4 v = load4(g, p, n);
        const uint32_t key = v.x & 0xFFFFFFu;
        const bool same = n == 4u && (v.y & 0xFFFFFFu) == key && (v.z & 0xFFFFFFu) == key && (v.w & 0xFFFFFFu) == key;
        // a wave whose every active lane holds four pixels of one colour: one add per channel for the whole wave
        const uint32_t first = __builtin_amdgcn_readfirstlane(key);
        if (__all(same && key == first)) {
            const unsigned long long act = __ballot(1);
            if (__lane_id() == static_cast<unsigned>(__ffsll(static_cast<long long>(act)) - 1)) {
                const uint32_t cnt = 4u * static_cast<uint32_t>(__popcll(act));
                atomicAdd(&mine[0][(key >> 16) & 255u], cnt);
                atomicAdd(&mine[1][(key >> 8) & 255u], cnt);
                atomicAdd(&mine[2][key & 255u], cnt);
            }
            return;
        }
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {                                  // R, G, B
            const uint32_t sh = 16u - 8u * c;
            const uint32_t b0 = (v.x >> sh) & 255u, b1 = (v.y >> sh) & 255u, b2 = (v.z >> sh) & 255u, b3 = (v.w >> sh) & 255u;
            if (n == 4u && b1 == b0 && b2 == b0 && b3 == b0) {
                atomicAdd(&mine[c][b0], 4u);
            } else {
                atomicAdd(&mine[c][b0], 1u);
                if (n > 1u) atomicAdd(&mine[c][b1], 1u);
                if (n > 2u) atomicAdd(&mine[c][b2], 1u);
                if (n > 3u) atomicAdd(&mine[c][b3], 1u);
            }
        }
    });
    __syncthreads();
    unsigned long long* out = g.hist + static_cast<size_t>(blockIdx.y) * 768u;
    for (uint32_t i = threadIdx.x; i < 768u; i += kThreads) {
        unsigned long long s = 0;
        for (uint32_t wv = 0; wv < kWaves; ++wv) s += (&lds[wv][0][0])[i];
        if (s) atomicAdd(out + i, s);
    }
}

__global__ void __launch_bounds__(kThreads) apply_kernel(const Geometry g, double threshold) {
    __shared__ uint32_t map[3][256];                     // already shifted into place: R << 16, G << 8, B
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (wv < 3u) {
        const unsigned long long* hc = g.hist + static_cast<size_t>(blockIdx.y) * 768u + wv * 256u;
        unsigned long long c[4], local = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) { c[k] = hc[4u * lane + k]; local += c[k]; }
        unsigned long long incl = local;                                  // inclusive scan over the wave
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        const unsigned long long all = __shfl(incl, 63, 64);
        const double total = static_cast<double>(static_cast<unsigned long long>(g.w) * g.h);   // pixels_sampled
        int lo = 256, hi = -1;
        unsigned long long before = incl - local;                        // sum of the bins below 4 * lane
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const int ix = static_cast<int>(4u * lane + k);
            const unsigned long long up_to = before + c[k], from = all - before;   // area from below / from above (:20-38)
            if (lo == 256 && static_cast<double>(up_to) / total > threshold) lo = ix;
            if (static_cast<double>(from) / total > threshold) hi = ix;
            before = up_to;
        }
        for (uint32_t d = 32; d > 0; d >>= 1) {                           // first bin from below, first bin from above
            lo = min(lo, __shfl_xor(lo, d, 64));
            hi = max(hi, __shfl_xor(hi, d, 64));
        }
        const uint64_t low = lo == 256 ? 0u : static_cast<uint64_t>(lo), high = hi < 0 ? 255u : static_cast<uint64_t>(hi);
        const double scale = 255.0 / static_cast<double>(high - low);     // usize subtraction: wraps when high < low
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint64_t v = 4u * lane + k;
            double r = __builtin_round(static_cast<double>(v > low ? v - low : 0u) * scale);
            r = (r != r || r > 255.0) ? 255.0 : r < 0.0 ? 0.0 : r;        // `.min(255).max(0)`: a NaN gives 255
            map[wv][v] = static_cast<uint32_t>(r) << (16u - 8u * wv);
        }
    }
    __syncthreads();
    auto m = [&](uint32_t px) { return (px & 0xFF000000u) | map[0][(px >> 16) & 255u] | map[1][(px >> 8) & 255u] | map[2][px & 255u]; };
    for_groups(g, [&](uint32_t* p, uint32_t n) {
        if (g.vec16 && n == 4u) {
            uint4 v = *reinterpret_cast<const uint4*>(p);
            v.x = m(v.x); v.y = m(v.y); v.z = m(v.z); v.w = m(v.w);
            *reinterpret_cast<uint4*>(p) = v;
        } else {
            for (uint32_t k = 0; k < n; ++k) p[k] = m(p[k]);
        }
    });
}

}  // namespace
}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_white_balance_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w, uint32_t h,
                                     uint32_t stride, float threshold, uint64_t* d_histograms, void* hip_stream) {
    if (n_images == 0) return IFHIP_OK;
    if (w == 0 || h == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (w > static_cast<uint32_t>(INT32_MAX) || h > static_cast<uint32_t>(INT32_MAX))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimension overflow");
    int rc = check_frames(d_bgra, image_bytes, w, h, stride, "bitmap");
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_histograms) & 7u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: histograms must be 8-byte aligned");
    if (n_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: more than 65535 images per launch");
    if ((rc = require_gfx950(nullptr))) return rc;
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // workgroups per frame: about kTargetBlocks in all, at least one row each, and few enough pixels per workgroup that a
    // u32 LDS count cannot overflow
    uint64_t per = std::max<uint64_t>(1u, (kTargetBlocks + n_images - 1u) / n_images);
    per = std::max<uint64_t>(per, (static_cast<uint64_t>(w) * h + 0x7FFFFFFFull) / 0x80000000ull);
    per = std::min<uint64_t>(per, h);
    Geometry g{};
    g.bgra = d_bgra; g.image_bytes = image_bytes; g.w = w; g.h = h; g.stride = stride;
    g.rows_per_block = static_cast<uint32_t>((h + per - 1u) / per);
    per = (h + g.rows_per_block - 1u) / g.rows_per_block;
    g.vec16 = ((reinterpret_cast<uintptr_t>(d_bgra) | image_bytes | stride) & 15u) == 0 ? 1u : 0u;
    const size_t hist_bytes = static_cast<size_t>(n_images) * 768u * sizeof(uint64_t);
    void* scratch = nullptr;
    if (!d_histograms) HIP_TRY(static_cast<hipError_t>(cached_malloc_for_stream(&scratch, hist_bytes, st, true)));
    g.hist = reinterpret_cast<unsigned long long*>(d_histograms ? static_cast<void*>(d_histograms) : scratch);
    hipError_t e = hipMemsetAsync(g.hist, 0, hist_bytes, st);
    const dim3 grid(static_cast<uint32_t>(per), n_images);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(histogram_kernel, grid, dim3(kThreads), 0, st, g);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(apply_kernel, grid, dim3(kThreads), 0, st, g, static_cast<double>(threshold));   // f64::from(f32)
        e = hipGetLastError();
    }
    const hipError_t fe = scratch ? static_cast<hipError_t>(cached_free_after(scratch, st)) : hipSuccess;
    HIP_TRY(e);
    HIP_TRY(fe);
    return IFHIP_OK;
}

int ifhip_white_balance(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, float threshold, uint64_t* histograms) {
    HostFrame s;
    int rc = s.up(bgra, w, h, stride, 768u * sizeof(uint64_t));
    if (rc) return rc;
    if ((rc = ifhip_white_balance_batch_device(s.d, s.image_bytes, 1, w, h, stride, threshold,
                                               reinterpret_cast<uint64_t*>(s.side_output()), nullptr))) return rc;
    return s.down(bgra, histograms);
}

}  // extern "C"
