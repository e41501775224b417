// color_profile.hip -- gfx950 kernel + C ABI for codecs/cms.rs::transform_to_srgb (called from mozjpeg_decoder.rs:409,
// libpng_decoder.rs:376 and webp.rs) on frames that already sit in HBM: the plan of csrc/color_profile.cpp applied in
// place, the arithmetic of csrc/color_profile_core.hpp.
//
// One launch, element-wise and memory-bound: 16-byte loads and stores, four pixels a lane, a dword tail for w % 4 (and for
// frames whose base, pitch or stride is not a multiple of 16).  Each workgroup stages its tables in LDS once, 40 KiB:
//   linear light   3 x 256 f32, eight copies each with copy k in the banks k, k + 8, k + 16, k + 24 (dword address =
//                  index * 8 + lane % 8): the four lanes of a 32-lane ds_read_b32 group that share a copy meet on four banks,
//                  2-way on average and 4-way at worst on random bytes, where a single copy costs about 3.5 LDS cycles a
//                  group (csrc/resample_device.hpp BankedLut; 32 copies would take 96 KiB and leave one workgroup a CU)
//   linear->sRGB   the 16384-byte table of csrc/color.cpp as it is: byte reads, about 3.5 cycles a group on random pixels
// About 16 LDS cycles per 32 pixels against some 31 clocks of HBM time for their 256 bytes.  The matrix stays in the kernel
// arguments (scalar loads).  Workgroups of 1 024 lanes, two to a CU: the CU's 32 waves behind 80 KiB of tables, filled twice.
// Measured against 256 and 512 lanes (four workgroups a CU, 16 and 32 waves) and against non-temporal loads and stores
// (DESIGN 4.14): waves in flight decide, not the tables -- random bytes run as fast as photographs.  The batch is the grid's
// y dimension.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "color_profile.hpp"
#include "color_profile_core.hpp"
#include "hip_entry.hpp"

namespace ifhip {
namespace {

constexpr uint32_t kThreads = 1024;
constexpr uint32_t kCopiesLog2 = 3, kCopies = 1u << kCopiesLog2;
constexpr uint32_t kTargetBlocks = 512;                // 256 CUs x 2 workgroups (32 waves a CU)
constexpr uint32_t kMinPixelsPerBlock = 8192;          // the 19 KiB of table reads of a workgroup against at least 32 KiB of pixels

struct Args {
    uint8_t* bgra;
    size_t image_bytes;
    uint32_t w, h, stride;
    uint32_t rows_per_block;                            // rows [blockIdx.x * rows_per_block, ..) of frame blockIdx.y
    uint32_t vec16;                                     // base, image_bytes and stride are multiples of 16
    const uint8_t* l2s;                                 // 16384 bytes in HBM
    ifhip_color_plan plan;
};
static_assert(sizeof(Args) <= 4096, "the plan travels in the kernel arguments");

struct LdsL2S {
    const uint8_t* t;
    __device__ __forceinline__ uint32_t operator[](uint32_t i) const { return t[i]; }
};

}  // namespace

__global__ void __launch_bounds__(kThreads) color_transform_kernel(const Args a) {
    __shared__ __attribute__((aligned(16))) float lin[3 * 256 * kCopies];
    __shared__ __attribute__((aligned(16))) uint8_t l2s[16384];
    for (uint32_t i = threadIdx.x; i < 768u; i += kThreads) {
        const float v = (&a.plan.linear[0][0])[i];
        const float4 v4 = make_float4(v, v, v, v);
        reinterpret_cast<float4*>(lin)[2u * i] = v4;
        reinterpret_cast<float4*>(lin)[2u * i + 1u] = v4;
    }
    for (uint32_t i = threadIdx.x; i < 1024u; i += kThreads) reinterpret_cast<uint4*>(l2s)[i] = reinterpret_cast<const uint4*>(a.l2s)[i];
    __syncthreads();
    const float* mine = lin + (threadIdx.x & (kCopies - 1u));
    const LdsL2S out{l2s};
    auto m = [&](uint32_t px) {
        const float lr = mine[((px >> 16) & 255u) << kCopiesLog2];
        const float lg = mine[(256u + ((px >> 8) & 255u)) << kCopiesLog2];
        const float lb = mine[(512u + (px & 255u)) << kCopiesLog2];
        return color_pixel(px, lr, lg, lb, a.plan.matrix, out);
    };
    // the four-pixel groups of the workgroup's rows: gpr >= 1024 -> the lanes walk along each row; narrower rows -> each
    // lane keeps one group column and the workgroup takes 1024 / gpr rows per step (as csrc/white_balance.hip)
    const uint32_t gpr = (a.w + 3u) >> 2;
    const uint32_t r0 = blockIdx.x * a.rows_per_block, r1 = min(a.h, r0 + a.rows_per_block);
    uint8_t* frame = a.bgra + static_cast<size_t>(blockIdx.y) * a.image_bytes;
    auto group = [&](uint32_t y, uint32_t c) {
        uint32_t* p = reinterpret_cast<uint32_t*>(frame + static_cast<size_t>(y) * a.stride) + 4u * c;
        const uint32_t n = min(4u, a.w - 4u * c);
        if (a.vec16 && n == 4u) {
            uint4 v = *reinterpret_cast<const uint4*>(p);
            v.x = m(v.x); v.y = m(v.y); v.z = m(v.z); v.w = m(v.w);
            *reinterpret_cast<uint4*>(p) = v;
        } else {
            for (uint32_t k = 0; k < n; ++k) p[k] = m(p[k]);
        }
    };
    if (gpr >= kThreads) {
        for (uint32_t y = r0; y < r1; ++y)
            for (uint32_t c = threadIdx.x; c < gpr; c += kThreads) group(y, c);
    } else {
        const uint32_t per = kThreads / gpr, ro = threadIdx.x / gpr, c = threadIdx.x - ro * gpr;
        if (ro < per)
            for (uint32_t y = r0 + ro; y < r1; y += per) group(y, c);
    }
}

}  // namespace ifhip

using namespace ifhip;

extern "C" {

const char* ifhip_color_plan_status_text(int status) { return color_plan_status_text(status); }

int ifhip_color_plan_from_icc(const uint8_t* icc, size_t len, ifhip_color_plan* out) {
    const ColorPlanResult r = color_plan_from_icc(icc, len, out);
    if (r.status != IFHIP_COLOR_PLANNED) (void)fail(IFHIP_INVALID_ARGUMENT, "ColorProfileError: the ICC profile is %s: %s", color_plan_status_text(r.status), r.reason);
    return r.status;
}

int ifhip_color_plan_from_gamma_primaries(double gamma, const double xy[8], ifhip_color_plan* out) {
    const ColorPlanResult r = color_plan_from_gamma_primaries(gamma, xy, out);
    if (r.status != IFHIP_COLOR_PLANNED) (void)fail(IFHIP_INVALID_ARGUMENT, "ColorProfileError: gAMA and cHRM are %s: %s", color_plan_status_text(r.status), r.reason);
    return r.status;
}

int ifhip_color_transform_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w, uint32_t h,
                                       uint32_t stride, const ifhip_color_plan* plan, void* hip_stream) {
    if (!plan) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null colour plan");
    if (n_images == 0) return IFHIP_OK;
    if (w == 0 || h == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (w > static_cast<uint32_t>(INT32_MAX) || h > static_cast<uint32_t>(INT32_MAX))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimension overflow");
    int rc = check_frames(d_bgra, image_bytes, w, h, stride, "bitmap");
    if (rc) return rc;
    if (n_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: more than 65535 images per launch");
    if ((rc = require_gfx950(nullptr))) return rc;
    Args a{};
    const float* s2l = nullptr;
    if ((rc = device_color_tables(&s2l, &a.l2s))) return rc;
    // workgroups per frame: about kTargetBlocks in all, none with less than kMinPixelsPerBlock unless the frame is smaller,
    // at least one row each
    uint64_t per = std::max<uint64_t>(1u, (kTargetBlocks + n_images - 1u) / n_images);
    per = std::min<uint64_t>(per, std::max<uint64_t>(1u, static_cast<uint64_t>(w) * h / kMinPixelsPerBlock));
    per = std::min<uint64_t>(per, h);
    a.bgra = d_bgra; a.image_bytes = image_bytes; a.w = w; a.h = h; a.stride = stride;
    a.rows_per_block = static_cast<uint32_t>((h + per - 1u) / per);
    per = (h + a.rows_per_block - 1u) / a.rows_per_block;
    a.vec16 = ((reinterpret_cast<uintptr_t>(d_bgra) | image_bytes | stride) & 15u) == 0 ? 1u : 0u;
    a.plan = *plan;
    hipLaunchKernelGGL(color_transform_kernel, dim3(static_cast<uint32_t>(per), n_images), dim3(kThreads), 0, static_cast<hipStream_t>(hip_stream), a);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_color_transform(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, const ifhip_color_plan* plan) {
    if (!plan) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null colour plan");
    HostFrame s;
    int rc = s.up(bgra, w, h, stride);
    if (rc) return rc;
    if ((rc = ifhip_color_transform_batch_device(s.d, s.image_bytes, 1, w, h, stride, plan, nullptr))) return rc;
    return s.down(bgra);
}

}  // extern "C"
