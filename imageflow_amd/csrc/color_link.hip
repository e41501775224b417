// color_link.hip -- gfx950 kernels + C ABI for the sources codecs/lcms2_transform.rs converts and csrc/color_profile.hip cannot
// express: grey frames with a GRAY profile (a table of 256 bytes) and frames with a LUT-based RGB profile (a device link of
// 33^3 nodes), on frames that already sit in HBM, in place.  The links come from csrc/color_link.cpp, the arithmetic of a pixel
// from csrc/color_link_core.hpp.
//
// One launch, the frame walk of csrc/color_profile.hip: 16-byte loads and stores, four pixels a lane, a dword tail for w % 4
// (and for frames whose base, pitch or stride is not a multiple of 16), rows_per_block rows a workgroup, the batch in the
// grid's y dimension.
//   RGB link   the nodes stay in HBM, padded to 8 bytes (287 496 bytes: more than a workgroup's LDS, resident in L2); a pixel
//              reads the four nodes of its tetrahedron's walk, one 8-byte load each, and interpolates the three channels in
//              integers.  Neighbouring pixels of a photograph fall into neighbouring cells, so most loads hit the vector L1.
//              No LDS, 256 lanes a workgroup: occupancy is the registers' alone.
//   grey       the 256 bytes staged in LDS once a workgroup; one byte read a pixel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>

#include "../../include/imageflow_hip_color_link.h"
#include "color_link.hpp"
#include "color_link_core.hpp"
#include "hip_entry.hpp"

struct ifhip_color_link {
    ifhip::ColorLink host;
    std::mutex mu;                     // guards the device copy's creation
    void* d = nullptr;                 // nodes (8 bytes each) or the 256 bytes
    int device = -1;
    hipStream_t first = nullptr;       // the stream the upload was ordered on
    hipEvent_t uploaded = nullptr;
};

namespace ifhip {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTargetBlocks = 2048;               // 256 CUs x 8 workgroups of 4 waves
constexpr uint32_t kMinPixelsPerBlock = 2048;

struct Args {
    uint8_t* bgra;
    size_t image_bytes;
    uint32_t w, h, stride;
    uint32_t rows_per_block;                            // rows [blockIdx.x * rows_per_block, ..) of frame blockIdx.y
    uint32_t vec16;                                     // base, image_bytes and stride are multiples of 16
    const void* link;
};

struct DeviceNodes {
    const uint64_t* __restrict__ n;
    __device__ __forceinline__ uint64_t operator()(uint32_t i) const { return n[i]; }
};

// the four-pixel groups of the workgroup's rows: gpr >= kThreads -> the lanes walk along each row; narrower rows -> each lane
// keeps one group column and the workgroup takes kThreads / gpr rows per step (as csrc/color_profile.hip)
template <typename Pixel>
__device__ __forceinline__ void walk_frame(const Args& a, const Pixel& m) {
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

}  // namespace

__global__ void __launch_bounds__(kThreads) color_link_rgb_kernel(const Args a) {
    const DeviceNodes nodes{static_cast<const uint64_t*>(a.link)};
    walk_frame(a, [&](uint32_t px) { return link_pixel(px, nodes); });
}

__global__ void __launch_bounds__(kThreads) color_link_gray_kernel(const Args a) {
    __shared__ __attribute__((aligned(4))) uint8_t table[256];
    if (threadIdx.x < 64u) reinterpret_cast<uint32_t*>(table)[threadIdx.x] = static_cast<const uint32_t*>(a.link)[threadIdx.x];
    __syncthreads();
    walk_frame(a, [&](uint32_t px) { return link_gray_pixel(px, table); });
}

namespace {

// the link's device copy: made by the first call that needs it, ordered on that call's stream; other streams wait for the
// upload's event on the device
int device_copy(ifhip_color_link* link, hipStream_t stream, const void** out) {
    int device = -1;
    int rc = require_gfx950(&device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(link->mu);
    if (!link->d) {
        const bool gray = link->host.kind == kColorLinkGray;
        const size_t bytes = gray ? 256u : kLinkNodes * sizeof(uint64_t);
        const void* src = gray ? static_cast<const void*>(link->host.gray) : static_cast<const void*>(link->host.nodes.data());
        void* d = nullptr;
        hipEvent_t ev = nullptr;
        HIP_TRY(DEV_MALLOC(&d, bytes));
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipEventRecord(ev, stream);
        if (e != hipSuccess) {
            if (ev) (void)hipEventDestroy(ev);
            (void)DEV_FREE(d);
            return fail(IFHIP_GPU_ERROR, "GpuError: the upload of a colour link failed: %s", hipGetErrorString(e));
        }
        link->d = d; link->device = device; link->first = stream; link->uploaded = ev;
    }
    if (link->device != device) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: the colour link lives on device %d, the call runs on device %d", link->device, device);
    if (stream != link->first) HIP_TRY(hipStreamWaitEvent(stream, link->uploaded, 0));
    *out = link->d;
    return IFHIP_OK;
}

}  // namespace
}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_color_link_from_icc(const uint8_t* icc, size_t len, int frame_is_gray, ifhip_color_link** link) {
    if (!link) {
        (void)fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null colour link pointer");
        return IFHIP_COLOR_MALFORMED;
    }
    *link = nullptr;
    ifhip_color_link* l = new ifhip_color_link;
    const ColorPlanResult r = color_link_from_icc(icc, len, frame_is_gray != 0, &l->host);
    if (r.status != IFHIP_COLOR_PLANNED) {
        delete l;
        (void)fail(IFHIP_INVALID_ARGUMENT, "ColorProfileError: the ICC profile is %s: %s", color_plan_status_text(r.status), r.reason);
        return r.status;
    }
    *link = l;
    return IFHIP_COLOR_PLANNED;
}

void ifhip_color_link_free(ifhip_color_link* link) {
    if (!link) return;
    if (link->d) (void)DEV_FREE(link->d);               // waits for the device: no launch still reads the copy
    if (link->uploaded) (void)hipEventDestroy(link->uploaded);
    delete link;
}

int ifhip_color_link_kind(const ifhip_color_link* link) { return link ? link->host.kind : 0; }

int ifhip_color_link_copy_nodes(const ifhip_color_link* link, void* out, size_t capacity, size_t* written) {
    if (!link || !out) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null colour link or buffer");
    const bool gray = link->host.kind == kColorLinkGray;
    const size_t bytes = gray ? 256u : kLinkNodes * 3u * sizeof(uint16_t);
    if (capacity < bytes) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: the link's contents need %zu bytes, the buffer has %zu", bytes, capacity);
    if (gray) {
        std::memcpy(out, link->host.gray, 256);
    } else {
        uint16_t* o = static_cast<uint16_t*>(out);
        for (uint32_t i = 0; i < kLinkNodes; ++i)
            for (uint32_t c = 0; c < 3u; ++c) o[3u * i + c] = static_cast<uint16_t>(link->host.nodes[i] >> (16u * c));
    }
    if (written) *written = bytes;
    return IFHIP_OK;
}

int ifhip_color_link_transform_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w, uint32_t h,
                                            uint32_t stride, ifhip_color_link* link, void* hip_stream) {
    if (!link) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null colour link");
    if (n_images == 0) return IFHIP_OK;
    if (w == 0 || h == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (w > static_cast<uint32_t>(INT32_MAX) || h > static_cast<uint32_t>(INT32_MAX))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimension overflow");
    int rc = check_frames(d_bgra, image_bytes, w, h, stride, "bitmap");
    if (rc) return rc;
    if (n_images > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: more than 65535 images per launch");
    Args a{};
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if ((rc = device_copy(link, stream, &a.link))) return rc;
    // workgroups per frame: about kTargetBlocks in all, none with less than kMinPixelsPerBlock unless the frame is smaller,
    // at least one row each
    uint64_t per = std::max<uint64_t>(1u, (kTargetBlocks + n_images - 1u) / n_images);
    per = std::min<uint64_t>(per, std::max<uint64_t>(1u, static_cast<uint64_t>(w) * h / kMinPixelsPerBlock));
    per = std::min<uint64_t>(per, h);
    a.bgra = d_bgra; a.image_bytes = image_bytes; a.w = w; a.h = h; a.stride = stride;
    a.rows_per_block = static_cast<uint32_t>((h + per - 1u) / per);
    per = (h + a.rows_per_block - 1u) / a.rows_per_block;
    a.vec16 = ((reinterpret_cast<uintptr_t>(d_bgra) | image_bytes | stride) & 15u) == 0 ? 1u : 0u;
    const dim3 grid(static_cast<uint32_t>(per), n_images);
    if (link->host.kind == kColorLinkGray) hipLaunchKernelGGL(color_link_gray_kernel, grid, dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL(color_link_rgb_kernel, grid, dim3(kThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

int ifhip_color_link_transform(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, ifhip_color_link* link) {
    if (!link) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null colour link");
    HostFrame s;
    int rc = s.up(bgra, w, h, stride);
    if (rc) return rc;
    if ((rc = ifhip_color_link_transform_batch_device(s.d, s.image_bytes, 1, w, h, stride, link, nullptr))) return rc;
    return s.down(bgra);
}

}  // extern "C"
