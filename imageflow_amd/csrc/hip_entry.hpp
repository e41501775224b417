// hip_entry.hpp -- the host code around the kernel launches of the C entry points, for the translation units that include
// hip_runtime.h (common.hpp stays free of it): the status of a failed HIP call, the check of a batch of BGRA frames, and
// the device memory of the synchronous host-buffer drop-ins, taken from the devmem.cpp cache like every other block.
// What the file decoders share on top of this (batch check, staged block, drop-in frame) is in decode_handoff.hpp, what
// the file coders share (the opening of a batch, the drop-in that brings a file down) in encode_handoff.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.hpp"

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return fail(IFHIP_GPU_ERROR, "GpuError: %s failed: %s", #expr, hipGetErrorString(e__));     \
    } while (0)

namespace ifhip {

// Frame i of a batch starts at p + i * image_bytes: 4-byte aligned rows of at least 4*w bytes, and the frame, (h-1) rows
// of `stride` and one of 4*w bytes, inside its image_bytes.  What an op does with empty frames or batches, and the caps
// of its launch grid, are the op's own checks.
inline int check_frames(const void* p, size_t image_bytes, uint32_t w, uint32_t h, uint32_t stride, const char* what) {
    if (!p) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null %s pointer", what);
    if (static_cast<uint64_t>(w) * 4u > stride || (stride & 3u) || (image_bytes & 3u) || (reinterpret_cast<uintptr_t>(p) & 3u))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: %s rows must be 4-byte aligned and stride >= 4*w", what);
    if (h > 0 && static_cast<uint64_t>(h - 1u) * stride + 4ull * w > image_bytes)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: image_bytes %zu is smaller than %u rows of stride %u", image_bytes, h, stride);
    return IFHIP_OK;
}

// A device block that goes back to the cache at the end of the scope (cached_free: after a wait for the device).
struct DeviceBlock {
    void* p = nullptr;
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock&) = delete;
    DeviceBlock& operator=(const DeviceBlock&) = delete;
    ~DeviceBlock() { (void)cached_free(p); }
    hipError_t alloc(size_t bytes) { return DEV_MALLOC(&p, bytes); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// One host bitmap staged through HBM around a device call: image_bytes = h*stride rounded up to 16, then `side` bytes for
// a side output of the call (a rectangle, histograms).  up() uploads the frame's valid bytes, (h-1)*stride + 4*w; down()
// waits for the null stream and copies them back to `host` and the side output to `side_out` (either may be null).
struct HostFrame {
    DeviceBlock block;
    uint8_t* d = nullptr;
    size_t image_bytes = 0, valid = 0, side = 0;
    uint8_t* side_output() const { return d + image_bytes; }
    int up(const uint8_t* host, uint32_t w, uint32_t h, uint32_t stride, size_t side_bytes = 0) {
        if (w == 0 || h == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
        if (!host) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null bitmap pointer");
        if (static_cast<uint64_t>(w) * 4u > stride || (stride & 3u))
            return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: stride smaller than a BGRA row or not a multiple of 4");
        valid = static_cast<size_t>(h - 1u) * stride + static_cast<size_t>(w) * 4u;
        image_bytes = (static_cast<size_t>(h) * stride + 15u) & ~static_cast<size_t>(15);
        side = side_bytes;
        if (int rc = require_gfx950(nullptr)) return rc;
        HIP_TRY(block.alloc(image_bytes + side));
        d = block.as<uint8_t>();
        HIP_TRY(hipMemcpy(d, host, valid, hipMemcpyHostToDevice));
        return IFHIP_OK;
    }
    int down(uint8_t* host, void* side_out = nullptr) const {
        HIP_TRY(hipStreamSynchronize(nullptr));
        if (host) HIP_TRY(hipMemcpy(host, d, valid, hipMemcpyDeviceToHost));
        if (side_out) HIP_TRY(hipMemcpy(side_out, side_output(), side, hipMemcpyDeviceToHost));
        return IFHIP_OK;
    }
    // For a side output that is a coded file of `pitch` bytes, then its length, then its status word: waits, reads the two
    // words and, where there is a file (status 0), copies it to `out` (null: the length alone) when `capacity` holds it.
    int down_file(size_t pitch, uint8_t* out, size_t capacity, size_t* len, uint32_t* status) const {
        HIP_TRY(hipStreamSynchronize(nullptr));
        uint32_t len_status[2] = {0, 0};
        HIP_TRY(hipMemcpy(len_status, side_output() + pitch, 8, hipMemcpyDeviceToHost));
        *status = len_status[1];
        *len = len_status[1] ? 0u : len_status[0];
        if (!*len || !out) return IFHIP_OK;
        if (capacity < *len) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: the file needs %zu bytes, the buffer has %zu", *len, capacity);
        HIP_TRY(hipMemcpy(out, side_output(), *len, hipMemcpyDeviceToHost));
        return IFHIP_OK;
    }
};

}  // namespace ifhip
