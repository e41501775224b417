// decode_handoff.hpp -- the host code that the file decoders (png_decode.hip, webp_decode.hip, gif_decode.hip) share around
// their kernels: the argument check and file walk of ifhip_*_decode_batch_device, the block a batch is staged through, and the
// frame of the synchronous host-buffer drop-in ifhip_*_decode.  A new reader brings its parse call, its layout and its kernels.
#pragma once
#include <cstring>
#include <vector>

#include "hip_entry.hpp"

namespace ifhip {

inline size_t pad16(size_t bytes) { return (bytes + 15u) & ~static_cast<size_t>(15); }

// ifhip_*_decode_batch_device behind `n_files == 0`: the argument checks, then one walk per file -- parse(file, len, i, &item)
// says whether the file gets a frame; (*ok)[i] stays null for one that does not, and the device part gives it its status word.
template <typename Item, typename Parse>
int walk_decode_batch(const uint8_t* const* files, const size_t* lens, uint32_t n_files, const void* d_frames, const void* frame_bytes, const void* strides,
                      const void* d_status, std::vector<Item>* items, std::vector<const Item*>* ok, Parse parse) {
    if (!files || !lens || !d_frames || !frame_bytes || !strides || !d_status) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    if (n_files > 65535u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..65535 files per batch");
    items->resize(n_files);
    ok->assign(n_files, nullptr);
    for (uint32_t i = 0; i < n_files; ++i) {
        if (!files[i]) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer (file %u)", i);
        if (parse(files[i], lens[i], i, &(*items)[i])) (*ok)[i] = &(*items)[i];
    }
    return IFHIP_OK;
}

// A batch's device block of `total` + 16 bytes whose first `uploaded` bytes come from the host: alloc() gives `host`, writable
// and `uploaded` bytes long (pinned where the cache has a block, pageable otherwise); send() copies it up on the stream and
// waits, so the staging block is free again on return.  The device block goes back to the cache behind the work queued on
// the stream by the end of the scope.
struct StagedBlock {
    uint8_t* block = nullptr;
    uint8_t* host = nullptr;
    explicit StagedBlock(void* hip_stream) : st(static_cast<hipStream_t>(hip_stream)) {}
    StagedBlock(const StagedBlock&) = delete;
    StagedBlock& operator=(const StagedBlock&) = delete;
    ~StagedBlock() {
        if (pin) (void)cached_host_free(pin);
        if (block) (void)cached_free_after(block, st);
    }
    int alloc(size_t total, size_t uploaded_bytes) {
        if (int rc = require_gfx950(nullptr)) return rc;
        HIP_TRY(DEV_MALLOC(&block, total + 16u));
        uploaded = uploaded_bytes;
        if (cached_host_malloc(&pin, uploaded) == 0) host = static_cast<uint8_t*>(pin);
        else { pin = nullptr; pageable.resize(uploaded); host = pageable.data(); }
        return IFHIP_OK;
    }
    int send() {
        hipError_t e = hipMemcpyAsync(block, host, uploaded, hipMemcpyHostToDevice, st);
        const hipError_t w = static_cast<hipError_t>(wait_stream(st));
        if (pin) (void)cached_host_free(pin);
        pin = nullptr;
        HIP_TRY(e);
        HIP_TRY(w);
        return IFHIP_OK;
    }

private:
    hipStream_t st;
    void* pin = nullptr;
    std::vector<uint8_t> pageable;
    size_t uploaded = 0;
};

// The destination of ifhip_*_decode: a host bitmap of w x h BGRA pixels at `stride` inside `capacity` bytes.
inline int check_decode_destination(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, size_t capacity) {
    if (!bgra) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null bitmap pointer");
    if (static_cast<uint64_t>(w) * 4u > stride || (stride & 3u)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: stride smaller than a BGRA row or not a multiple of 4");
    const uint64_t needs = static_cast<uint64_t>(h - 1u) * stride + 4ull * w;
    if (needs > capacity) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: the frame needs %llu bytes, the buffer has %zu", static_cast<unsigned long long>(needs), capacity);
    return IFHIP_OK;
}

// The device part of ifhip_*_decode on the null stream: the bitmap goes up, device(frame, image_bytes, stride, d_status)
// decodes one file into it, the bitmap and the file's status word come down.
template <typename Device>
int decode_to_host_frame(uint32_t w, uint32_t h, uint8_t* bgra, uint32_t stride, Device device, uint32_t* status) {
    HostFrame f;
    if (int rc = f.up(bgra, w, h, stride, 16u)) return rc;
    if (int rc = device(f.d, f.image_bytes, stride, reinterpret_cast<uint32_t*>(f.side_output()))) return rc;
    uint32_t side[4] = {0, 0, 0, 0};
    if (int rc = f.down(bgra, side)) return rc;
    *status = side[0];
    return IFHIP_OK;
}

}  // namespace ifhip
