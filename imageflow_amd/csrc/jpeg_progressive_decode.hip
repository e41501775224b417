// jpeg_progressive_decode.hip -- progressive (SOF2) Huffman JPEG entropy decoding on gfx950: the kernels and the entry points
// of include/imageflow_hip_jpeg_progressive.h.  The algorithm is stated once, in jpeg_progressive_core.hpp (which also says
// what bounds each access); the host front end is jpeg_progressive_read.cpp.  Here: the wave as the device has it, the two
// kernels, the batch's hand-off.
//
// Launches.  One clear of the planes (progressive writes are sparse, a component may have no AC scan at all; it also zeroes
// the status words), then ONE launch per dependency level with every stream of that level of every file of the batch: scans of
// one level never touch the same coefficient bit, so their streams run side by side, and a level reads what the level before
// completed because launches on one stream are ordered.  The count depends on the deepest level of the batch, not on its files
// or scans (Pillow's and this library's scripts: 3 levels).
//
// A workgroup is one wave and decodes one stream.  LDS: up to three Huffman tables (an interleaved DC scan; 3 x 2448 bytes) and
// the stream's stage of 1024 words, 11 440 bytes in all: LDS admits 14 such workgroups a CU (the compiler's figure: 4 waves a
// SIMD), 34 VGPRs, no scratch.  Occupancy is not what limits it: the walk is latency-bound (a chain of readlane / scalar steps
// per symbol), streams are what there is to run side by side, and a file without restart markers has ten.  Values go to the
// planes with ordinary vector stores.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/imageflow_hip_jpeg_progressive.h"
#include "decode_handoff.hpp"
#include "jpeg_progressive_read.hpp"

namespace ifhip {

static_assert(IFHIP_JPEG_PROG_NO_SUCH_CODE == kProgNoSuchCode && IFHIP_JPEG_PROG_PAST_SE == kProgPastSe && IFHIP_JPEG_PROG_REFINE_SIZE == kProgRefineSize &&
              IFHIP_JPEG_PROG_OUT_OF_BITS == kProgOutOfBits && IFHIP_JPEG_PROG_BOUNDS == kProgBounds, "the header's status words are the core's");

struct ProgDevWave {
    template <typename T> struct Var {
        T v;
        __device__ __forceinline__ T& operator[](uint32_t) { return v; }
        // lane `lane` (wave-uniform) of the value, in a scalar register
        __device__ __forceinline__ T read(uint32_t lane) const {
            return static_cast<T>(__builtin_amdgcn_readlane(static_cast<int>(v), __builtin_amdgcn_readfirstlane(static_cast<int>(lane))));
        }
    };
    template <typename F> __device__ __forceinline__ void lanes(F f) { f(threadIdx.x); }
    template <typename F> __device__ __forceinline__ uint64_t ballot(F f) { return __ballot(f(threadIdx.x)); }
    __device__ __forceinline__ void sync() { __syncthreads(); }          // the workgroup is this one wave
    __device__ __forceinline__ void raise(uint32_t* word, uint32_t flags) { if (threadIdx.x == 0u) atomicOr(word, flags); }
};

constexpr uint32_t kProgClearThreads = 256;

__global__ __launch_bounds__(kProgClearThreads) void jpeg_progressive_clear_kernel(const ProgArgs a) {
    prog_clear_thread(a, blockIdx.y / 3u, blockIdx.y % 3u, static_cast<uint64_t>(blockIdx.x) * kProgClearThreads + threadIdx.x,
                      static_cast<uint64_t>(gridDim.x) * kProgClearThreads);
}

__global__ __launch_bounds__(kProgWave) void jpeg_progressive_level_kernel(const ProgArgs a, const uint32_t first) {
    __shared__ alignas(16) uint8_t scratch[kProgScratchBytes];
    ProgDevWave w;
    prog_stream_workgroup(w, a, first + blockIdx.x, scratch);
}

static int prog_decode_launch(const ProgPrepared* const* files, uint32_t n, void* const* coef, const size_t* plane_bytes, uint32_t* d_status, void* hip_stream) {
    ProgLayout L;
    if (!prog_layout_batch(files, n, coef, plane_bytes, &L))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: a coefficient plane is null, not 8-byte aligned or smaller than blocks_w * blocks_h * 128 bytes");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StagedBlock staged(st);
    if (int rc = staged.alloc(L.blob.size(), L.blob.size())) return rc;
    std::memcpy(staged.host, L.blob.data(), L.blob.size());
    if (int rc = staged.send()) return rc;
    const ProgArgs a = L.args(staged.block, d_status);
    const char* stop = debug_switch("jpeg_progressive_stop_after");     // tools/bench_jpeg_progressive_decode.py: the launches' times by difference
    const long stop_after = stop ? std::strtol(stop, nullptr, 10) : 1000000L;     // 0: the clear alone, k: the first k levels
    const uint32_t clear_x = static_cast<uint32_t>(std::min<uint64_t>((L.max_plane_blocks * 16u + kProgClearThreads - 1u) / kProgClearThreads, 1024u));
    hipLaunchKernelGGL(jpeg_progressive_clear_kernel, dim3(std::max(clear_x, 1u), n * 3u), dim3(kProgClearThreads), 0, st, a);
    for (uint32_t l = 0; l + 1u < L.level_first.size() && static_cast<long>(l) < stop_after; ++l) {
        const uint32_t first = L.level_first[l], count = L.level_first[l + 1u] - first;
        if (count) hipLaunchKernelGGL(jpeg_progressive_level_kernel, dim3(count), dim3(kProgWave), 0, st, a, first);
    }
    HIP_TRY(hipGetLastError());
    return IFHIP_OK;
}

}  // namespace ifhip

using namespace ifhip;

struct ifhip_jpeg_progressive_prepared { ProgPrepared P; };

extern "C" {

int ifhip_jpeg_progressive_prepare(ifhip_jpeg_progressive_prepared** prepared, const uint8_t* jpeg, size_t len) {
    if (!prepared) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    *prepared = nullptr;
    if (!jpeg) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    try {
        auto h = std::make_unique<ifhip_jpeg_progressive_prepared>();
        if (int rc = prog_prepare(jpeg, len, &h->P)) return rc;
        *prepared = h.release();
        return IFHIP_OK;
    } catch (const std::bad_alloc&) { return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: host memory");
    } catch (const std::exception& ex) { return fail(IFHIP_INVALID_STATE, "InvalidState: %s", ex.what()); }
}

int ifhip_jpeg_progressive_prepared_info(const ifhip_jpeg_progressive_prepared* prepared, uint32_t* width, uint32_t* height, int* n_components,
                                         uint8_t* h_samp3, uint8_t* v_samp3, uint32_t* blocks_w3, uint32_t* blocks_h3, uint16_t* qt3x64,
                                         uint32_t* n_scans, uint32_t* n_streams, uint32_t* n_levels) {
    if (!prepared) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null prepared file");
    const ProgPrepared& P = prepared->P;
    if (width) *width = P.width;
    if (height) *height = P.height;
    if (n_components) *n_components = static_cast<int>(P.ncomp);
    for (uint32_t c = 0; c < 3; ++c) {
        const bool has = c < P.ncomp;
        if (h_samp3) h_samp3[c] = has ? P.hs[c] : 0;
        if (v_samp3) v_samp3[c] = has ? P.vs[c] : 0;
        if (blocks_w3) blocks_w3[c] = has ? P.bw[c] : 0;
        if (blocks_h3) blocks_h3[c] = has ? P.bh[c] : 0;
        if (qt3x64) { if (has) std::memcpy(qt3x64 + 64 * c, P.qt[c], 128); else std::memset(qt3x64 + 64 * c, 0, 128); }
    }
    if (n_scans) *n_scans = static_cast<uint32_t>(P.scans.size());
    if (n_streams) *n_streams = static_cast<uint32_t>(P.streams.size());
    if (n_levels) *n_levels = P.n_levels;
    return IFHIP_OK;
}

void ifhip_jpeg_progressive_prepared_destroy(ifhip_jpeg_progressive_prepared* prepared) { delete prepared; }

int ifhip_jpeg_progressive_decode_batch_device(const ifhip_jpeg_progressive_prepared* const* prepared, uint32_t n_files, int16_t* const* d_coef0,
                                               int16_t* const* d_coef1, int16_t* const* d_coef2, const size_t* plane_bytes, uint32_t* d_status,
                                               void* hip_stream) {
    if (n_files == 0) return IFHIP_OK;
    if (!prepared || !d_coef0 || !d_coef1 || !d_coef2 || !plane_bytes || !d_status) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    if (n_files > 16384u) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: 1..16384 files per batch");
    try {
        std::vector<const ProgPrepared*> files(n_files);
        std::vector<void*> coef(3u * n_files);
        for (uint32_t i = 0; i < n_files; ++i) {
            if (!prepared[i]) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null prepared file (file %u)", i);
            files[i] = &prepared[i]->P;
            coef[3u * i] = d_coef0[i]; coef[3u * i + 1u] = d_coef1[i]; coef[3u * i + 2u] = d_coef2[i];
        }
        return prog_decode_launch(files.data(), n_files, coef.data(), plane_bytes, d_status, hip_stream);
    } catch (const std::bad_alloc&) { return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: host memory");
    } catch (const std::exception& ex) { return fail(IFHIP_INVALID_STATE, "InvalidState: %s", ex.what()); }
}

int ifhip_jpeg_progressive_decode(const uint8_t* jpeg, size_t len, int16_t* coef0, int16_t* coef1, int16_t* coef2, uint16_t* qt3x64, uint32_t* status) {
    if (status) *status = 0;
    if (!jpeg) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    try {
        ProgPrepared P;
        if (int rc = prog_prepare(jpeg, len, &P)) return rc;
        int16_t* host[3] = {coef0, coef1, coef2};
        size_t bytes[3] = {0, 0, 0}, off[3] = {0, 0, 0}, total = 0;
        for (uint32_t c = 0; c < P.ncomp; ++c) {
            if (!host[c]) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null coefficient plane");
            bytes[c] = static_cast<size_t>(P.bw[c]) * P.bh[c] * 128u;
            off[c] = total;
            total += pad16(bytes[c]);
        }
        if (int rc = require_gfx950(nullptr)) return rc;
        DeviceBlock block;
        HIP_TRY(block.alloc(total + 16u));
        uint8_t* d = block.as<uint8_t>();
        void* coef[3] = {nullptr, nullptr, nullptr};
        for (uint32_t c = 0; c < P.ncomp; ++c) coef[c] = d + off[c];
        const ProgPrepared* file = &P;
        if (int rc = prog_decode_launch(&file, 1, coef, bytes, reinterpret_cast<uint32_t*>(d + total), nullptr)) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        uint32_t word = 0;
        HIP_TRY(hipMemcpy(&word, d + total, 4, hipMemcpyDeviceToHost));
        for (uint32_t c = 0; c < P.ncomp; ++c) HIP_TRY(hipMemcpy(host[c], d + off[c], bytes[c], hipMemcpyDeviceToHost));
        if (qt3x64) for (uint32_t c = 0; c < P.ncomp; ++c) std::memcpy(qt3x64 + 64 * c, P.qt[c], 128);
        if (status) *status = word;
        else if (word) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: progressive JPEG entropy data (status %u)", word);
        return IFHIP_OK;
    } catch (const std::bad_alloc&) { return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: host memory");
    } catch (const std::exception& ex) { return fail(IFHIP_INVALID_STATE, "InvalidState: %s", ex.what()); }
}

}  // extern "C"
