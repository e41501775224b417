// bandwidth_probes.cpp -- measurement tools of the C ABI: HBM copy / read / mixed read-write bandwidth, and the average
// duration of back-to-back resample launches between two events.  Nothing here plans or stages a resample.
#include <algorithm>

#include "hip_entry.hpp"

namespace ifhip {
hipError_t launch_read_probe(const uint8_t* d, size_t bytes, uint32_t* sink, hipStream_t st);
hipError_t launch_mix_probe(const uint8_t* d, uint8_t* out, size_t bytes, uint32_t every, uint32_t* sink, hipStream_t st);
}  // namespace ifhip

using namespace ifhip;

namespace {
int require_device() {                 // a gfx950 device, with the message every resample entry point gives without one
    const float* s2l = nullptr;
    const uint8_t* l2s = nullptr;
    return device_color_tables(&s2l, &l2s);
}
}  // namespace

namespace {
// Scope guards: every early return of an entry point releases what it created.
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create() {
        hipError_t e = hipEventCreate(&e0);
        return e != hipSuccess ? e : hipEventCreate(&e1);
    }
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};
struct DeviceBuffer {
    void* p = nullptr;
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
};
}  // namespace

extern "C" {

int ifhip_time_scale_and_render_batch_device(const ifhip_resample_plan* plan, const uint8_t* d_in,
                                             size_t in_image_bytes, uint32_t in_stride, int in_alpha_meaningful,
                                             uint32_t n_images, uint8_t* d_canvas, size_t canvas_image_bytes,
                                             uint32_t canvas_w, uint32_t canvas_h, uint32_t canvas_stride, uint32_t x,
                                             uint32_t y, int working_space, int compositing, uint32_t matte_bgra,
                                             int force_kernel, void* hip_stream, int launches,
                                             float* avg_ms_per_launch) {
    if (launches < 1 || !avg_ms_per_launch) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: launches/avg pointer");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    EventPair ev;
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.e0, st));
    int rc = IFHIP_OK;
    for (int i = 0; i < launches && rc == IFHIP_OK; ++i)
        rc = ifhip_scale_and_render_batch_device(plan, d_in, in_image_bytes, in_stride, in_alpha_meaningful, n_images, d_canvas,
                                                 canvas_image_bytes, canvas_w, canvas_h, canvas_stride, x, y, working_space, compositing,
                                                 matte_bgra, nullptr, force_kernel, st);
    hipError_t er = hipEventRecord(ev.e1, st);
    if (er == hipSuccess) er = hipEventSynchronize(ev.e1);
    float ms = 0.f;
    if (er == hipSuccess) er = hipEventElapsedTime(&ms, ev.e0, ev.e1);
    if (rc) return rc;
    if (er != hipSuccess) return fail(IFHIP_GPU_ERROR, "GpuError: event timing failed: %s", hipGetErrorString(er));
    *avg_ms_per_launch = ms / static_cast<float>(launches);
    return IFHIP_OK;
}

int ifhip_measure_copy_bandwidth(size_t bytes, int iters, double* bytes_per_second) {
    if (!bytes_per_second || iters < 1 || bytes == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: copy bandwidth probe");
    if (int rc = require_device()) return rc;
    DeviceBuffer a, b;
    HIP_TRY(a.alloc(bytes));
    HIP_TRY(b.alloc(bytes));
    HIP_TRY(hipMemset(a.p, 1, bytes));
    HIP_TRY(hipMemcpy(b.p, a.p, bytes, hipMemcpyDeviceToDevice));
    EventPair ev;
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.e0, nullptr));
    for (int i = 0; i < iters; ++i) HIP_TRY(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, nullptr));
    HIP_TRY(hipEventRecord(ev.e1, nullptr));
    HIP_TRY(hipEventSynchronize(ev.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *bytes_per_second = 2.0 * static_cast<double>(bytes) * iters / (static_cast<double>(ms) * 1e-3);
    return IFHIP_OK;
}

int ifhip_measure_read_bandwidth(size_t bytes, int iters, double* bytes_per_second) {
    if (!bytes_per_second || iters < 1 || bytes < (1u << 20)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: read bandwidth probe");
    if (int rc = require_device()) return rc;
    bytes &= ~static_cast<size_t>(4095);
    DeviceBuffer a, sink;
    HIP_TRY(a.alloc(bytes));
    HIP_TRY(sink.alloc(4096));
    HIP_TRY(hipMemset(a.p, 1, bytes));
    HIP_TRY(hipMemset(sink.p, 0, 4096));
    HIP_TRY(launch_read_probe(static_cast<const uint8_t*>(a.p), bytes, static_cast<uint32_t*>(sink.p), nullptr));   // warm-up
    EventPair ev;
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.e0, nullptr));
    for (int i = 0; i < iters; ++i) HIP_TRY(launch_read_probe(static_cast<const uint8_t*>(a.p), bytes, static_cast<uint32_t*>(sink.p), nullptr));
    HIP_TRY(hipEventRecord(ev.e1, nullptr));
    HIP_TRY(hipEventSynchronize(ev.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *bytes_per_second = static_cast<double>(bytes) * iters / (static_cast<double>(ms) * 1e-3);
    return IFHIP_OK;
}

int ifhip_measure_mixed_bandwidth(size_t read_bytes, uint32_t read_vectors_per_write, int iters, double* bytes_per_second) {
    if (!bytes_per_second || iters < 1 || read_bytes < (1u << 20) || read_vectors_per_write < 1u)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: mixed bandwidth probe");
    if (int rc = require_device()) return rc;
    read_bytes &= ~static_cast<size_t>(4095);
    const size_t write_cap = read_bytes / read_vectors_per_write + (static_cast<size_t>(64) << 20);   // every workgroup's span keeps its own output span
    DeviceBuffer a, out, sink;
    HIP_TRY(a.alloc(read_bytes));
    HIP_TRY(out.alloc(std::max(write_cap, read_bytes)));
    HIP_TRY(sink.alloc(8192));
    HIP_TRY(hipMemset(a.p, 1, read_bytes));
    HIP_TRY(hipMemset(sink.p, 0, 8192));
    HIP_TRY(launch_mix_probe(static_cast<const uint8_t*>(a.p), static_cast<uint8_t*>(out.p), read_bytes, read_vectors_per_write, static_cast<uint32_t*>(sink.p), nullptr));   // warm-up
    EventPair ev;
    HIP_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.e0, nullptr));
    for (int i = 0; i < iters; ++i)
        HIP_TRY(launch_mix_probe(static_cast<const uint8_t*>(a.p), static_cast<uint8_t*>(out.p), read_bytes, read_vectors_per_write, static_cast<uint32_t*>(sink.p), nullptr));
    HIP_TRY(hipEventRecord(ev.e1, nullptr));
    HIP_TRY(hipEventSynchronize(ev.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    uint32_t stores_per_lane = 0;
    HIP_TRY(hipMemcpy(&stores_per_lane, static_cast<const uint32_t*>(sink.p) + 1024, 4, hipMemcpyDeviceToHost));
    const double written = static_cast<double>(stores_per_lane) * 16.0 * 1024.0 * (256.0 * 8.0);
    *bytes_per_second = (static_cast<double>(read_bytes) + written) * iters / (static_cast<double>(ms) * 1e-3);
    return IFHIP_OK;
}

}  // extern "C"
