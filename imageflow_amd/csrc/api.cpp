// api.cpp -- the C ABI of libimageflow_hip.so (include/imageflow_hip.h) over the gfx950 resample kernels.
//
// Host responsibilities only: argument validation with the reference's error kinds (graphics/scaling.rs:24-48), the device
// copies of a plan's tables, the launch of what the planner chose (resample_plan.cpp decides kernel and geometry; nothing
// in it touches the device), the process-wide plan cache, and HBM staging for the host-buffer drop-in entry points.  No
// pixel arithmetic happens on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "hip_entry.hpp"
#include "resample_plan.hpp"

namespace ifhip {
hipError_t launch_fused(const ResampleArgs& a, int slots, bool alpha, bool per_pixel, uint32_t grid, uint32_t block,
                        size_t lds, hipStream_t st);
hipError_t launch_generic(const ResampleArgs& a, bool alpha, float4* scratch, uint32_t img0, uint32_t n_img,
                          hipStream_t st);
hipError_t launch_banded(const ResampleArgs& a, bool alpha, const BandedArgs& b, uint32_t grid_x, size_t lds, hipStream_t st);
hipError_t launch_apply_matte(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w, uint32_t h,
                              uint32_t stride, uint32_t matte, float mb, float mg, float mr, float ma,
                              const float* s2l, const uint8_t* l2s, hipStream_t st);
}  // namespace ifhip

using namespace ifhip;

namespace {
// ---- per-device colour tables -----------------------------------------------------------------------
struct DeviceTables {
    float* s2l = nullptr;
    float* s2f = nullptr;
    uint8_t* l2s = nullptr;
    uint16_t* l2s_thr = nullptr;
};
std::mutex g_dev_mu;
std::map<int, DeviceTables> g_dev_tables;

int device_tables(DeviceTables* out) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0)
        return fail(IFHIP_GPU_UNAVAILABLE, "GpuUnavailable: no HIP device (hipGetDevice failed); this library has no CPU path");
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = g_dev_tables.find(dev);
    if (it == g_dev_tables.end()) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(IFHIP_GPU_UNAVAILABLE, "GpuUnavailable: device %d is %s, this library is built for gfx950 only", dev, prop.gcnArchName);
        const ColorTables& t = color_tables();
        DeviceTables d;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d.s2l), sizeof t.s2l));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d.s2f), sizeof t.s2f));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d.l2s), sizeof t.l2s));
        HIP_TRY(hipMemcpy(d.s2l, t.s2l, sizeof t.s2l, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.s2f, t.s2f, sizeof t.s2f, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.l2s, t.l2s, sizeof t.l2s, hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d.l2s_thr), sizeof t.l2s_thr));
        HIP_TRY(hipMemcpy(d.l2s_thr, t.l2s_thr, sizeof t.l2s_thr, hipMemcpyHostToDevice));
        it = g_dev_tables.emplace(dev, d).first;
    }
    *out = it->second;
    return IFHIP_OK;
}

template <typename T>
int upload(const std::vector<T>& v, T** out) {
    *out = nullptr;
    if (v.empty()) return IFHIP_OK;
    HIP_TRY(DEV_MALLOC(out, v.size() * sizeof(T)));
    HIP_TRY(static_cast<hipError_t>(copy_to_device(*out, v.data(), v.size() * sizeof(T))));
    return IFHIP_OK;
}

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------
struct ifhip_resample_plan {
    int device = -1;
    PlanTables t;                   // the host tables; below, their device copies
    uint32_t *d_v_left = nullptr, *d_v_count = nullptr, *d_v_off = nullptr;
    uint32_t *d_h_left = nullptr, *d_h_count = nullptr, *d_h_off = nullptr;
    float *d_v_w = nullptr, *d_h_w = nullptr, *d_h_wu = nullptr, *d_h_wg = nullptr, *d_h_wg2 = nullptr;
    uint4* d_h_meta = nullptr;
    uint32_t *d_h_meta2 = nullptr, *d_h_meta3 = nullptr;
    Strip* d_strips[2] = {nullptr, nullptr};        // [in_alpha_meaningful]

    ~ifhip_resample_plan() {
        for (void* p : {(void*)d_v_left, (void*)d_v_count, (void*)d_v_off, (void*)d_h_left, (void*)d_h_count,
                        (void*)d_h_off, (void*)d_v_w, (void*)d_h_w, (void*)d_h_wu, (void*)d_h_meta, (void*)d_h_wg, (void*)d_h_meta2, (void*)d_h_wg2, (void*)d_h_meta3, (void*)d_strips[0],
                        (void*)d_strips[1]})
            if (p) (void)DEV_FREE(p);
        for (auto& kv : t.schedules) {
            if (kv.second.d_steps) (void)DEV_FREE(kv.second.d_steps);
            if (kv.second.d_band_begin) (void)DEV_FREE(kv.second.d_band_begin);
        }
    }
};

namespace {

bool trace_launch() { return debug_switch("trace_launch") != nullptr; }      // one stderr line per launch: its geometry (tools/)

// The device copy of a planned schedule, uploaded the first time it is launched.
int schedule_on_device(const PlanTables& t, PlannedSchedule* s) {
    std::lock_guard<std::mutex> lk(t.mu);
    if (s->d_steps) return IFHIP_OK;
    VStep* steps = nullptr;
    int rc = upload(s->host.steps, &steps);
    if (rc) return rc;
    rc = upload(s->host.band_begin, &s->d_band_begin);
    if (rc) { (void)DEV_FREE(steps); return rc; }
    s->d_steps = steps;
    return IFHIP_OK;
}

int validate_render(uint32_t in_w, uint32_t in_h, uint32_t in_stride, uint32_t cw, uint32_t ch, uint32_t c_stride,
                    uint32_t x, uint32_t y, uint32_t w, uint32_t h, int working_space, int compositing, uint32_t in_px_bytes = 4) {
    if (static_cast<uint64_t>(h) + y > ch || static_cast<uint64_t>(w) + x > cw)                 // scaling.rs:24-29
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Destination rectangle for scale2d is out of bounds");
    if (w == 0 || h == 0 || in_w == 0 || in_h == 0)                                              // bitmaps.rs:700-702
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (static_cast<uint64_t>(in_w) * in_px_bytes > in_stride || static_cast<uint64_t>(cw) * 4u > c_stride)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: stride smaller than a BGRA row");
    if (c_stride & 3u)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: canvas stride must be a multiple of 4 bytes");
    if (working_space != IFHIP_SPACE_SRGB && working_space != IFHIP_SPACE_LINEAR)
        return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: working floatspace %d", working_space);
    if (compositing < IFHIP_REPLACE_SELF || compositing > IFHIP_BLEND_WITH_MATTE)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: compositing mode %d", compositing);
    return IFHIP_OK;
}

int enqueue_batch(const ifhip_resample_plan* p, const uint8_t* d_in, size_t in_image_bytes, uint32_t in_stride,
                  int alpha, uint32_t n_images, uint8_t* d_canvas, size_t canvas_image_bytes, uint32_t cw, uint32_t ch,
                  uint32_t c_stride, uint32_t x, uint32_t y, int working_space, int compositing, uint32_t matte,
                  float* d_f32, int force_kernel, hipStream_t st, const uint8_t* d_cb = nullptr, const uint8_t* d_cr = nullptr,
                  bool probe = false) {
    // probe (planar source only): everything up to the launch -- IFHIP_OK means the real call will run the fused kernel
    // d_cb / d_cr: planar YCbCr source (d_in = the Y plane, in_stride = sample pitch, in_image_bytes = plane size).  That form
    // exists only on the fused kernel: kNotFusable tells the caller to go through a BGRA bitmap instead.
    if (!p) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null plan");
    const PlanTables& t = p->t;
    const bool ycc = d_cb != nullptr;
    int rc = validate_render(t.in_w, t.in_h, in_stride, cw, ch, c_stride, x, y, t.out_w, t.out_h, working_space, compositing, ycc ? 1u : 4u);
    if (rc) return rc;
    if (n_images == 0) return IFHIP_OK;
    if (!d_in || !d_canvas || (ycc && !d_cr)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null bitmap pointer");
    if ((reinterpret_cast<uintptr_t>(d_canvas) & 3u) || (canvas_image_bytes & 3u))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: canvas pixels must be 4-byte aligned");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != p->device) return fail(IFHIP_INVALID_STATE, "InvalidState: plan belongs to device %d, current device is %d", p->device, dev);
    DeviceTables tb;
    rc = device_tables(&tb);
    if (rc) return rc;

    LaunchInputs in = launch_inputs_now();
    in.alpha = alpha; in.ycc = ycc; in.n_images = n_images; in.in_image_bytes = in_image_bytes; in.in_stride = in_stride;
    in.src_low_bits = (reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_cb) | reinterpret_cast<uintptr_t>(d_cr)) & 15u;
    in.force_kernel = force_kernel; in.working_space = working_space; in.probe = probe;
    const LaunchChoice c = choose_launch(t, in);
    if (c.status) return c.status;
    if (trace_launch()) std::fprintf(stderr, "%s\n", format_launch(t, in, c).c_str());       // development aid: what this call launches
    if (probe) return IFHIP_OK;

    const ColorTables& host_tb = color_tables();
    ResampleArgs a;
    std::memset(&a, 0, sizeof a);
    a.in = d_in; a.in_image_bytes = in_image_bytes; a.in_stride = in_stride; a.in_w = t.in_w; a.in_h = t.in_h;
    a.in_cb = d_cb; a.in_cr = d_cr; a.ycc = ycc ? 1u : 0u;
    a.canvas = d_canvas; a.canvas_image_bytes = canvas_image_bytes; a.c_stride = c_stride; a.x = x; a.y = y;
    a.out_w = t.out_w; a.out_h = t.out_h; a.f32_dump = d_f32;
    a.h_meta = p->d_h_meta; a.h_wu = p->d_h_wu; a.h_wu_floats = static_cast<uint32_t>(t.wu.size());
    a.h_left = p->d_h_left; a.h_count = p->d_h_count;
    a.v_left = p->d_v_left; a.v_count = p->d_v_count; a.v_off = p->d_v_off; a.v_w = p->d_v_w;
    a.h_off = p->d_h_off; a.h_w = p->d_h_w;
    a.linear = working_space == IFHIP_SPACE_LINEAR;
    a.lut_in = a.linear ? tb.s2l : tb.s2f;
    a.l2s = tb.l2s;
    a.l2s_thr = tb.l2s_thr;
    a.mode = compositing;
    const float* s2 = a.linear ? host_tb.s2l : host_tb.s2f;       // matte colour in working space, scaling.rs:141-143
    a.m0 = s2[matte & 255u]; a.m1 = s2[(matte >> 8) & 255u]; a.m2 = s2[(matte >> 16) & 255u];
    a.matte_a = static_cast<float>(matte >> 24) * (1.0f / 255.0f);
    a.n_images = n_images;

    if (c.kernel == LaunchKernel::Banded) {
        HIP_TRY(launch_banded(a, alpha != 0, c.banded, c.grid, c.lds, st));
        return IFHIP_OK;
    }
    if (c.kernel == LaunchKernel::Fused) {
        if ((rc = schedule_on_device(t, c.schedule))) return rc;
        a.steps = c.schedule->d_steps; a.band_begin = c.schedule->d_band_begin; a.n_bands = c.n_bands;
        a.strips = p->d_strips[alpha ? 1 : 0]; a.n_strips = c.n_strips;
        a.h_groups = c.two_col ? 16u + c.fast_groups : c.fast_groups;                    // (16 + G2: the two-column form)
        if (c.two_col) { a.h_wu = p->d_h_wg2; a.h_wu_floats = static_cast<uint32_t>(t.wg2.size()); a.h_meta2 = p->d_h_meta3; }
        else if (c.fast_groups) { a.h_wu = p->d_h_wg; a.h_wu_floats = static_cast<uint32_t>(t.wg.size()); a.h_meta2 = p->d_h_meta2; }
        a.lut_copies_log2 = c.lut_copies_log2;
        a.h_w_in_lds = c.w_in_lds ? 1u : 0u;
        a.l2s_in_lds = c.l2s_in_lds ? 1u : 0u;
        a.frames_per_wg = c.frames_per_wg;
        a.lanes_per_frame = c.lanes_per_frame;
        HIP_TRY(launch_fused(a, t.slots, alpha != 0, c.per_pixel, c.grid, c.lanes_per_frame * c.frames_per_wg, c.lds, st));
        return IFHIP_OK;
    }
    // generic two-pass path through an HBM scratch of [chunk][out_h][in_w] float4: stream-ordered scratch from the block
    // cache -- nothing is shared between concurrent calls on the same plan, and the memory is reusable as soon as the last
    // kernel of this call has run (no host wait here)
    const size_t per_image = static_cast<size_t>(t.out_h) * t.in_w * sizeof(float4);
    float4* scratch = nullptr;
    HIP_TRY(static_cast<hipError_t>(cached_malloc_for_stream(reinterpret_cast<void**>(&scratch), per_image * c.chunk, st, true)));
    hipError_t le = hipSuccess;
    for (uint32_t i0 = 0; i0 < n_images && le == hipSuccess; i0 += c.chunk) {
        const uint32_t n = std::min(c.chunk, n_images - i0);
        le = launch_generic(a, alpha != 0, scratch, i0, n, st);
    }
    const hipError_t fe = static_cast<hipError_t>(cached_free_after(scratch, st));
    HIP_TRY(le);
    HIP_TRY(fe);
    return IFHIP_OK;
}
}  // namespace

namespace ifhip {
// The resampler fed by the JPEG stage's component planes (jpeg_kernels.hip).  IFHIP_OK, an error, or kNotFusable.
int resample_from_ycc_planes_v(const ifhip_resample_plan* plan, const uint8_t* d_y, const uint8_t* d_cb, const uint8_t* d_cr,
                             size_t plane_bytes, uint32_t pitch, uint32_t n_images, uint8_t* d_canvas, size_t canvas_image_bytes,
                             uint32_t cw, uint32_t ch, uint32_t c_stride, uint32_t x, uint32_t y, int working_space, int compositing,
                             uint32_t matte, void* hip_stream, bool probe) {
    return enqueue_batch(plan, d_y, plane_bytes, pitch, 0, n_images, d_canvas, canvas_image_bytes, cw, ch, c_stride, x, y,
                         working_space, compositing, matte, nullptr, -1, static_cast<hipStream_t>(hip_stream), d_cb, d_cr, probe);
}
void resample_plan_shape(const ifhip_resample_plan* plan, uint32_t* in_w, uint32_t* in_h, uint32_t* out_w, uint32_t* out_h) {
    *in_w = plan->t.in_w; *in_h = plan->t.in_h; *out_w = plan->t.out_w; *out_h = plan->t.out_h;
}
int device_color_tables(const float** s2l, const uint8_t** l2s) {
    DeviceTables tb;
    const int rc = device_tables(&tb);
    if (rc) return rc;
    *s2l = tb.s2l; *l2s = tb.l2s;
    return IFHIP_OK;
}

// Resample plans (contribution tables of one shape on the device, immutable, thread-safe) are shared by every caller of the
// process that does not bring its own: a service resizes to a handful of sizes, and a plan costs a dozen uploads.  Keyed by
// (device, shape, filter, sharpen); least recently used of 256 goes.
namespace {
struct PlanKey {
    int device; uint32_t in_w, in_h, w, h; int filter; uint32_t sharpen_bits;
    bool operator<(const PlanKey& o) const {
        return std::tie(device, in_w, in_h, w, h, filter, sharpen_bits) < std::tie(o.device, o.in_w, o.in_h, o.w, o.h, o.filter, o.sharpen_bits);
    }
};
std::mutex g_plan_mu;
typedef std::map<PlanKey, std::pair<std::shared_ptr<ifhip_resample_plan>, uint64_t>> PlanMap;
PlanMap& plan_map() { static PlanMap* m = new PlanMap; return *m; }        // never destroyed: no HIP calls from static destructors at exit
uint64_t g_plan_clock = 0;
constexpr size_t kPlanCacheMax = 256;
}  // namespace
int cached_plan(uint32_t in_w, uint32_t in_h, uint32_t w, uint32_t h, int filter, float sharpen, std::shared_ptr<ifhip_resample_plan>* out) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0)
        return fail(IFHIP_GPU_UNAVAILABLE, "GpuUnavailable: no HIP device (hipGetDevice failed); this library has no CPU path");
    uint32_t bits;
    std::memcpy(&bits, &sharpen, 4);
    const PlanKey key{dev, in_w, in_h, w, h, filter, bits};
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        auto it = plan_map().find(key);
        if (it != plan_map().end()) { it->second.second = ++g_plan_clock; *out = it->second.first; return IFHIP_OK; }
    }
    ifhip_resample_plan* raw = nullptr;
    const int rc = ifhip_resample_plan_create(&raw, in_w, in_h, w, h, filter, sharpen);
    if (rc) return rc;
    // A plan's tables are only ever READ by kernels, and every caller waits for its stream before it drops its reference, so
    // the last reference -- whoever holds it -- goes with nothing in flight on the plan; the deleter still waits for the
    // releasing thread's stream (a job's stream is its thread's stream) and, where the thread has none, the whole device
    // (cached_free).
    std::shared_ptr<ifhip_resample_plan> sp(raw, [](ifhip_resample_plan* q) {
        if (hipStream_t st = static_cast<hipStream_t>(thread_stream()); st && hipStreamQuery(st) != hipSuccess) (void)wait_stream(st);
        (void)hipGetLastError();
        ifhip_resample_plan_destroy(q);
    });
    std::shared_ptr<ifhip_resample_plan> evicted;                // released AFTER the lock: its deleter waits for a stream
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        PlanMap& plans = plan_map();
        if (plans.size() >= kPlanCacheMax) {                     // (callers still holding the victim keep it alive)
            auto victim = plans.begin();
            for (auto it = plans.begin(); it != plans.end(); ++it) if (it->second.second < victim->second.second) victim = it;
            evicted = std::move(victim->second.first);
            plans.erase(victim);
        }
        *out = plans.emplace(key, std::make_pair(sp, ++g_plan_clock)).first->second.first;
    }
    return IFHIP_OK;
}
}  // namespace ifhip

// ======================================================================================================
// extern "C"
// ======================================================================================================
extern "C" {

const char* ifhip_last_error_message(void) { return last_error(); }
const char* ifhip_version(void) { return "imageflow_hip 0.1 (gfx950)"; }

int ifhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int usable = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++usable;
    }
    return usable;
}

int ifhip_set_cu_budget(uint32_t compute_units) {
    if (compute_units > kComputeUnits) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: CU budget %u (the device has %u)", compute_units, kComputeUnits);
    set_cu_budget(compute_units);
    return IFHIP_OK;
}

int ifhip_set_device(int ordinal) {
    if (hipSetDevice(ordinal) != hipSuccess)
        return fail(IFHIP_GPU_UNAVAILABLE, "GpuUnavailable: hipSetDevice(%d) failed", ordinal);
    return IFHIP_OK;
}

uint32_t ifhip_stride_for_width(uint32_t w) {
    const uint64_t row = (static_cast<uint64_t>(w) * 4u + 63u) / 64u * 64u;
    return row > 0xFFFFFFC0ull ? 0u : static_cast<uint32_t>(row);          // 0 = the width has no 32-bit stride
}

int ifhip_populate_weights(int filter, int lobe_mode, float lobe_value, double kernel_width_scale,
                           uint32_t output_line_size, uint32_t input_line_size, uint32_t* left_pixel,
                           uint32_t* tap_count, float* weights, uint32_t weights_capacity, uint32_t* n_weights) {
    FilterSpec spec;
    if (!filter_spec_for(filter, &spec)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: unknown filter %d", filter);
    spec.blur *= kernel_width_scale;                 // set_kernel_width_scale, weights.rs:155-157
    spec.lobe_mode = lobe_mode; spec.lobe_value = lobe_value;
    AxisWeights w;
    int rc = build_axis_weights(spec, output_line_size, input_line_size, &w);
    if (rc) return rc;
    if (n_weights) *n_weights = static_cast<uint32_t>(w.w.size());
    if (weights_capacity == 0) return IFHIP_OK;
    if (w.w.size() > weights_capacity) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: weights_capacity too small");
    if (left_pixel) std::memcpy(left_pixel, w.left.data(), w.left.size() * sizeof(uint32_t));
    if (tap_count) std::memcpy(tap_count, w.count.data(), w.count.size() * sizeof(uint32_t));
    if (weights) std::memcpy(weights, w.w.data(), w.w.size() * sizeof(float));
    return IFHIP_OK;
}

int ifhip_table_srgb_to_floatspace(int working_space, float* out256) {
    if (!out256) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null table pointer");
    const ColorTables& t = color_tables();
    if (working_space == IFHIP_SPACE_LINEAR) std::memcpy(out256, t.s2l, sizeof t.s2l);
    else if (working_space == IFHIP_SPACE_SRGB) std::memcpy(out256, t.s2f, sizeof t.s2f);
    else return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: working floatspace %d", working_space);
    return IFHIP_OK;
}

int ifhip_table_linear_to_srgb(uint8_t* out16384) {
    if (!out16384) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null table pointer");
    std::memcpy(out16384, color_tables().l2s, 16384);
    return IFHIP_OK;
}

int ifhip_table_linear_to_srgb_thresholds(uint16_t* out256) {
    if (!out256) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null table pointer");
    std::memcpy(out256, color_tables().l2s_thr, 512);
    return IFHIP_OK;
}

int ifhip_resample_plan_create(ifhip_resample_plan** plan, uint32_t in_w, uint32_t in_h, uint32_t w, uint32_t h,
                               int filter, float sharpen_percent_goal) {
    if (!plan) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null plan out-pointer");
    *plan = nullptr;
    if (w == 0 || h == 0 || in_w == 0 || in_h == 0)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    FilterSpec spec;
    int rc = resample_filter_spec(filter, sharpen_percent_goal, &spec);
    if (rc) return rc;
    DeviceTables tb;
    if ((rc = device_tables(&tb))) return rc;                   // (no CPU path: no device, no tables)
    std::unique_ptr<ifhip_resample_plan> p(new ifhip_resample_plan);
    HIP_TRY(hipGetDevice(&p->device));
    PlanTables& t = p->t;
    if ((rc = build_plan_tables(in_w, in_h, w, h, spec, &t))) return rc;
    if ((rc = upload(t.wv.left, &p->d_v_left)) || (rc = upload(t.wv.count, &p->d_v_count)) ||
        (rc = upload(t.wv.offset, &p->d_v_off)) || (rc = upload(t.wv.w, &p->d_v_w)) ||
        (rc = upload(t.wh.left, &p->d_h_left)) || (rc = upload(t.wh.count, &p->d_h_count)) ||
        (rc = upload(t.wh.offset, &p->d_h_off)) || (rc = upload(t.wh.w, &p->d_h_w)) || (rc = upload(t.wu, &p->d_h_wu)) || (rc = upload(t.hmeta, &p->d_h_meta)))
        return rc;
    if (t.h_fast_groups && ((rc = upload(t.wg, &p->d_h_wg)) || (rc = upload(t.hmeta2, &p->d_h_meta2)))) return rc;
    if (t.h_two_groups && ((rc = upload(t.wg2, &p->d_h_wg2)) || (rc = upload(t.hmeta3, &p->d_h_meta3)))) return rc;
    for (int al = 0; al < 2; ++al)
        if (t.sets[al].ok && (rc = upload(t.sets[al].strips, &p->d_strips[al]))) return rc;
    *plan = p.release();
    return IFHIP_OK;
}

void ifhip_resample_plan_destroy(ifhip_resample_plan* plan) { delete plan; }

int ifhip_resample_plan_kernel_kind(const ifhip_resample_plan* plan, int in_alpha_meaningful) {
    return (plan && plan->t.fused_possible && plan->t.sets[in_alpha_meaningful ? 1 : 0].ok) ? 0 : 1;
}

// What the fast horizontal pass of the fused kernel would run for this plan: groups of four source columns per output
// (0: not available) and groups of two (0: not available or not fewer taps); see build_plan_tables.
int ifhip_resample_plan_horizontal_groups(const ifhip_resample_plan* plan, uint32_t* four_column_groups, uint32_t* two_column_groups) {
    if (!plan) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null plan");
    if (four_column_groups) *four_column_groups = plan->t.h_fast_groups;
    if (two_column_groups) *two_column_groups = plan->t.h_two_groups;
    return IFHIP_OK;
}


int ifhip_scale_and_render_batch_device(const ifhip_resample_plan* plan, const uint8_t* d_in, size_t in_image_bytes,
                                        uint32_t in_stride, int in_alpha_meaningful, uint32_t n_images,
                                        uint8_t* d_canvas, size_t canvas_image_bytes, uint32_t canvas_w,
                                        uint32_t canvas_h, uint32_t canvas_stride, uint32_t x, uint32_t y,
                                        int working_space, int compositing, uint32_t matte_bgra, float* d_f32_dump,
                                        int force_kernel, void* hip_stream) {
    return enqueue_batch(plan, d_in, in_image_bytes, in_stride, in_alpha_meaningful, n_images, d_canvas,
                         canvas_image_bytes, canvas_w, canvas_h, canvas_stride, x, y, working_space, compositing,
                         matte_bgra, d_f32_dump, force_kernel, static_cast<hipStream_t>(hip_stream));
}

// ---- host-buffer drop-ins ---------------------------------------------------------------------------------
}  // extern "C"

namespace {
// ---- staging of the host-buffer drop-ins -------------------------------------------------------------
// imageflow runs "one Context per thread" (imageflow_abi/src/lib.rs:20-27), so every calling thread gets its own
// HIP stream, pinned host staging and HBM staging, all grow-only and kept between calls: no hipMalloc / hipFree /
// hipMemset on the call path, no null-stream serialisation between threads.  A thread's staging returns to a pool
// when the thread ends (no HIP call at thread exit) and is adopted by the next new thread.
struct HostStage {
    int device = -1;
    hipStream_t stream = nullptr;
    uint8_t *pin_in = nullptr, *pin_c = nullptr, *d_in = nullptr, *d_c = nullptr;
    size_t pin_in_cap = 0, pin_c_cap = 0, d_in_cap = 0, d_c_cap = 0;
};
std::mutex g_stage_mu;
std::vector<HostStage*> g_stage_pool;
struct StageLease {
    HostStage* s = nullptr;
    ~StageLease() {
        if (!s) return;
        std::lock_guard<std::mutex> lk(g_stage_mu);
        g_stage_pool.push_back(s);
    }
};
thread_local StageLease t_stage;

int grow_pinned(uint8_t** p, size_t* cap, size_t want) {
    if (*cap >= want) return IFHIP_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const size_t sz = (want + (want >> 2) + 4095u) & ~static_cast<size_t>(4095);
    if (hipHostMalloc(reinterpret_cast<void**>(p), sz, hipHostMallocDefault) != hipSuccess)
        return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: %zu bytes of pinned host staging", sz);
    *cap = sz;
    return IFHIP_OK;
}
int grow_device(uint8_t** p, size_t* cap, size_t want) {
    if (*cap >= want) return IFHIP_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    const size_t sz = (want + (want >> 2) + 4095u) & ~static_cast<size_t>(4095);
    if (hipMalloc(reinterpret_cast<void**>(p), sz) != hipSuccess)
        return fail(IFHIP_ALLOCATION_FAILED, "AllocationFailed: %zu bytes of HBM staging", sz);
    *cap = sz;
    return IFHIP_OK;
}

int host_stage(HostStage** out) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0)
        return fail(IFHIP_GPU_UNAVAILABLE, "GpuUnavailable: no HIP device (hipGetDevice failed); this library has no CPU path");
    HostStage*& s = t_stage.s;
    if (s && s->device != dev) {                       // the thread switched devices: hand the old staging back
        std::lock_guard<std::mutex> lk(g_stage_mu);
        g_stage_pool.push_back(s);
        s = nullptr;
    }
    if (!s) {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        for (size_t i = 0; i < g_stage_pool.size(); ++i)
            if (g_stage_pool[i]->device == dev) { s = g_stage_pool[i]; g_stage_pool.erase(g_stage_pool.begin() + static_cast<long>(i)); break; }
    }
    if (!s) {
        std::unique_ptr<HostStage> n(new HostStage);
        n->device = dev;
        HIP_TRY(hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking));
        s = n.release();
    }
    *out = s;
    return IFHIP_OK;
}

// Host -> HBM through the pinned buffer in chunks: the DMA of chunk k runs while the CPU copies chunk k+1.
hipError_t upload_chunked(HostStage* s, uint8_t* d_dst, uint8_t* pinned, const uint8_t* src, size_t bytes) {
    constexpr size_t kChunk = 4u << 20;
    for (size_t off = 0; off < bytes; off += kChunk) {
        const size_t n = std::min(kChunk, bytes - off);
        std::memcpy(pinned + off, src + off, n);
        const hipError_t e = hipMemcpyAsync(d_dst + off, pinned + off, n, hipMemcpyHostToDevice, s->stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

extern "C" {
int ifhip_scale_and_render(const uint8_t* in, uint32_t in_w, uint32_t in_h, uint32_t in_stride, int in_alpha_meaningful,
                           uint8_t* canvas, uint32_t canvas_w, uint32_t canvas_h, uint32_t canvas_stride,
                           int /*canvas_alpha_meaningful*/, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int filter,
                           float sharpen_percent_goal, int working_space, int compositing, uint32_t matte_bgra) {
    int rc = validate_render(in_w, in_h, in_stride, canvas_w, canvas_h, canvas_stride, x, y, w, h, working_space, compositing);
    if (rc) return rc;
    if (!in || !canvas) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null bitmap pointer");
    // plans are cached per (device, shape, filter, sharpen): a server resizing many frames of the same size pays for the
    // weight tables and the vertical schedule once
    std::shared_ptr<ifhip_resample_plan> plan_ref;
    rc = cached_plan(in_w, in_h, w, h, filter, sharpen_percent_goal, &plan_ref);
    if (rc) return rc;
    ifhip_resample_plan* plan = plan_ref.get();
    HostStage* s = nullptr;
    if ((rc = host_stage(&s))) return rc;
    // stage: source rows as given; only the canvas rows the rect touches
    const size_t in_bytes = (static_cast<size_t>(in_h) * in_stride + 15u) & ~static_cast<size_t>(15);
    const size_t in_valid = static_cast<size_t>(in_h - 1) * in_stride + static_cast<size_t>(in_w) * 4u;
    const size_t c_rows_bytes = (static_cast<size_t>(h) * canvas_stride + 3u) & ~static_cast<size_t>(3);
    const size_t c_valid = static_cast<size_t>(h - 1) * canvas_stride + static_cast<size_t>(canvas_w) * 4u;
    if ((rc = grow_pinned(&s->pin_in, &s->pin_in_cap, in_valid)) || (rc = grow_pinned(&s->pin_c, &s->pin_c_cap, c_valid)) ||
        (rc = grow_device(&s->d_in, &s->d_in_cap, in_bytes + 64)) || (rc = grow_device(&s->d_c, &s->d_c_cap, c_rows_bytes + 64)))
        return rc;
    uint8_t* crow0 = canvas + static_cast<size_t>(y) * canvas_stride;
    hipError_t e = upload_chunked(s, s->d_in, s->pin_in, in, in_valid);
    // the kernels read whole 16-byte groups up to the row stride: the tail of the last row gets defined bytes
    if (e == hipSuccess) e = hipMemsetAsync(s->d_in + in_valid, 0, in_bytes + 64 - in_valid, s->stream);
    // the canvas rows travel to the device only when the call can leave some of their bytes untouched or reads them
    const bool canvas_needed = compositing == IFHIP_BLEND_WITH_SELF || x != 0 || w != canvas_w;
    if (e == hipSuccess && canvas_needed) e = upload_chunked(s, s->d_c, s->pin_c, crow0, c_valid);
    if (e == hipSuccess) {
        rc = enqueue_batch(plan, s->d_in, in_bytes, in_stride, in_alpha_meaningful, 1, s->d_c, c_rows_bytes,
                           canvas_w, h, canvas_stride, x, 0, working_space, compositing, matte_bgra, nullptr, -1, s->stream);
        if (rc == IFHIP_OK) {
            e = hipMemcpyAsync(s->pin_c, s->d_c, c_valid, hipMemcpyDeviceToHost, s->stream);
            if (e == hipSuccess) e = static_cast<hipError_t>(ifhip::wait_stream(s->stream));
            if (e == hipSuccess) {
                if (canvas_needed) std::memcpy(crow0, s->pin_c, c_valid);
                else                                      // whole rows were produced: leave the caller's row padding alone
                    for (uint32_t j = 0; j < h; ++j)
                        std::memcpy(crow0 + static_cast<size_t>(j) * canvas_stride, s->pin_c + static_cast<size_t>(j) * canvas_stride,
                                    static_cast<size_t>(canvas_w) * 4u);
            }
        } else (void)static_cast<hipError_t>(ifhip::wait_stream(s->stream));
    } else (void)static_cast<hipError_t>(ifhip::wait_stream(s->stream));
    if (rc) return rc;
    if (e != hipSuccess) return fail(IFHIP_GPU_ERROR, "GpuError: staging failed: %s", hipGetErrorString(e));
    return IFHIP_OK;
}

int ifhip_apply_matte_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w, uint32_t h,
                                   uint32_t stride, int alpha_meaningful, uint32_t matte_bgra, void* hip_stream) {
    if (!alpha_meaningful) return IFHIP_OK;                       // blend.rs:11-13
    if (w == 0 || h == 0 || n_images == 0) return IFHIP_OK;
    int rc = check_frames(d_bgra, image_bytes, w, h, stride, "bitmap");
    if (rc) return rc;
    DeviceTables tb;
    if ((rc = device_tables(&tb))) return rc;
    const ColorTables& t = color_tables();
    HIP_TRY(launch_apply_matte(d_bgra, image_bytes, n_images, w, h, stride, matte_bgra, t.s2l[matte_bgra & 255u],
                               t.s2l[(matte_bgra >> 8) & 255u], t.s2l[(matte_bgra >> 16) & 255u],
                               static_cast<float>(matte_bgra >> 24) * (1.0f / 255.0f), tb.s2l, tb.l2s,
                               static_cast<hipStream_t>(hip_stream)));
    return IFHIP_OK;
}

int ifhip_apply_matte(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int alpha_meaningful, uint32_t matte_bgra) {
    if (!alpha_meaningful) return IFHIP_OK;
    if (w == 0 || h == 0) return IFHIP_OK;
    if (!bgra) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null bitmap pointer");
    if (static_cast<uint64_t>(w) * 4u > stride || (stride & 3u))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: BGRA rows must be 4-byte aligned and stride >= 4*w");
    const size_t valid = static_cast<size_t>(h - 1) * stride + static_cast<size_t>(w) * 4u;
    const size_t bytes = (static_cast<size_t>(h) * stride + 15u) & ~static_cast<size_t>(15);
    HostStage* s = nullptr;
    int rc = host_stage(&s);
    if (rc) return rc;
    if ((rc = grow_pinned(&s->pin_c, &s->pin_c_cap, valid)) || (rc = grow_device(&s->d_c, &s->d_c_cap, bytes + 64))) return rc;
    hipError_t e = upload_chunked(s, s->d_c, s->pin_c, bgra, valid);
    if (e == hipSuccess) {
        rc = ifhip_apply_matte_batch_device(s->d_c, bytes, 1, w, h, stride, 1, matte_bgra, s->stream);
        if (rc == IFHIP_OK) {
            e = hipMemcpyAsync(s->pin_c, s->d_c, valid, hipMemcpyDeviceToHost, s->stream);
            if (e == hipSuccess) e = static_cast<hipError_t>(ifhip::wait_stream(s->stream));
            if (e == hipSuccess) std::memcpy(bgra, s->pin_c, valid);
        } else (void)static_cast<hipError_t>(ifhip::wait_stream(s->stream));
    } else (void)static_cast<hipError_t>(ifhip::wait_stream(s->stream));
    if (rc) return rc;
    if (e != hipSuccess) return fail(IFHIP_GPU_ERROR, "GpuError: staging failed: %s", hipGetErrorString(e));
    return IFHIP_OK;
}

}  // extern "C"
