// shim_runtime.hpp -- what a job of the ABI shim runs on (shim_runtime.cpp): status words as errors, the device and the stream
// of a job, its device memory, and the hipEvents behind the nodes' device times.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/imageflow_hip.h"
#include "common.hpp"           // the library's per-job memory cache and thread stream (devmem.cpp)
#include "shim_errors.hpp"

namespace ifshim {

// (what every call of a job goes through is defined here, inline: check, hip_check, quiesce, job_malloc, job_free)
inline void check(int rc) {                                  // ifhip_status -> ErrorCategory
    if (rc == IFHIP_OK) return;
    const char* m = ifhip_last_error_message();
    const std::string msg = m ? m : "";
    int cat = kInternalError;
    if (rc == IFHIP_INVALID_ARGUMENT) cat = msg.rfind("ImageMalformed", 0) == 0 ? kImageMalformed : kArgumentInvalid;
    else if (rc == IFHIP_METHOD_NOT_IMPLEMENTED) cat = kActionNotSupported;
    else if (rc == IFHIP_ALLOCATION_FAILED) cat = kOutOfMemory;
    throw FlowErr{cat, msg};
}
inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) raise(e == hipErrorOutOfMemory ? kOutOfMemory : kInternalError, "GpuError: %s: %s", what, hipGetErrorString(e));
}

extern __thread hipStream_t t_job_stream;                 // the stream of the job this thread is running (null outside a job); __thread: read in place, no initialisation wrapper
extern std::atomic<int> g_spread_contexts;                // ifhip_shim_spread_contexts
extern std::atomic<uint32_t> g_context_counter;
extern std::atomic<int> g_jobs_in_flight;                 // send_json calls that hold a stream right now
const std::vector<int>& usable_devices();                 // HIP ordinals of the gfx950 devices
struct DeviceScope {                                      // the calling thread on the context's device for one call
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int dev);
    ~DeviceScope();
};
struct StreamLease {                                      // a job slot and a stream of the current device for one send_json
    hipStream_t st = nullptr;
    int dev = 0;
    StreamLease();
    ~StreamLease();
};
// Before anything of a job goes back to the cache: the job's stream -- the only one its blocks were ever used on -- is idle.
inline void quiesce() {
    if (t_job_stream && hipStreamQuery(t_job_stream) != hipSuccess) (void)static_cast<hipError_t>(ifhip::wait_stream(t_job_stream));
    (void)hipGetLastError();
}
inline hipError_t job_malloc(void** p, size_t bytes) { return static_cast<hipError_t>(ifhip::cached_malloc(p, bytes)); }
inline void job_free(void* p) { if (p) { quiesce(); (void)ifhip::cached_free(p); } }

// The hipEvents behind a node's `gpu_microseconds`, kept between jobs (two driver calls per node saved) and per device.
struct TimingEvents {
    std::mutex mu;
    std::map<int, std::vector<hipEvent_t>> spare;
    hipEvent_t take(int device);
    void give(int device, hipEvent_t e);
};
TimingEvents& timing_events();

}  // namespace ifshim
