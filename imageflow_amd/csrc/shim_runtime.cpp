// shim_runtime.cpp -- the device side of a job of the ABI shim (shim_runtime.hpp): the stream pool and the admission of jobs,
// contexts over devices, the job's device memory and the timing events.
#include "shim_runtime.hpp"

#include <condition_variable>
#include <cstring>
#include <string>

namespace ifshim {

// ---- the stream of a job ------------------------------------------------------------------------------------------------
// One Context per thread (imageflow_abi/src/lib.rs:20-27): every job runs on a stream of its own (non-blocking: nothing a
// job does waits for another thread's job), leased from a pool for the duration of one send_json; device memory comes from
// the library's size-class cache (devmem.cpp) and goes back without a driver call.  Whatever a job frees it frees behind
// quiesce() -- a look at the job's stream, a wait if it is still busy -- so the block is idle (ifhip::QuiescedScope around
// the whole job); nodes themselves do not wait for the device.
namespace {                                               // (of this file alone, as kJobSlots below)
std::mutex g_stream_mu;
struct DeviceQueues { std::vector<hipStream_t> pool; int slots_taken = 0; std::condition_variable slot_cv; };
std::map<int, DeviceQueues> g_queues;                     // per device ordinal: a stream belongs to the device it was created on
}  // namespace
__thread hipStream_t t_job_stream = nullptr;              // the stream of the job this thread is running (null outside a job)
// Admission: jobs beyond kJobSlots PER DEVICE wait for a slot on the host.  The rate grows with the jobs admitted -- batches
// of the coalesced decode fill up, the device always has somebody's pixel stage to run -- until the host's CPUs are the
// limit: 7 800 jobs/s at 20, 9 900 at 40, 11 100 at 48 for the thumbnail job on a 16-CPU container (round 5,
// profiles/r5_abi_jobs_slots_after_host_fixes.txt); 40 leaves a quarter of that container's CPUs to the caller.  (Rounds 4
// and 5 measured a FALL above 20 admitted jobs and blamed the runtime's hardware queues; it was the 17-32-file decode
// batches, see kMaxCoalesce.)
constexpr int kJobSlots = 40;
// Contexts and devices.  The reference's guidance is one Context per thread (imageflow_abi/src/lib.rs:20-27) and jobs are
// independent, so a node's GPUs are fed by giving every context a device: with ifhip_shim_spread_contexts(1) a new context
// takes the next usable device round-robin and all its jobs run there, whichever thread calls (no collective: a job's
// outputs are host buffers).  Without it (the default) a context follows the calling thread's current device, as before.
std::atomic<int> g_spread_contexts{0};
std::atomic<uint32_t> g_context_counter{0};
// HIP ordinals of the gfx950 devices, asked of the driver once (hipGetDeviceProperties fills a kilobyte struct per call, and
// a service creates thousands of contexts a second)
const std::vector<int>& usable_devices() {
    static const std::vector<int> list = [] {
        std::vector<int> v;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return v; }
        for (int i = 0; i < n; ++i) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, i) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) v.push_back(i);
            else (void)hipGetLastError();
        }
        return v;
    }();
    return list;
}
DeviceScope::DeviceScope(int dev) {
    if (dev < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
    if (prev != dev) {
        if (hipSetDevice(dev) == hipSuccess) switched = true;
        else (void)hipGetLastError();                 // (the first GPU call of the job reports)
    }
}
DeviceScope::~DeviceScope() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
StreamLease::StreamLease() {
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    {
        std::unique_lock<std::mutex> lk(g_stream_mu);
        constexpr int slots = kJobSlots;
        DeviceQueues& q = g_queues[dev];              // (map nodes do not move: the reference survives the wait)
        while (q.slots_taken >= slots) q.slot_cv.wait(lk);
        ++q.slots_taken;
        if (!q.pool.empty()) { st = q.pool.back(); q.pool.pop_back(); }
    }
    if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); st = nullptr; }   // (no device: the null stream, the first GPU call reports)
    t_job_stream = st;
    ifhip_set_thread_stream(st);
}
StreamLease::~StreamLease() {
    t_job_stream = nullptr;
    ifhip_set_thread_stream(nullptr);
    if (st) (void)static_cast<hipError_t>(ifhip::wait_stream(st));
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        DeviceQueues& q = g_queues[dev];
        if (st) q.pool.push_back(st);
        --q.slots_taken;
        q.slot_cv.notify_one();                       // (one waiter of THIS device; waking all of them cost a third of the job rate at 64 threads)
    }
}

hipEvent_t TimingEvents::take(int device) {
    {
        std::lock_guard<std::mutex> lk(mu);
        auto& v = spare[device];
        if (!v.empty()) { hipEvent_t e = v.back(); v.pop_back(); return e; }
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return e;
}
void TimingEvents::give(int device, hipEvent_t e) {
    if (!e) return;
    std::lock_guard<std::mutex> lk(mu);
    auto& v = spare[device];
    if (v.size() < 256) v.push_back(e); else (void)hipEventDestroy(e);
}
TimingEvents& timing_events() { static TimingEvents* t = new TimingEvents; return *t; }   // (never destroyed: jobs may outlive static teardown)

std::atomic<int> g_jobs_in_flight{0};

}  // namespace ifshim
