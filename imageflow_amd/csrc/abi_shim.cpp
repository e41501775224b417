// abi_shim.cpp -- the OUTER drop-in boundary: a subset of libimageflow's C ABI v3.2 (imageflow_abi/src/lib.rs:389-1496,
// header bindings/headers/imageflow_default.h) over the gfx950 kernels, declared in include/imageflow_abi_subset.h.
//
// Deliberately thin: a context with an io table, a sticky error and a response list; a small
// JSON reader; and a straight-line interpreter for the `v1/build` / `v1/execute` job shapes that reach the pixel hot
// path -- decode(baseline JPEG) -> [orientation / crop / canvas primitives] -> resample_2d | constrain | command_string
// -> encode -- as `steps` or as a `graph` with `input` edges (one producer per node, any number of consumers).  It is
// NOT imageflow's router or graph engine: nodes outside that list answer ActionNotSupported, and everything a job
// computes is computed by the ifhip_* entry points of this library on frames that stay in HBM.
// A command_string's querystring is parsed and expanded into nodes by csrc/querystring.cpp (fit modes, crop, rotate, filters:
// imageflow_riapi's Instructions and Ir4Layout::add_steps); the interpreter runs that node list like any other.
//
// Two labelled EXTENSIONS, because the reference's JSON API has no raw-pixel I/O:
//   * decode accepts, besides JPEG and PNG (csrc/png_decode.hip), the container "IFBGRA1\0" + u32le w, h, stride, alpha_meaningful + rows;
//   * encode writes a real JPEG for the libjpeg_turbo preset -- baseline, optimised tables, progressive (device pixel stage + host Huffman coder, jpeg_write.cpp),
//     a progressive JPEG with optimised tables for the mozjpeg preset (raw forward stage + trellis quantisation + device coder, jpeg_trellis.hip),
//     a real PNG for the libpng preset (the device coder, png_encode.hip),
//     a palette PNG for the pngquant preset (the device quantiser, png_quantize.hip),
//     a lossless WebP for the webplossless preset (the device coder, webp_encode.hip),
//     and that container for every other preset (preferred_extension "ifbgra", mime "application/x-imageflow-bgra"):
//     the lodepng / lossy WebP coders are out of scope, the caller's encoder takes the frame;
//     "gif" is that container too unless ifhip_shim_context_set_gif_encoder switched the device GIF coder on (gif_encode.hip);
//   * with ifhip_shim_context_set_gif_animation on as well, an animated GIF source runs the job once per frame and the "gif"
//     encode nodes write one animated file (Job::run_job).
//
// Beside this file: shim_errors.hpp (the error categories and the exception a refusal travels in), shim_json.hpp / .cpp (the
// JSON reader and the parameter readers of the nodes: no GPU runtime, tests/shim_json_check.cpp runs them under the host
// sanitizers), shim_runtime.hpp / .cpp (a job's stream and device, its device memory, the timing events) and shim_job.hpp
// (frames, limits, the io table, the context, the records of a result), all in namespace ifshim.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/imageflow_abi_subset.h"
#include "../../include/imageflow_hip.h"
#include "../../include/imageflow_hip_webp_lossy_enc.h"   // the device lossy WebP coder (vp8_encode.hip), in a header of its own
#include "common.hpp"           // the library's per-job memory cache and thread stream (devmem.cpp)
#include "color_profile.hpp"   // a colour profile as a conversion plan (color_profile.cpp; the kernel: color_profile.hip)
#include "png_read.hpp"         // the PNG chunk walk and the device decode of a walked file (png_read.cpp, png_decode.hip)
#include "gif_read.hpp"         // the container walk and the device decode of a GIF (gif_read.cpp, gif_decode.hip)
#include "vp8_read.hpp"         // the host stage and the device decode of a lossy WebP (vp8_read.cpp, vp8_decode.hip)
#include "webp_read.hpp"        // the RIFF walk, the prepare and the device decode of a lossless WebP (webp_read.cpp, webp_decode.hip)
#include "layout.hpp"           // imageflow_riapi's constraint layout (constrain / watermark)
#include "querystring.hpp"      // imageflow_riapi's querystring: Instructions, their expansion into nodes (command_string)
#include "shim_job.hpp"          // frames, limits, Io, the context, the records; with it shim_json.hpp (JVal, parse_json, the parameter readers),
                                // shim_errors.hpp (Cat, FlowErr, raise) and shim_runtime.hpp (check, the job's stream, job_malloc / job_free, timing_events)

using namespace ifshim;

namespace {

const imageflow_json_response* respond(imageflow_context* c, int64_t status, const std::string& json) {
    c->responses.emplace_back(new imageflow_json_response{Response{status, json}});
    return c->responses.back().get();
}
const imageflow_json_response* respond_error(imageflow_context* c, int cat, const std::string& msg) {
    c->set_error(cat, msg);                                      // imageflow_abi/src/lib.rs:1001-1008
    const int code = http_code(cat);                             // JsonResponse::fail_with_message, json/mod.rs:170-181
    return respond(c, code, "{\n  \"code\": " + std::to_string(code) + ",\n  \"success\": false,\n  \"message\": \"" +
                                json_escape(msg) + "\",\n  \"data\": \"none\"\n}");      // ResponsePayload::None, a unit variant renamed "none" (imageflow_types/src/lib.rs:2061-2062)
}

// ---- decodes of different threads as ONE device call ---------------------------------------------------------------------
// A job decodes one file: 14 workgroups of the entropy kernels for a 4K JPEG, on a chip of 256 CUs, and the HIP runtime
// runs the streams of a process on a handful of hardware queues -- measured through this ABI (round 4): 5 300 jobs/s at 16
// threads and FEWER beyond, the GPU a fifth busy.  The entropy stage takes a batch of files of one geometry as cheaply as
// one (ifhip_jpeg_entropy_create / _decode_device), so concurrent decodes are coalesced: the first thread to arrive leads,
// gives the others a moment (only while other jobs are in flight at all), decodes everybody's file of its geometry in one
// call on its own stream and hands each job its image's planes; the rest wait on a condition variable.  A batch that fails
// (one damaged file) sends every member back to decode alone, so errors stay with the job that owns them.
// At most 16 files to a batch: the decode's cost per file is flat from 8 up (profiles/r5_abi_jobs_cliff_7_decode_batches.txt),
// and batches of 17-32 -- a sixth size class of 130 MB coefficient planes, everybody's pixel stages released at once --
// took 20-35 ms each where 16 take 3: the job rate fell from 6 500 to 800 whenever more than ~20 jobs were admitted
// (round 5, profiles/r5_abi_jobs_cliff_6_batch_cap.txt).
constexpr uint32_t kMaxCoalesce = 16;
struct DecodeRequest {
    ifhip_jpeg_prepared* prepared = nullptr;             // the job's file, prepared on the job's own thread
    uint32_t w = 0, h = 0;
    int ncomp = 0;
    uint8_t hs[3] = {0, 0, 0}, vs[3] = {0, 0, 0};
    // result
    std::shared_ptr<DecodedBatch> batch;
    uint32_t index = 0, batch_size = 0;
    bool done = false, retry_alone = false, taken = false;      // taken: a leader is decoding it
    std::condition_variable cv;                                 // this request's own wake-up (never a broadcast to every waiting job)
    bool same_geometry(const DecodeRequest& o) const {
        return w == o.w && h == o.h && ncomp == o.ncomp && std::memcmp(hs, o.hs, 3) == 0 && std::memcmp(vs, o.vs, 3) == 0;
    }
};
// one batch on the calling thread's job stream; throws FlowErr
std::shared_ptr<DecodedBatch> decode_files(const std::vector<DecodeRequest*>& reqs) {
    const uint32_t n = static_cast<uint32_t>(reqs.size());
    std::vector<ifhip_jpeg_prepared*> files(n);
    for (uint32_t i = 0; i < n; ++i) files[i] = reqs[i]->prepared;
    ifhip_jpeg_entropy* ent = nullptr;
    check(ifhip_jpeg_entropy_create_prepared(&ent, files.data(), n));
    struct EntGuard { ifhip_jpeg_entropy* e; ~EntGuard() { quiesce(); ifhip_jpeg_entropy_destroy(e); } } eg{ent};
    auto b = std::make_shared<DecodedBatch>();
    uint32_t nsub = 0, nseg = 0;
    check(ifhip_jpeg_entropy_info(ent, &b->w, &b->h, &b->ncomp, b->hs, b->vs, b->bw, b->bh, &nsub, &nseg));
    uint32_t n_cap = 1;                                          // (batch sizes as powers of two: six size classes in the cache, not thirty-two)
    while (n_cap < n) n_cap *= 2;
    for (int k = 0; k < 3; ++k) {
        b->per_image[k] = static_cast<size_t>(b->bw[k]) * b->bh[k] * 64u;
        hip_check(job_malloc(reinterpret_cast<void**>(&b->coef[k]), std::max<size_t>(1, b->per_image[k] * n_cap) * 2u), "hipMalloc(coefficients)");
    }
    // the quantisation tables ride along: queued before the decode, whose own wait for the stream covers them
    std::vector<uint16_t> qt(static_cast<size_t>(n) * 192u);
    check(ifhip_jpeg_entropy_quant_tables(ent, qt.data()));
    hip_check(job_malloc(reinterpret_cast<void**>(&b->d_qt), qt.size() * 2u), "hipMalloc(qt)");
    struct PinGuard { void* p = nullptr; ~PinGuard() { if (p) { quiesce(); (void)ifhip::cached_host_free(p); } } } qt_pin;
    hip_check(static_cast<hipError_t>(ifhip::stage_to_device(b->d_qt, qt.data(), qt.size() * 2u, &qt_pin.p)), "upload(qt)");
    uint32_t rounds = 0;
    check(ifhip_jpeg_entropy_decode_device(ent, b->coef[0], b->coef[1], b->coef[2], &rounds, t_job_stream));
    return b;
}
struct DecodeCoalescer {
    std::mutex mu;
    std::condition_variable leader_cv;                              // the gathering leader: "somebody arrived"
    std::vector<DecodeRequest*> queue;                              // requests nobody has taken yet, in arrival order
    bool leader_active = false;
    int decoding = 0;                                               // batches whose decode is on the device right now
    // Wake-ups are targeted: a request sleeps on its OWN condition variable and is woken when its batch is done or when it
    // is its turn to lead; arrivals wake only a leader that is counting them.  (One shared condition variable with
    // notify_all woke every waiting job on every arrival and every hand-over.  It was NOT what made the job rate fall above
    // 20 admitted jobs -- profiles/r5_abi_jobs_cliff_1_targeted_wakeups_no_effect.txt; that was the batch size, kMaxCoalesce --
    // but forty sleepers woken for one hand-over is work nobody needs.)
    void wake_next_leader() {                                       // (mu held) the oldest request nobody took: it may lead now
        if (!leader_active && !queue.empty()) queue.front()->cv.notify_one();
    }
    // -> r.batch / r.index set, or r.retry_alone
    void submit(DecodeRequest& r) {
        std::unique_lock<std::mutex> lk(mu);
        queue.push_back(&r);
        if (leader_active) leader_cv.notify_one();
        for (;;) {
            // At most `max_decoding` batches decode at a time; whoever arrives meanwhile waits here, and the next leader takes
            // ALL of them: the batch size follows the load by itself (group commit).  An entropy decode costs about the same
            // half millisecond for 1 file or 16 (three latency-bound launches), so a batch of 8 is an eighth of
            // the device time per job -- before, a new batch formed as soon as the last one had been gathered, 1.85 files per
            // batch at 2 300 jobs/s (round 5, profiles/r5_abi_trace_cfg4_8_threads.txt).
            constexpr int max_decoding = 2;
            while (!r.done && (r.taken || leader_active || decoding >= max_decoding || queue.front() != &r)) r.cv.wait(lk);
            if (r.done) return;
            leader_active = true;                                    // the oldest untaken request leads, for one batch
            // the moment given to the others: only while other jobs are in flight at all (a lone caller pays nothing) and no
            // decode is running (else the wait above was the moment)
            long window_us = (g_jobs_in_flight.load(std::memory_order_relaxed) > 1 && decoding == 0) ? 120 : 0;
            size_t wait_for = kMaxCoalesce;
            if (const char* e = ifhip::debug_switch("coalesce_window_us")) window_us = std::atol(e);
            if (const char* e = ifhip::debug_switch("coalesce_wait_for")) wait_for = static_cast<size_t>(std::max(1L, std::atol(e)));
            if (window_us > 0) {
                const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(window_us);
                while (queue.size() < wait_for && leader_cv.wait_until(lk, until) != std::cv_status::timeout) {}
            }
            // this thread's own request first, then whoever shares its geometry, in arrival order
            // Whatever leaves this block early (a bad_alloc while the lists are built) hands the leadership on and takes this
            // request out of the queue: a leader flag left set would park every later job of the device on its own condition
            // variable for good, and the request itself dies with its caller's frame.
            struct Leading {
                DecodeCoalescer& c; DecodeRequest* me; bool armed = true;
                ~Leading() {                                         // (mu held on every path that gets here armed)
                    if (!armed) return;
                    c.queue.erase(std::remove(c.queue.begin(), c.queue.end(), me), c.queue.end());
                    c.leader_active = false;
                    c.wake_next_leader();
                }
            } leading{*this, &r};
            std::vector<DecodeRequest*> mine{&r}, rest;
            for (DecodeRequest* q : queue)
                if (q != &r) (mine.size() < kMaxCoalesce && q->same_geometry(r) ? mine : rest).push_back(q);
            queue.swap(rest);
            for (DecodeRequest* q : mine) q->taken = true;
            leading.armed = false;
            leader_active = false;                                   // leading = gathering: the next batch forms while this one decodes
            ++decoding;
            if (decoding < max_decoding) wake_next_leader();
            lk.unlock();
            std::shared_ptr<DecodedBatch> b;
            bool failed = false;
            try { b = decode_files(mine); } catch (...) { failed = true; }      // (anything at all: the batch's members retry alone and report their own error)
            lk.lock();
            --decoding;
            for (size_t i = 0; i < mine.size(); ++i) {
                DecodeRequest* q = mine[i];
                if (failed) q->retry_alone = true;
                else { q->batch = b; q->index = static_cast<uint32_t>(i); q->batch_size = static_cast<uint32_t>(mine.size()); }
                q->done = true;
                if (q != &r) q->cv.notify_one();
            }
            wake_next_leader();
        }
    }
};
DecodeCoalescer& coalescer_for_device() {
    static std::mutex mu;
    static std::map<int, DecodeCoalescer*> per_device;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    DecodeCoalescer*& c = per_device[dev];
    if (!c) c = new DecodeCoalescer;
    return *c;
}

// Resample plans are shared by all jobs of the process (ifhip::cached_plan).  A plan dropped from the cache while a job still
// holds it is destroyed by that job's thread, behind the wait for the thread's stream -- which is the job's (StreamLease).
std::shared_ptr<ifhip_resample_plan> shared_plan(uint32_t in_w, uint32_t in_h, uint32_t w, uint32_t h, int filter, float sharpen) {
    std::shared_ptr<ifhip_resample_plan> plan;
    check(ifhip::cached_plan(in_w, in_h, w, h, filter, sharpen, &plan));
    return plan;
}

struct Job {
    imageflow_context* c;
    std::vector<EncodeRecord> encodes;
    std::vector<DecodeRecord> decodes;
    std::vector<NodePerf> perf;
    Security sec;
    std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();

    // return_if_cancelled! (imageflow_core/src/errors.rs:124-140; polled in Engine::graph_execute before every node,
    // execution_engine.rs:502, at every bitmap borrow, context.rs:389-401, and inside the codecs)
    void poll_cancel() {
        if (c->cancellation_requested()) raise(kOperationCancelled, "OperationCancelled: the job was cancelled");
    }

    // one executed primitive: wall clock as the reference's per-node cost (execution_engine.rs:506-538) plus the time
    // the device spent on it (hipEvents on the stream every node of this interpreter launches on)
    // A node's performance record: wall time on the host and, between two hipEvents on the job's stream, the device's time.
    // The node does NOT wait for the device when it ends -- its launches stay in flight while the host prepares the next
    // node's; the events are read once, at the job's end (settle_perf).  (Until round 5 every node ended in
    // hipEventSynchronize: 4 host/device round trips per job and, under the runtime's default spinning wait, one busy host
    // core per job in flight -- profiles/r5_abi_jobs_host_cpu.txt.)
    struct Timed {
        Job* j; const char* name; std::chrono::steady_clock::time_point t0; hipEvent_t e0 = nullptr, e1 = nullptr;
        Timed(Job* job, const char* n) : j(job), name(n), t0(std::chrono::steady_clock::now()) {
            const int dev = j->c->device.load(std::memory_order_relaxed);
            e0 = timing_events().take(dev); e1 = timing_events().take(dev);
            if (!e0 || !e1 || hipEventRecord(e0, t_job_stream) != hipSuccess) {
                (void)hipGetLastError();
                timing_events().give(dev, e0); timing_events().give(dev, e1);
                e0 = e1 = nullptr;
            }
        }
        ~Timed() {
            if (e0 && hipEventRecord(e1, t_job_stream) != hipSuccess) {
                (void)hipGetLastError();
                const int dev = j->c->device.load(std::memory_order_relaxed);
                timing_events().give(dev, e0); timing_events().give(dev, e1);
                e0 = e1 = nullptr;
            }
            const auto ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            try { j->perf.push_back({name, static_cast<uint64_t>(ns), 0.f, e0, e1}); }
            catch (...) { const int dev = j->c->device.load(std::memory_order_relaxed); timing_events().give(dev, e0); timing_events().give(dev, e1); }
        }
    };
    // the device times of the nodes, once the job's stream has drained; `read` false (a failed job): the events just go back
    void settle_perf(bool read) {
        bool any = false;
        for (const NodePerf& n : perf) any = any || n.e0;
        if (!any) return;
        const bool drained = read && ifhip::wait_stream(t_job_stream) == 0;
        const int dev = c->device.load(std::memory_order_relaxed);
        for (NodePerf& n : perf) {
            if (!n.e0) continue;
            if (drained && hipEventElapsedTime(&n.gpu_ms, n.e0, n.e1) != hipSuccess) { (void)hipGetLastError(); n.gpu_ms = 0.f; }
            timing_events().give(dev, n.e0); timing_events().give(dev, n.e1);
            n.e0 = n.e1 = nullptr;
        }
    }
    ~Job() { settle_perf(false); }

    // matte_canvas: the frame is CreateCanvas' result for a colour other than the enum value Transparent (-1: decide by the
    // colour's alpha, for callers that have no JSON colour)
    FramePtr new_frame(uint32_t w, uint32_t h, bool alpha, uint32_t fill_color32 = 0, bool zero = true, int matte_canvas = -1) {
        if (w == 0 || h == 0) raise(kArgumentInvalid, "InvalidArgument: Bitmap dimensions cannot be zero");
        check_size(sec.max_frame_size, "max_frame_size", w, h);
        poll_cancel();                                               // borrow_bitmaps_mut (context.rs:389)
        auto f = std::make_shared<Frame>();
        f->w = w; f->h = h; f->stride = ifhip_stride_for_width(w); f->alpha = alpha;
        if (f->stride == 0) raise(kArgumentInvalid, "InvalidArgument: Bitmap width %u has no 32-bit stride", w);
        hip_check(job_malloc(reinterpret_cast<void**>(&f->d), f->bytes() + 64), "hipMalloc(frame)");
        if (zero) hip_check(hipMemsetAsync(f->d, 0, f->bytes() + 64, t_job_stream), "hipMemset(frame)");
        if (matte_canvas < 0 ? (fill_color32 >> 24) != 0 : matte_canvas != 0) { f->compose = IFHIP_BLEND_WITH_MATTE; f->matte = fill_color32; }   // create_canvas.rs:77-103
        if (fill_color32 >> 24) {                    // bitmaps.rs:829-837: canvases start filled unless the colour is transparent
            check(ifhip_fill_rect_batch_device(f->d, f->bytes(), 1, w, h, f->stride, IFHIP_REPLACE_SELF, 0, 0, w, h, fill_color32, t_job_stream));
        }
        return f;
    }
    // the frame's pixels on the device; a pending JPEG gets its pixel stage now (IDCT + colour into a bitmap)
    uint8_t* dev(const FramePtr& f) {
        if (f->pending) {
            uint8_t* d = nullptr;                                    // the frame takes the bitmap only once it holds the pixels:
            hip_check(job_malloc(reinterpret_cast<void**>(&d), f->bytes() + 64), "hipMalloc(frame)");     // a failed stage leaves
            struct Guard { uint8_t* p; ~Guard() { job_free(p); } } g{d};                                  // `pending` and no buffer
            PendingJpeg& p = *f->pending;
            check(ifhip_jpeg_idct_color_batch_device(p.st, p.coef[0], p.coef[1], p.coef[2], p.d_qt, 1, d, f->bytes(), f->stride, t_job_stream));
            hip_check(static_cast<hipError_t>(ifhip::wait_stream(t_job_stream)), "decode");
            f->d = d; g.p = nullptr;
            f->pending.reset();
        }
        return f->d;
    }
    bool lazy_decode = false;                                        // the decode node being run has exactly one consumer
    // clone_node: the Clone node MutProtect puts before a mutating node whose parent has other children (definitions.rs:
    // 320-341) = CreateCanvas(Transparent, parent.fmt) + CopyRectToCanvas (clone_crop_fill_expand.rs:151-175), which leaves
    // the copy in BlendWithSelf (copy_rect.rs:37); otherwise a private copy of this interpreter's that keeps the frame's state
    FramePtr clone(const FramePtr& in, bool clone_node = false) {
        FramePtr c2 = new_frame(in->w, in->h, in->alpha, 0, false);
        hip_check(hipMemcpyAsync(c2->d, dev(in), in->bytes(), hipMemcpyDeviceToDevice, t_job_stream), "clone");
        if (clone_node) c2->compose = IFHIP_BLEND_WITH_SELF;
        else { c2->compose = in->compose; c2->matte = in->matte; }
        return c2;
    }

    Io& input(int32_t id) {
        auto it = c->io.find(id);
        if (it == c->io.end() || it->second.is_output) raise(kArgumentInvalid, "InvalidArgument: io_id %d is not a registered input", id);
        return it->second;
    }
    Io& output(int32_t id) {
        auto it = c->io.find(id);
        if (it == c->io.end() || !it->second.is_output) raise(kArgumentInvalid, "InvalidArgument: io_id %d is not a registered output", id);
        return it->second;
    }

    static bool is_png(const Io& in) {
        static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
        return in.in_len >= 8 && std::memcmp(in.in, sig, 8) == 0;
    }
    static bool is_webp(const Io& in) {                                  // codecs/mod.rs:130-131: RIFF....WEBP, 12 bytes
        return in.in_len >= 12 && std::memcmp(in.in, "RIFF", 4) == 0 && std::memcmp(in.in + 8, "WEBP", 4) == 0;
    }
    // "GIF87a" / "GIF89a" and a logical screen with pixels.  A GIF8?a buffer whose screen is 0 x 0 describes no canvas to
    // decode into and stays ImageTypeNotSupported (known difference: the reference reports a GIF decoding error)
    static bool is_gif(const Io& in) {
        return in.in_len >= 13 && (std::memcmp(in.in, "GIF87a", 6) == 0 || std::memcmp(in.in, "GIF89a", 6) == 0) && (in.in[6] | in.in[7]) && (in.in[8] | in.in[9]);
    }
    // the walk of a WebP input for a decode: a lossy file is ImageTypeNotSupported (known difference: the reference decodes it)
    // unless the context's lossy decoder is switched on (ifhip_shim_context_set_webp_lossy_decoder): then P->lossless tells the two apart
    static void walk_webp(const Io& in, ifhip::WebpParsed* P, bool lossy_decoder) {
        int rc = ifhip::parse_webp_for_decode(in.in, in.in_len, P);
        if (rc == IFHIP_METHOD_NOT_IMPLEMENTED && lossy_decoder) rc = ifhip::parse_webp_lossy_for_decode(in.in, in.in_len, P);
        if (rc == IFHIP_METHOD_NOT_IMPLEMENTED) raise(kImageTypeNotSupported, "%s", ifhip_last_error_message());
        check(rc);
    }
    // MzDec::get_exif_rotation_flag (mozjpeg_decoder.rs:290-292): the EXIF orientation tag of a JPEG input, -1 = none
    // (a PNG has none: LibPngDecoder::get_exif_rotation_flag is None, libpng_decoder.rs:54-56)
    static int exif_flag(const Io& in) {
        int flag = -1;
        if (in.in_len >= 4 && in.in[0] == 0xFF && in.in[1] == 0xD8) (void)ifhip_jpeg_exif_orientation(in.in, in.in_len, &flag);
        return flag;
    }
    // header facts of an input (get_scaled_rotated_image_info's part that watermark / command_string need); `rotated`:
    // Context::swap_dimensions_by_exif (context.rs:486-501) -- flags 5..8 swap width and height
    void image_size(int32_t io_id, uint32_t* w, uint32_t* h, bool rotated = false) {
        Io& in = input(io_id);
        if (rotated) {
            image_size(io_id, w, h, false);
            const int flag = exif_flag(in);
            if (flag >= 5 && flag <= 8) std::swap(*w, *h);
            return;
        }
        if (in.in_len >= kRawHeader && std::memcmp(in.in, kRawMagic, 8) == 0) {
            uint32_t hdr[4];
            std::memcpy(hdr, in.in + 8, 16);
            *w = hdr[0]; *h = hdr[1];
            return;
        }
        if (is_png(in)) {                                                // codecs/mod.rs:398-415 sniffing: the 8-byte signature
            ifhip_png_file_info pi;
            check(ifhip_png_info(in.in, in.in_len, &pi));
            *w = pi.width; *h = pi.height;
            return;
        }
        if (is_webp(in)) {                                               // WebPDecoder: no EXIF orientation (webp.rs:176-179)
            ifhip::WebpParsed P;
            walk_webp(in, &P, c->webp_lossy_decoder.load(std::memory_order_relaxed));
            *w = P.w; *h = P.h;
            return;
        }
        if (is_gif(in)) {                                                // GifDecoder: the logical screen, no EXIF orientation (gif/mod.rs:181-198)
            ifhip::GifParsed P;
            check(ifhip::parse_gif_header(in.in, in.in_len, &P));
            *w = P.w; *h = P.h;
            return;
        }
        int nc = 0;
        uint8_t hs[3], vs[3];
        uint32_t bw[3], bh[3], ri = 0;
        uint16_t qt[192];
        if (in.in_len < 3 || in.in[0] != 0xFF || in.in[1] != 0xD8)
            raise(kImageTypeNotSupported, "ImageTypeNotSupported: io_id %d is neither a JPEG nor the raw BGRA extension", io_id);
        int progressive = 0;
        (void)ri;
        const int rc = ifhip_jpeg_frame_info(in.in, in.in_len, w, h, &nc, hs, vs, bw, bh, qt, &progressive);
        if (rc == IFHIP_METHOD_NOT_IMPLEMENTED)
            raise(kImageTypeNotSupported, "ImageTypeNotSupported: %s (Huffman-coded 8-bit JPEG with 1 or 3 components only; keep other files on libjpeg)", ifhip_last_error_message());
        check(rc);
    }

    // Progressive / multi-scan files: entropy decoding on the host (csrc/jpeg_read.cpp), planes uploaded, everything else as usual
    std::shared_ptr<DecodedBatch> decode_on_host(const Io& in) {
        auto b = std::make_shared<DecodedBatch>();
        uint16_t qt[192];
        int progressive = 0;
        const int frc = ifhip_jpeg_frame_info(in.in, in.in_len, &b->w, &b->h, &b->ncomp, b->hs, b->vs, b->bw, b->bh, qt, &progressive);
        if (frc == IFHIP_METHOD_NOT_IMPLEMENTED)
            raise(kImageTypeNotSupported, "ImageTypeNotSupported: %s (Huffman-coded 8-bit JPEG with 1 or 3 components only; keep other files on libjpeg)", ifhip_last_error_message());
        check(frc);
        std::vector<int16_t> host[3];
        for (int k = 0; k < 3; ++k) {
            b->per_image[k] = static_cast<size_t>(b->bw[k]) * b->bh[k] * 64u;
            host[k].resize(std::max<size_t>(b->per_image[k], 64u));
        }
        poll_cancel();
        check(ifhip_jpeg_read_coefficients_host(in.in, in.in_len, host[0].data(), host[1].data(), host[2].data(), qt));
        for (int k = 0; k < 3; ++k) {
            hip_check(job_malloc(reinterpret_cast<void**>(&b->coef[k]), host[k].size() * 2u), "hipMalloc(coefficients)");
            hip_check(static_cast<hipError_t>(ifhip::copy_to_device(b->coef[k], host[k].data(), host[k].size() * 2u)), "upload(coefficients)");
        }
        hip_check(job_malloc(reinterpret_cast<void**>(&b->d_qt), sizeof qt), "hipMalloc(qt)");
        hip_check(static_cast<hipError_t>(ifhip::copy_to_device(b->d_qt, qt, sizeof qt)), "upload(qt)");
        return b;
    }

    // ---- colour management: codecs/cms.rs::transform_to_srgb, EXTENSION -- off unless the caller switches it on ------------
    // A source that is not sRGB (kind 2 of the three classifiers) and was not told discard_color_profile.  Off (the default):
    // the refusal, as ever.  On (ifhip_shim_context_set_color_management, or the decoder command "convert_color_profile"):
    // the plan of csrc/color_profile.cpp from the ICC bytes (`icc` non-null) or from gAMA + cHRM (`gama_chrm`: gAMA, then the
    // eight cHRM values, x 100000), true = apply it to the decoded frame.  A profile of a kind that is not converted here keeps
    // the refusal; a malformed one is ErrorKind::ColorProfileError (category ImageMalformed, errors.rs:241), which
    // ignore_color_profile_errors swallows as the reference does for every failure of its transform
    // (mozjpeg_decoder.rs:409-415, libpng_decoder.rs:376-382): the samples stay as they are.
    bool color_plan_for(int32_t io_id, const Io& in, const char* what, const char* reference_line, const uint8_t* icc, size_t icc_len,
                        const uint32_t* gama_chrm, ifhip_color_plan* plan) {
        if (!c->color_management.load(std::memory_order_relaxed) && !in.told_convert_profile)
            raise(kActionNotSupported, "ActionNotSupported: io_id %d %s; this build has no colour management%s%s%s.  Tell the decoder "
                  "\"discard_color_profile\" to decode the samples as they are, or keep the file on the reference.  (Conversion to sRGB on the device is an "
                  "extension that is off by default: ifhip_shim_context_set_color_management, or the decoder command \"convert_color_profile\", switches it on.)",
                  io_id, what, reference_line ? " (the reference converts such frames to sRGB, " : "", reference_line ? reference_line : "", reference_line ? ")" : "");
        ifhip::ColorPlanResult r;
        if (icc) r = ifhip::color_plan_from_icc(icc, icc_len, plan);
        else {
            double xy[8];
            for (int k = 0; k < 8; ++k) xy[k] = gama_chrm[1 + k] / 100000.0;
            r = ifhip::color_plan_from_gamma_primaries(gama_chrm[0] / 100000.0, xy, plan);
        }
        if (r.status == IFHIP_COLOR_PLANNED) return true;
        if (r.status == IFHIP_COLOR_NOT_CONVERTIBLE)
            raise(kActionNotSupported, "ActionNotSupported: io_id %d %s, and the profile is %s: %s (matrix/TRC RGB profiles and gAMA + cHRM are converted; GRAY, "
                  "CMYK, Lab and LUT-based profiles and curves that lift black are not).  Tell the decoder \"discard_color_profile\" to decode the samples as they are, or keep the file on "
                  "the reference.", io_id, what, ifhip::color_plan_status_text(r.status), r.reason);
        if (in.told_ignore_profile_errors) return false;
        raise(kImageMalformed, "ColorProfileError: the colour profile of io_id %d is %s: %s.  Tell the decoder \"ignore_color_profile_errors\" to decode the "
              "samples as they are.", io_id, ifhip::color_plan_status_text(r.status), r.reason);
    }
    // in place, on the job's stream, behind the decode that filled the frame; the plan is copied by the launch
    void convert_to_srgb(const FramePtr& f, const ifhip_color_plan& plan) {
        check(ifhip_color_transform_batch_device(dev(f), f->bytes(), 1, f->w, f->h, f->stride, &plan, t_job_stream));
    }
    // one file through a decoder's device part on the job's stream: queue(d_status) launches it; -> the file's status word, waited for
    template <typename Queue>
    uint32_t decoded_status(const char* label, Queue queue) {
        uint32_t* d_status = nullptr;
        hip_check(job_malloc(reinterpret_cast<void**>(&d_status), 16), "hipMalloc(status)");
        struct Guard { void* p; ~Guard() { job_free(p); } } guard{d_status};
        poll_cancel();
        check(queue(d_status));
        uint32_t status = 0;
        hip_check(hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, t_job_stream), "download(status)");
        hip_check(static_cast<hipError_t>(ifhip::wait_stream(t_job_stream)), label);
        return status;
    }

    // LibPngDecoder::read_frame (codecs/libpng_decoder.rs:82-104 -> c_components/lib/codec_png_wrapper.c:131-246) on the device:
    // the host walks the chunks, the IDAT stream is inflated, un-filtered and expanded to BGRA by csrc/png_decode.hip.  The
    // JPEG downscale hints do not apply (tell_decoder accepts and ignores them, libpng_decoder.rs:58-80).
    FramePtr decode_png(int32_t io_id, Io& in) {
        ifhip::PngParsed P;                                                           // ONE walk over the chunks: the facts and where the IDAT payloads lie
        check(ifhip::parse_png(in.in, in.in_len, &P, true));                          // a bad CRC, a malformed critical chunk: ImageMalformed
        check_size(sec.max_decode_size, "max_decode_size", P.w, P.h);                 // on the header, before anything is staged
        // The colour policy of the JPEG path below (DESIGN 8 "Colour management"): the reference transforms a frame whose iCCP,
        // or gAMA + cHRM, is not sRGB (libpng_decoder.rs:340-383); so does this build once switched on, else it refuses -- never
        // other colours.
        ifhip_color_plan color_plan;
        bool convert = false;
        if (!in.told_discard_profile && P.color_kind == 2) {
            static const uint8_t kNoProfile = 0;                                      // an iCCP that did not inflate: zero bytes of profile, malformed
            uint32_t gama_chrm[9] = {P.gama};
            std::memcpy(gama_chrm + 1, P.chrm, sizeof P.chrm);
            convert = color_plan_for(io_id, in, P.has_iccp ? "carries an embedded ICC profile that is not sRGB" : "carries gAMA and cHRM chunks that do not describe sRGB",
                                     "codecs/libpng_decoder.rs:376", P.has_iccp ? (P.icc.empty() ? &kNoProfile : P.icc.data()) : nullptr, P.icc.size(), gama_chrm, &color_plan);
        }
        if (P.inflated > 0x7FFF0000ull) raise(kImageMalformed, "ImageMalformed: LibPNG error: the image data of io_id %d would inflate beyond 2^31 bytes", io_id);
        FramePtr f = new_frame(P.w, P.h, P.alpha_used, 0, true);                      // (max_frame_size inside)
        const ifhip::PngParsed* parsed = &P;
        const size_t bytes = f->bytes();
        const uint32_t status = decoded_status("decode(png)", [&](uint32_t* d_status) { return ifhip::png_decode_parsed_device(&parsed, 1, &f->d, &bytes, &f->stride, d_status, t_job_stream); });
        if (status) raise(kImageMalformed, "ImageMalformed: LibPNG error: %s (io_id %d, status %u)", ifhip::png_status_text(status), io_id, status);
        if (convert) convert_to_srgb(f, color_plan);
        decodes.push_back({io_id, P.w, P.h, "image/png", "png"});
        return f;
    }

    // WebPDecoder::read_frame (codecs/webp.rs:162-248 -> WebPDecode, MODE_BGRA) on the device for a lossless file: the host walks
    // the container and prepares the stream, the token loop and the inverse transforms run in csrc/webp_decode.hip.  The JPEG
    // downscale hints are accepted and ignored; a told WebP hint that differs from the file's size would need libwebp's
    // decode-time rescaler (webp.rs:181-188), which is not built.
    FramePtr decode_webp(int32_t io_id, Io& in) {
        ifhip::WebpParsed P;
        walk_webp(in, &P, c->webp_lossy_decoder.load(std::memory_order_relaxed));
        check_size(sec.max_decode_size, "max_decode_size", P.w, P.h);                 // on the header, before anything is staged
        ifhip_color_plan color_plan;
        const bool convert = !in.told_discard_profile && P.color_kind == 2 &&
                             color_plan_for(io_id, in, "carries an embedded ICC profile that is not sRGB", nullptr, P.icc, P.icc_len, nullptr, &color_plan);
        if (in.told_webp && (in.told_webp_w != P.w || in.told_webp_h != P.h))
            raise(kActionNotSupported, "ActionNotSupported: webp_decoder_hints %ux%u for io_id %d (%ux%u): libwebp's decode-time rescaler is not built "
                  "(the reference shrinks during the decode, codecs/webp.rs:181-188); decode at full size and resample", in.told_webp_w, in.told_webp_h, io_id, P.w, P.h);
        FramePtr f = new_frame(P.w, P.h, P.has_alpha, 0, true);                       // (max_frame_size inside)
        const size_t bytes = f->bytes();
        uint32_t status = 0;
        const char* status_text = nullptr;                                            // (each decoder words its own status)
        if (!P.lossless) {
            // EXTENSION (ifhip_shim_context_set_webp_lossy_decoder): a still `VP8 ` (+ `ALPH`) file.  The host reads the key frame's header
            // and bool-decodes its partitions (csrc/vp8_read.cpp), the pixels are made in csrc/vp8_decode.hip; libwebp's default options.
            ifhip::Vp8Job J;
            ifhip::vp8_prepare_job(P, &J);                                            // on this job's thread, like webp_prepare_job
            status = J.frame.status;
            const ifhip::Vp8Job* job = &J;
            if (!status) status = decoded_status("decode(webp lossy)", [&](uint32_t* d_status) { return ifhip::vp8_decode_prepared_device(&job, 1, &f->d, &bytes, &f->stride, d_status, t_job_stream); });
            if (status) status_text = ifhip::vp8_status_text(status);
        } else {
            ifhip::WebpJob J;
            ifhip::webp_prepare_job(P, &J);                                           // on this job's thread, like ifhip_jpeg_entropy_prepare
            if (J.status) raise(kImageMalformed, "ImageMalformed: libwebp decoding error %s (io_id %d, status %u)", ifhip::webp_status_text(J.status), io_id, J.status);
            const ifhip::WebpJob* job = &J;
            status = decoded_status("decode(webp)", [&](uint32_t* d_status) { return ifhip::webp_decode_prepared_device(&job, 1, &f->d, &bytes, &f->stride, d_status, t_job_stream); });
            if (status) status_text = ifhip::webp_status_text(status);
        }
        if (status) raise(kImageMalformed, "ImageMalformed: libwebp decoding error %s (io_id %d, status %u)", status_text, io_id, status);
        if (convert) convert_to_srgb(f, color_plan);
        decodes.push_back({io_id, P.w, P.h, "image/webp", "webp"});
        return f;
    }

    // GifDecoder::read_frame (codecs/gif/mod.rs:207-298) on the device: the host walks the container up to the selected frame
    // (csrc/gif_read.cpp), the LZW streams of frames 0..N are decoded and the frames composed with their disposal by
    // csrc/gif_decode.hip; frame N's screen enters the graph as bgra_32 with meaningful alpha.  The limits come first, on the
    // header (mod.rs:55-85: max_decode_size, else max_frame_size, on the logical screen).  GIF carries neither EXIF nor a
    // colour profile; the JPEG and WebP hints are accepted and ignored.
    struct GifSource { bool seen; int repeat; uint32_t delay; bool user_input; } gif_source{false, -1, 0u, false};   // of the first GIF the job decoded
    FramePtr decode_gif(int32_t io_id, Io& in) {
        if (anim.active && anim.in_decode_node && anim.sources.count(io_id)) return animated_screen(io_id);
        ifhip::GifParsed P;
        check(ifhip::parse_gif_header(in.in, in.in_len, &P));
        check_size(sec.max_decode_size, "max_decode_size", P.w, P.h);
        check_size(sec.max_frame_size, "max_frame_size", P.w, P.h);
        const int32_t target = in.told_frame ? in.told_frame_n : 0;
        check(ifhip::parse_gif(in.in, in.in_len, static_cast<uint32_t>(std::max<int32_t>(target, 0)), &P));
        auto refuse = [&](uint32_t status) {
            if (status == IFHIP_GIF_DEC_NO_SUCH_FRAME)                                // mod.rs:217-224
                raise(kArgumentInvalid, "InvalidArgument: frame=%d requested but GIF only has %zu frames", target, P.frames.size());
            if (status == IFHIP_GIF_DEC_FRAME_TOO_LARGE) raise(kArgumentInvalid, "SizeLimitExceeded: %s (io_id %d)", ifhip::gif_status_text(status), io_id);
            raise(kImageMalformed, "ImageMalformed: GIF decoding error: %s (io_id %d, status %u)", ifhip::gif_status_text(status), io_id, status);
        };
        if (P.status) refuse(P.status);
        FramePtr f = new_frame(P.w, P.h, true, 0, true);
        const ifhip::GifParsed* parsed = &P;
        const size_t bytes = f->bytes();
        const uint32_t status = decoded_status("decode(gif)", [&](uint32_t* d_status) { return ifhip::gif_decode_parsed_device(&parsed, 1, &f->d, &bytes, &f->stride, d_status, t_job_stream); });
        if (status) refuse(status);
        if (!gif_source.seen) {                                                  // what GifEncoder::write_frame asks the job's GIF decoder for (mod.rs:436-483)
            const ifhip::GifFrameInfo& last = P.frames.back();
            gif_source = {true, P.repeat < 0 ? 0 : P.repeat, last.delay, last.user_input != 0u};   // (no NETSCAPE2.0 block: get_repeat's Infinite, mod.rs:167-170)
        }
        decodes.push_back({io_id, P.w, P.h, "image/gif", "gif"});
        return f;
    }

    // decode: MozJpegDecoder::read_frame (codecs/mozjpeg_decoder.rs:295-420) on the device, or the raw extension
    FramePtr decode(int32_t io_id, uint32_t hint_w, uint32_t hint_h, bool luma_spatial, bool luma_srgb) {
        Timed t(this, "primitive_decoder");
        Io& in = input(io_id);
        if (in.in_len >= kRawHeader && std::memcmp(in.in, kRawMagic, 8) == 0) {
            uint32_t hdr[4];
            std::memcpy(hdr, in.in + 8, 16);
            const uint32_t w = hdr[0], h = hdr[1], stride = hdr[2];
            if (w == 0 || h == 0 || stride < w * 4ull || (stride & 3u) || in.in_len < kRawHeader + static_cast<size_t>(h - 1) * stride + w * 4ull)
                raise(kImageMalformed, "ImageMalformed: raw BGRA container header does not match its length");
            check_size(sec.max_decode_size, "max_decode_size", w, h);
            FramePtr f = new_frame(w, h, hdr[3] != 0, 0, true);
            hip_check(hipMemcpy2DAsync(f->d, f->stride, in.in + kRawHeader, stride, w * 4ull, h, hipMemcpyHostToDevice, t_job_stream), "upload(raw frame)");
            hip_check(static_cast<hipError_t>(ifhip::wait_stream(t_job_stream)), "upload(raw frame)");
            decodes.push_back({io_id, w, h, "application/x-imageflow-bgra", "ifbgra"});
            return f;
        }
        if (is_png(in)) return decode_png(io_id, in);
        if (is_webp(in)) return decode_webp(io_id, in);
        if (is_gif(in)) return decode_gif(io_id, in);
        if (in.in_len < 3 || in.in[0] != 0xFF || in.in[1] != 0xD8)                        // codecs/mod.rs:398-415 sniffing
            raise(kImageTypeNotSupported, "ImageTypeNotSupported: io_id %d is neither a JPEG nor the raw BGRA extension", io_id);
        {   // limits before anything is staged (mozjpeg_decoder.rs:196-214 checks max_decode_size on the header)
            uint32_t hw = 0, hh = 0;
            image_size(io_id, &hw, &hh);
            check_size(sec.max_decode_size, "max_decode_size", hw, hh);
        }
        ifhip_color_plan color_plan;
        bool convert = false;
        {   // MzDec::read_frame transforms the frame to sRGB whenever the file carries an ICC profile (mozjpeg_decoder.rs:370-420)
            // unless the decoder was told discard_color_profile (:88-91).  A profile that is not sRGB itself would come out with
            // other colours than the reference's: the job is refused -- loudly -- unless colour management is switched on, and
            // then the frame is converted behind its decode (a profile that IS sRGB: the reference's transform is the identity up
            // to its rounding).
            int kind = 0;
            std::vector<uint8_t> icc;
            if (!in.told_discard_profile && ifhip::jpeg_icc_profile(in.in, in.in_len, &kind, &icc) == IFHIP_OK && kind == 2)
                convert = color_plan_for(io_id, in, "carries an embedded ICC profile that is not sRGB", "codecs/mozjpeg_decoder.rs:409", icc.data(), icc.size(), nullptr, &color_plan);
        }
        // the entropy stage: this file, together with whatever other threads' jobs want decoded right now (DecodeCoalescer)
        DecodeRequest rq;
        const int prc = ifhip_jpeg_entropy_prepare(&rq.prepared, in.in, in.in_len);          // parse, un-stuff, pack, tables: on this job's thread
        struct PreparedGuard { ifhip_jpeg_prepared* p; ~PreparedGuard() { ifhip_jpeg_prepared_destroy(p); } } prepared_guard{rq.prepared};
        if (prc == IFHIP_METHOD_NOT_IMPLEMENTED) {
            // not a single-scan baseline file: progressive (what the reference's mozjpeg preset writes) or multi-scan -- the scans
            // are decoded on the host as MzDec does (libjpeg's jdphuff.c), the pixel stage behind them stays on the GPU
            rq.batch = decode_on_host(in);
            rq.index = 0; rq.batch_size = 1;
        } else {
            check(prc);
            check(ifhip_jpeg_prepared_info(rq.prepared, &rq.w, &rq.h, &rq.ncomp, rq.hs, rq.vs));
            check(ifhip_jpeg_prepared_upload(rq.prepared, t_job_stream));      // the file's PCIe transfer starts now, not when a batch leader gets to it
            poll_cancel();                                           // the decoder's cancellation point (mozjpeg_decoder.rs:346-362 loop)
            coalescer_for_device().submit(rq);
            if (rq.retry_alone) {                                    // the shared call failed (somebody's file, maybe this one): alone, errors are this job's
                std::vector<DecodeRequest*> one{&rq};
                rq.batch = decode_files(one);
                rq.index = 0; rq.batch_size = 1;
            }
        }
        if (rq.batch_size > 1) c->coalesced_decodes.fetch_add(1, std::memory_order_relaxed);
        const std::shared_ptr<DecodedBatch> batch = rq.batch;
        const uint32_t w = batch->w, h = batch->h;
        const int ncomp = batch->ncomp;
        const uint8_t* hs = batch->hs;
        const uint8_t* vs = batch->vs;
        // MzDec::apply_downscaling (mozjpeg_decoder.rs:588-618): smallest i/8 (7 skipped) that still covers the hint
        int scale = 8;
        if (hint_w > 0 && hint_h > 0 && (w > hint_w || h > hint_h))                   // downscale_if_wider_than = width, or_if_taller_than = height (:72-77)
            for (int i = 1; i < 8; ++i) {
                if (i == 7) continue;
                if ((static_cast<uint64_t>(w) * i + 7) / 8 >= hint_w && (static_cast<uint64_t>(h) * i + 7) / 8 >= hint_h) { scale = i; break; }
            }
        ifhip_jpeg_stage* st = nullptr;
        const bool spatial = scale < 8 && luma_spatial;
        check(ifhip_jpeg_stage_create(&st, w, h, ncomp, hs, vs, scale, spatial ? 1 : 0, spatial && luma_srgb ? 1 : 0, 1));
        auto pend = std::make_unique<PendingJpeg>();                                  // owns the stage and a share of the decoded batch
        pend->st = st;
        pend->batch = batch;
        for (int k = 0; k < 3; ++k) pend->coef[k] = batch->coef[k] + static_cast<size_t>(rq.index) * batch->per_image[k];
        pend->d_qt = batch->d_qt + static_cast<size_t>(rq.index) * 192u;
        uint32_t ow = 0, oh = 0;
        check(ifhip_jpeg_stage_output_size(st, &ow, &oh));
        if (ow == 0 || oh == 0) raise(kArgumentInvalid, "InvalidArgument: Bitmap dimensions cannot be zero");
        check_size(sec.max_frame_size, "max_frame_size", ow, oh);
        poll_cancel();                                                                // borrow_bitmaps_mut (context.rs:389), as new_frame
        auto f = std::make_shared<Frame>();                                           // alpha not meaningful (:101-123)
        f->w = ow; f->h = oh; f->stride = ifhip_stride_for_width(ow); f->alpha = false;
        f->pending = std::move(pend);
        if (!lazy_decode) (void)dev(f);                                               // several consumers: one bitmap for all of them
        // a frame to convert never takes the fused decode + resample call, which forms no BGRA frame: its pixel stage runs now
        // (dev), then the conversion; whoever resamples it -- a node, a command_string, a watermark -- finds an ordinary frame
        if (convert) convert_to_srgb(f, color_plan);
        {   // Context::get_image_decodes reports get_unscaled_rotated_image_info (context.rs:519-538)
            const int flag = exif_flag(in);
            const bool swap = flag >= 5 && flag <= 8;
            decodes.push_back({io_id, swap ? h : w, swap ? w : h, "image/jpeg", "jpg"});
        }
        return f;
    }

    static ResampleHints parse_hints(const JVal* hints, const char* node) {
        ResampleHints r;
        if (!hints || hints->is_null()) return r;
        if (hints->t != JVal::Obj) raise(kInvalidJson, "InvalidJson: %s.hints must be an object", node);
        if (const JVal* s = hints->get("sharpen_percent")) if (s->t == JVal::Num) { r.has_sharpen = true; r.sharpen = static_cast<float>(s->n); }
        r.down = parse_filter(hints->get("down_filter"), r.down);
        r.up = parse_filter(hints->get("up_filter"), r.up);
        if (const JVal* cs = hints->get("scaling_colorspace"))
            if (cs->t == JVal::Str) {
                if (cs->s == "srgb") r.space = IFHIP_SPACE_SRGB;
                else if (cs->s != "linear") raise(kInvalidJson, "InvalidJson: scaling_colorspace must be srgb or linear");
            }
        if (const JVal* b = hints->get("background_color"))
            if (!b->is_null()) {
                r.has_bg = true;
                r.bg_keyword_transparent = b->t == JVal::Str && b->s == "transparent";
                r.bg = parse_color(b, "hints.background_color");
            }
        if (const JVal* rw = hints->get("resample_when"))
            if (rw->t == JVal::Str) {                                                // s::ResampleWhen (lib.rs:899-907)
                if (rw->s == "always") r.resample_when = ResampleHints::kAlways;
                else if (rw->s == "size_differs") r.resample_when = ResampleHints::kSizeDiffers;
                else if (rw->s == "size_differs_or_sharpening_requested") r.resample_when = ResampleHints::kSizeDiffersOrSharpen;
                else raise(kInvalidJson, "InvalidJson: unknown resample_when '%s'", rw->s.c_str());
            }
        if (const JVal* sw = hints->get("sharpen_when"))
            if (sw->t == JVal::Str) {                                                // s::SharpenWhen
                if (sw->s == "always") r.sharpen_when = ResampleHints::kSAlways;
                else if (sw->s == "downscaling") r.sharpen_when = ResampleHints::kSDown;
                else if (sw->s == "upscaling") r.sharpen_when = ResampleHints::kSUp;
                else if (sw->s == "size_differs") r.sharpen_when = ResampleHints::kSSizeDiffers;
                else raise(kInvalidJson, "InvalidJson: unknown sharpen_when '%s'", sw->s.c_str());
            }
        return r;
    }
    static float gated_sharpen(const ResampleHints& hi, uint32_t w, uint32_t h, uint32_t in_w, uint32_t in_h) {   // scale_render.rs:55-65, 263-274
        const bool size_differs = w != in_w || h != in_h, downscaling = w < in_w || h < in_h, upscaling = w > in_w || h > in_h;
        const float raw = hi.has_sharpen ? hi.sharpen : 0.f;
        switch (hi.sharpen_when) {
        case ResampleHints::kSAlways: return raw;
        case ResampleHints::kSDown: return downscaling ? raw : 0.f;
        case ResampleHints::kSUp: return upscaling ? raw : 0.f;
        case ResampleHints::kSSizeDiffers: return size_differs ? raw : 0.f;
        }
        return raw;
    }

    // DrawImageDef::render (flow/nodes/scale_render.rs:221-320): the one caller of the hot path.  compose = the
    // node's `blend` (None = Compose).
    void draw_image_exact(const FramePtr& canvas, const FramePtr& in, uint32_t x, uint32_t y, uint32_t w, uint32_t h, bool compose, const ResampleHints& hi) {
        Timed t(this, "draw_image_to_canvas");
        if (canvas == in) raise(kGraphInvalid, "InvalidNodeConnections: Canvas and Input are the same bitmap!");
        if (static_cast<uint64_t>(x) + w > canvas->w || static_cast<uint64_t>(y) + h > canvas->h)                       // :237-240
            raise(kArgumentInvalid, "InvalidNodeParams: DrawImageExact target rect x1=%u,y1=%u,w=%u,h=%u does not fit canvas size %ux%u.", x, y, w, h, canvas->w, canvas->h);
        if (w == 0 || h == 0) raise(kArgumentInvalid, "InvalidNodeParams: DrawImageExact target size must be non-zero");
        if (hi.resample_when != ResampleHints::kDefault && hi.resample_when != ResampleHints::kAlways)                 // :246-251
            raise(kArgumentInvalid, "InvalidNodeParams: DrawImageExact already has a canvas and cannot honor ResampleWhen");
        const bool upscaling = w > in->w || h > in->h;                                                                 // :253
        const int filter = upscaling ? hi.up : hi.down;                                                                // :257-261
        const float sharpen = gated_sharpen(hi, w, h, in->w, in->h);
        if (canvas->compose == IFHIP_REPLACE_SELF && compose) canvas->compose = IFHIP_BLEND_WITH_SELF;                 // :284-286
        if (canvas->compose == IFHIP_BLEND_WITH_MATTE && !compose && canvas->alpha) canvas->compose = IFHIP_REPLACE_SELF;   // :287-292
        poll_cancel();
        const std::shared_ptr<ifhip_resample_plan> plan_ref = shared_plan(in->w, in->h, w, h, filter, sharpen);
        ifhip_resample_plan* plan = plan_ref.get();
        if (in->pending) {                            // MzDec::read_frame + scale_and_render as one device call (mozjpeg_decoder.rs:346-362 -> :304-313)
            PendingJpeg& pj = *in->pending;
            int fused_call = 0;
            check(ifhip_jpeg_decode_resample_batch_device(pj.st, pj.coef[0], pj.coef[1], pj.coef[2], pj.d_qt, 1, plan, dev(canvas), canvas->bytes(), canvas->w,
                                                          canvas->h, canvas->stride, x, y, hi.space, canvas->compose, canvas->matte, &fused_call, t_job_stream));
            if (fused_call) c->fused_decode_resamples.fetch_add(1, std::memory_order_relaxed);
        } else
        check(ifhip_scale_and_render_batch_device(plan, in->d, in->bytes(), in->stride, in->alpha ? 1 : 0, 1, dev(canvas), canvas->bytes(),
                                                  canvas->w, canvas->h, canvas->stride, x, y, hi.space, canvas->compose, canvas->matte, nullptr, -1, t_job_stream));
        hip_check(static_cast<hipError_t>(ifhip::wait_stream(t_job_stream)), "draw_image_exact");
        canvas->compose = IFHIP_BLEND_WITH_SELF;                                                                       // :314
    }

    // Resample2D (scale_render.rs:30-120): removed from the graph unless it resamples or has a matte to apply to a
    // Bgra32 parent; otherwise CreateCanvas{parent.fmt, background_color} + Scale2d, which becomes DrawImageExact with
    // blend = Overwrite when the background is transparent (:139-201)
    FramePtr resample(const FramePtr& in, uint32_t w, uint32_t h, const JVal* hints_json) {
        if (w == 0 || h == 0) raise(kArgumentInvalid, "InvalidNodeParams: resample_2d target size must be non-zero");
        ResampleHints hi = parse_hints(hints_json, "resample_2d");
        const bool size_differs = w != in->w || h != in->h;
        const bool apply_matte = in->alpha && hi.has_bg && !hi.bg_keyword_transparent;                                 // :44-47
        const float sharpen = gated_sharpen(hi, w, h, in->w, in->h);
        const bool sharpen_requested = sharpen != 0.f;                                                                 // :67
        bool do_resample = false;
        switch (hi.resample_when) {                                                                                    // :69-78
        case ResampleHints::kAlways: do_resample = true; break;
        case ResampleHints::kSizeDiffers: do_resample = size_differs; break;
        default: do_resample = size_differs || sharpen_requested; break;
        }
        if (!do_resample && !apply_matte) return in;                                                                   // delete_node_and_snap_together (:115)
        hi.has_sharpen = true; hi.sharpen = sharpen;                                                                   // Some(sharpen_percent), sharpen_when passed on (:84-94)
        hi.resample_when = ResampleHints::kAlways;
        const uint32_t bg = hi.has_bg ? hi.bg : 0u;
        FramePtr canvas;
        {
            Timed t(this, "create_canvas");
            canvas = new_frame(w, h, in->alpha, bg, true, hi.has_bg && !hi.bg_keyword_transparent);                    // format: parent.fmt (:96-105)
        }
        draw_image_exact(canvas, in, 0, 0, w, h, (bg >> 24) != 0, hi);                                                 // blend Overwrite iff bgcolor.is_transparent() (:176-184)
        // the canvas keeps parent.fmt: nothing in scaling.rs:50-90 or DrawImageDef::render clears alpha_meaningful after an
        // opaque matte (only the encoder-side Bitmap::apply_matte does, bitmaps.rs:528-541), so a later node still sees Bgra32
        return canvas;
    }

    // constrain (flow/nodes/constrain.rs:41-98 -> imageflow_riapi process_constraint, csrc/layout.cpp)
    static void constrain_params(const JVal& p, const char* node, std::string* mode, bool* has_w, bool* has_h, int64_t* tw, int64_t* th) {
        const JVal* jm = p.get("mode");
        *mode = jm && jm->t == JVal::Str ? jm->s : "";
        const JVal *jw = p.get("w"), *jh = p.get("h");
        *has_w = jw && jw->t == JVal::Num; *has_h = jh && jh->t == JVal::Num;
        *tw = *has_w ? want_u32(p, "w", node) : 0; *th = *has_h ? want_u32(p, "h", node) : 0;
    }
    FramePtr constrain(const FramePtr& in, const JVal& p) {
        std::string m;
        bool has_w, has_h;
        int64_t tw, th;
        constrain_params(p, "constrain", &m, &has_w, &has_h, &tw, &th);
        const int mode = ifhip::constraint_mode_from_name(m);
        if (mode < 0) raise(kInvalidJson, "InvalidJson: unknown constrain mode '%s'", m.c_str());
        float gx = 50.f, gy = 50.f;
        const bool has_gravity = parse_gravity(p.get("gravity"), &gx, &gy);
        ifhip::ConstraintLayout lay;
        std::string err;
        if (!ifhip::process_constraint(mode, static_cast<int32_t>(in->w), static_cast<int32_t>(in->h), has_w ? tw : -1, has_h ? th : -1, has_gravity, gx, gy, &lay, &err))
            raise(kArgumentInvalid, "InvalidNodeParams: Constraint error: %s", err.c_str());                              // constrain.rs:50-52
        FramePtr f = in;
        if (lay.has_crop) {                                                                                                // :55-57
            Timed t(this, "crop_mutate");
            f = crop_frame(f, lay.crop[0], lay.crop[1], lay.crop[2], lay.crop[3]);
        }
        // canvas_color overrides the hints' background_color (:60-76)
        const JVal* hints = p.get("hints");
        const JVal* cc = p.get("canvas_color");
        const bool has_cc = cc && !cc->is_null();
        JVal merged;
        if (has_cc) {
            if (hints && hints->t == JVal::Obj) merged = *hints;
            merged.t = JVal::Obj;
            bool set = false;
            for (auto& kv : merged.o) if (kv.first == "background_color") { kv.second = *cc; set = true; }
            if (!set) merged.o.emplace_back("background_color", *cc);
            hints = &merged;
        }
        f = resample(f, static_cast<uint32_t>(lay.scale_w), static_cast<uint32_t>(lay.scale_h), hints);                    // :78-82
        if (lay.has_pad) {                                                                                                 // :84-92: canvas_color or Transparent
            Timed t(this, "expand_canvas");
            f = expand_frame(f, lay.pad[0], lay.pad[1], lay.pad[2], lay.pad[3], has_cc ? parse_color(cc, "constrain.canvas_color") : 0u, !has_cc || keyword_transparent(cc));
        }
        return f;
    }
    // ConstraintGravity (imageflow_types lib.rs:1054-1061): "center" | {"percentage": {x, y}} -> false for centre / absent
    static bool parse_gravity(const JVal* g, float* gx, float* gy) {
        if (!g || g->is_null() || (g->t == JVal::Str && g->s == "center")) return false;
        const JVal* pc = g->get("percentage");
        const JVal *jx = pc ? pc->get("x") : nullptr, *jy = pc ? pc->get("y") : nullptr;
        if (!jx || !jy || jx->t != JVal::Num || jy->t != JVal::Num) raise(kInvalidJson, "InvalidJson: gravity is \"center\" or {\"percentage\":{x,y}}");
        *gx = static_cast<float>(jx->n); *gy = static_cast<float>(jy->n);
        return true;
    }
    // Crop (clone_crop_fill_expand.rs:519-541), materialised as a copy that keeps the parent's state
    FramePtr crop_frame(const FramePtr& in, uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2) {
        if (x2 <= x1 || y2 <= y1 || x2 > in->w || y2 > in->h) raise(kArgumentInvalid, "InvalidNodeParams: Invalid crop bounds");
        FramePtr cv = new_frame(x2 - x1, y2 - y1, in->alpha, 0, true);
        const int compose = in->compose;                                              // Bitmap::crop is a window onto the same bitmap
        const uint32_t matte = in->matte;                                             // (bitmaps.rs:841-859): its compositing mode stays
        copy_into_canvas(in, cv, x1, y1, x2 - x1, y2 - y1, 0, 0);
        cv->compose = compose; cv->matte = matte;
        return cv;
    }
    // CropWhitespace (clone_crop_fill_expand.rs:564-627): detect_content (graphics/whitespace.rs:284-334) on the device, the
    // 16-byte rectangle back with a wait for the job's stream only -- the crop box decides the next allocation, which is why
    // the reference's estimate is Impossible -- then the padding and the ordinary Crop, shared-parent handling included
    FramePtr crop_whitespace(const FramePtr& in, uint32_t threshold, float percent_padding, bool in_shared) {
        uint32_t rect[4];
        {
            Timed t(this, "crop_whitespace");
            uint32_t* d_rect = nullptr;
            hip_check(job_malloc(reinterpret_cast<void**>(&d_rect), 16), "hipMalloc(rect)");
            struct Guard { uint32_t* p; ~Guard() { job_free(p); } } g{d_rect};
            check(ifhip_detect_content_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, in->alpha ? 1 : 0, threshold, d_rect, t_job_stream));
            hip_check(hipMemcpyAsync(rect, d_rect, sizeof rect, hipMemcpyDeviceToHost, t_job_stream), "download(rect)");
            hip_check(static_cast<hipError_t>(ifhip::wait_stream(t_job_stream)), "crop_whitespace");
        }
        if (rect[2] <= rect[0] || rect[3] <= rect[1])                                 // :585-589
            raise(kInternalError, "InvalidState: Whitespace detection returned invalid rectangle");
        // `(percent_padding / 100f32 * (x2 - x1 + y2 - y1) as f32 / 2f32).ceil() as i64` (:590-593), saturating
        const float pf = std::ceil(percent_padding / 100.0f * static_cast<float>(rect[2] - rect[0] + rect[3] - rect[1]) / 2.0f);
        const int64_t pad = pf != pf ? 0 : pf >= 9.2233720e18f ? INT64_MAX : pf <= -9.2233720e18f ? INT64_MIN : static_cast<int64_t>(pf);
        // i64 sums wrap and `as u32` truncates, as in a release build
        auto add = [](int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b)); };
        const int64_t neg = static_cast<int64_t>(0ull - static_cast<uint64_t>(pad));
        const uint32_t x1 = static_cast<uint32_t>(std::max<int64_t>(0, add(rect[0], neg))), y1 = static_cast<uint32_t>(std::max<int64_t>(0, add(rect[1], neg)));
        const uint32_t x2 = static_cast<uint32_t>(std::min<int64_t>(in->w, add(rect[2], pad))), y2 = static_cast<uint32_t>(std::min<int64_t>(in->h, add(rect[3], pad)));
        Timed t(this, "crop_mutate");
        FramePtr cv = crop_frame(in, x1, y1, x2, y2);
        if (in_shared) { cv->compose = IFHIP_BLEND_WITH_SELF; cv->matte = 0; }        // as the Crop node below: MutProtect
        return cv;
    }
    // RoundImageCorners (flow/nodes/round_corners.rs:22-93): EnableTransparency first when the colour is not opaque (:30-34,
    // enable_transparency.rs:68-95), then the MutProtect'ed mutate node -- BlendWithSelf (:72-73) and
    // flow_bitmap_bgra_clear_around_rounded_corners (graphics/rounded_corners.rs:187-346) on the device.  radii: JSON order.
    FramePtr round_corners(const FramePtr& in, int mode, const float radii[4], uint32_t color) {
        if ((color >> 24) != 255u && !in->alpha) {
            check(ifhip_normalize_unused_alpha_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, 0, t_job_stream));
            in->alpha = true;
        }
        Timed t(this, "round_image_corners_mut");
        in->compose = IFHIP_BLEND_WITH_SELF; in->matte = 0;
        check(ifhip_round_corners_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, mode, radii, color, t_job_stream));
        return in;
    }
    // WhiteBalanceSrgbMutDef (flow/nodes/white_balance.rs:106-122): histograms, area thresholds and maps on the device;
    // threshold None is the f32 0.006 (:77)
    FramePtr white_balance(const FramePtr& in, float threshold) {
        Timed t(this, "white_balance_srgb_mut");
        check(ifhip_white_balance_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, threshold, nullptr, t_job_stream));
        return in;
    }
    // ExpandCanvas (:224-262): CreateCanvas of the colour (Bgra32 unless the colour is opaque) + CopyRectToCanvas
    FramePtr expand_frame(const FramePtr& in, uint32_t l, uint32_t t2, uint32_t r, uint32_t b, uint32_t color, bool color_is_keyword_transparent) {
        const uint64_t nw = static_cast<uint64_t>(in->w) + l + r, nh = static_cast<uint64_t>(in->h) + t2 + b;
        check_size(sec.max_frame_size, "max_frame_size", nw, nh);                     // before the 32-bit sums can wrap
        FramePtr cv = new_frame(static_cast<uint32_t>(nw), static_cast<uint32_t>(nh), (color >> 24) == 255 ? in->alpha : true, color, true, !color_is_keyword_transparent);
        return copy_into_canvas(in, cv, 0, 0, in->w, in->h, l, t2);
    }

    // command_string {kind: "ir4", value: "width=200&..."}: the querystring form of BASELINE config 1.  The text is parsed and
    // expanded by csrc/querystring.cpp (Instructions -> Ir4Layout::add_steps / Ir4Expand::get_decode_commands, the function
    // behind ifhip_shim_expand_command_string); what comes back -- decoder commands and a list of nodes in JSON -- runs through
    // run_node like any other step, so the `performance` block names the nodes the reference's expansion would.  The encoder
    // half (quality, jpeg.quality, format=jpg) is read here.
    FramePtr command_string(const JVal& p, FramePtr in, bool in_shared = false) {
        const JVal* kind = p.get("kind");
        const JVal* value = p.get("value");
        if (!kind || kind->t != JVal::Str || kind->s != "ir4" || !value || value->t != JVal::Str)
            raise(kInvalidJson, "InvalidJson: command_string needs kind \"ir4\" and a value");
        ifhip::Ir4Instructions qs;
        std::string err;
        auto answer = [&](int rc) {
            if (rc == ifhip::kQsRefused) raise(kActionNotSupported, "%s", err.c_str());
            if (rc != ifhip::kQsOk) raise(err.rfind("InvalidJson", 0) == 0 ? kInvalidJson : kArgumentInvalid, "%s", err.c_str());
        };
        answer(ifhip::parse_querystring(value->s, &qs, &err));
        std::string marks;
        if (const JVal* wm = p.get("watermarks")) if (!wm->is_null()) to_json(*wm, &marks);
        auto expansion = [&](uint32_t w, uint32_t h, uint32_t ref_w, uint32_t ref_h) {
            std::string json;
            answer(ifhip::expand_querystring(qs, static_cast<int32_t>(w), static_cast<int32_t>(h), static_cast<int32_t>(ref_w), static_cast<int32_t>(ref_h),
                                             marks.empty() ? nullptr : marks.c_str(), &json, &err));
            return parse_json(reinterpret_cast<const uint8_t*>(json.data()), json.size());
        };
        const JVal* dec = p.get("decode");
        const JVal* enc = p.get("encode");
        uint32_t src_w = 0, src_h = 0;
        // (the layout sees the frame BEHIND the decoder's orientation step, and the decoder hints are worked out from those
        // rotated sides and handed to the decoder as they are: command_string.rs:20-58, ir4/mod.rs:167-176)
        if (dec && dec->t == JVal::Num) image_size(static_cast<int32_t>(want_int(p, "decode", "command_string")), &src_w, &src_h, true);
        else if (in) { src_w = in->w; src_h = in->h; }
        else raise(kGraphInvalid, "GraphInvalid: command_string has neither a decode io nor an input frame");
        if (qs.trim_threshold.some) {
            // Ir4Expand::translate (ir4/mod.rs:97-121): a decode WITHOUT downscale hints, CropWhitespace on the decoded frame,
            // and the rest of the querystring laid out against the trimmed frame
            if (dec && dec->t == JVal::Num) { in = decode_oriented(static_cast<int32_t>(dec->n), 0, 0, false, false); dec = nullptr; }
            in = crop_whitespace(in, static_cast<uint32_t>(std::max<int32_t>(0, qs.trim_threshold.v)), qs.trim_padding, false);
            src_w = in->w; src_h = in->h;
        }
        if (dec && dec->t == JVal::Num) {
            // Ir4Expand::get_decode_commands against the file's size: discard_color_profile, the JPEG pre-shrink hints worked out
            // from the CROPPED window (get_downscaling), the WebP hint that goes out only with down.colorspace=srgb
            uint32_t hint_w = 0, hint_h = 0;
            bool spatial = qs.down_colorspace != ifhip::Ir4Instructions::kSrgb, gamma = spatial;
            Io& src = input(static_cast<int32_t>(dec->n));
            if (qs.ignoreicc.some && qs.ignoreicc.v) src.told_discard_profile = true;
            if (src_w) {
                const JVal ex = expansion(src_w, src_h, src_w, src_h);
                for (const JVal& cmd : ex.get("decoder_commands")->a) {
                    if (const JVal* j = cmd.get("jpeg_downscale_hints")) {
                        hint_w = want_u32(*j, "width", "jpeg_downscale_hints"); hint_h = want_u32(*j, "height", "jpeg_downscale_hints");
                        spatial = j->get("scale_luma_spatially")->b; gamma = j->get("gamma_correct_for_srgb_during_spatial_luma_scaling")->b;
                    } else if (cmd.get("webp_decoder_hints") && hint_w && is_webp(src)) { src.told_webp = true; src.told_webp_w = hint_w; src.told_webp_h = hint_h; }
                }
            }
            in = decode_oriented(static_cast<int32_t>(dec->n), hint_w, hint_h, spatial, gamma);
            if (!src_w) { src_w = in->w; src_h = in->h; }
        }
        // after a reduced decode the layout runs again on the decoded size, with the file's size as reference
        const JVal ex = expansion(in->w, in->h, src_w, src_h);
        const FramePtr given = in;
        FramePtr out = in;
        for (const JVal& n : ex.get("steps")->a) {
            std::string name;
            const JVal* params;
            node_of(n, &name, &params);
            bool shared = in_shared && out == given;
            if (shared && mutates_input(name)) { out = clone(out, true); shared = false; }            // the expansion's nodes are MutProtect where the graph's are
            if (name == "round_image_corners") {
                // (the radii as parsed, not through JSON: `s.roundcorners=nan` is a value the reference runs with)
                const double* q = qs.round_corners;
                const float radii[4] = {static_cast<float>(q[0]), static_cast<float>(q[1]), static_cast<float>(q[2]), static_cast<float>(q[3])};
                const bool all_eq = q[0] == q[1] && q[0] == q[2] && q[0] == q[3];
                out = round_corners(out, all_eq ? IFHIP_ROUND_CORNERS_PERCENTAGE : IFHIP_ROUND_CORNERS_PERCENTAGE_CUSTOM, radii, parse_color(params->get("background_color"), "round_image_corners.background_color"));
            } else out = run_node(name, *params, out, nullptr, shared);
        }
        if (enc && enc->t == JVal::Num) {
            // The reference keeps the source's format (a JPEG stays a JPEG, ir4/encoder.rs:30-37 OutputFormat::Keep) and hands
            // `jpeg.quality`, else `quality`, to its JPEG encoder (encoder.rs:74; 90 when neither is given, codecs/auto.rs).  Here a
            // querystring that names the format or a quality gets the classic JPEG writer with exactly that quality -- the
            // LIBJPEG-TURBO STYLE file (what the reference writes under jpeg.turbo=true); its default mozjpeg-style encoder
            // (trellis / scan search) is not built, so bytes and sizes differ from the reference's default for the same string
            // (README "Known differences", DESIGN "Encode").  One that names neither keeps this shim's labelled extension, the raw
            // BGRA container -- no key is accepted and then dropped.
            const int q = qs.jpeg_quality >= 0 ? qs.jpeg_quality : qs.quality;
            if (qs.jpeg_out || q >= 0) {
                JVal qv; qv.t = JVal::Num; qv.n = q >= 0 ? q : 90;
                JVal classic; classic.t = JVal::Obj; classic.o.emplace_back("quality", qv);
                JVal preset; preset.t = JVal::Obj; preset.o.emplace_back("libjpeg_turbo", classic);
                encode(out, static_cast<int32_t>(want_int(p, "encode", "command_string")), &preset, false);
            } else {
                encode(out, static_cast<int32_t>(want_int(p, "encode", "command_string")), nullptr, false);
            }
        }
        return out;
    }

    // The file a device coder writes for one frame: `pitch` bytes on the device, 16 to spare, and the coder's length and
    // status words behind it at `tail` (the pitch, rounded up as the coder's caller chooses).
    struct CodedFile {
        uint8_t* d = nullptr;
        uint32_t* d_len = nullptr;                                                   // length, status behind the file
        uint32_t len = 0, status = 0;
        ~CodedFile() { job_free(d); }
        hipError_t alloc(size_t pitch, size_t tail) {
            const hipError_t e = job_malloc(reinterpret_cast<void**>(&d), pitch + 16u);
            if (e == hipSuccess) d_len = reinterpret_cast<uint32_t*>(d + tail);
            return e;
        }
        void fetch(Io& o) {                                                          // after the coder's call; with status 0 the file goes into o.owned
            uint32_t len_status[2] = {0, 0};
            hip_check(static_cast<hipError_t>(ifhip::copy_to_host(len_status, d_len, 8)), "download(file length)");
            len = len_status[0]; status = len_status[1];
            if (status != 0 || len == 0) return;
            o.owned.assign(len, 0);
            hip_check(static_cast<hipError_t>(ifhip::copy_to_host(o.owned.data(), d, len)), "download(file)");
        }
    };

    // What a device coder's call in a job is named by: the label of its file's allocation, the coder in "dropped a file", the record.
    struct CoderNames { const char *label, *coder, *mime, *ext; };
    static constexpr CoderNames kPngNames{"hipMalloc(png file)", "PNG", "image/png", "png"}, kPalettePngNames{"hipMalloc(png file)", "palette PNG", "image/png", "png"},
        kWebpNames{"hipMalloc(webp file)", "WebP", "image/webp", "webp"}, kGifNames{"hipMalloc(gif file)", "GIF", "image/gif", "gif"};

    // Behind the stage: a file of `pitch` bytes, call(file) as the coder's one call on t_job_stream, and the file into `o`.
    // Returns the status word: 0 with the file written, or `lets_through` (not 0), which the caller answers itself.
    template <typename Call>
    uint32_t fetch_coded_file(Io& o, size_t pitch, const CoderNames& names, uint32_t lets_through, Call call) {
        CodedFile file;
        hip_check(file.alloc(pitch, pitch), names.label);
        check(call(file));
        poll_cancel();
        file.fetch(o);
        if (lets_through != 0 && file.status == lets_through) return file.status;
        if (file.status != 0 || file.len == 0) raise(kInternalError, "InternalError: the %s coder dropped a file sized for its worst case (status %u)", names.coder, file.status);
        o.written = true;
        return 0;
    }
    // One frame through a device file coder: create(&stage) for one image, a file of the stage's bound (rounded up to 16),
    // batch(stage, d_file, pitch, d_len) (d_len + 1: the status word), the file into `o` and its record.
    template <typename Stage, typename Create, typename Batch>
    uint32_t write_coded_frame(const FramePtr& f, Io& o, int32_t io_id, const CoderNames& names, uint32_t lets_through, Create create, void (*destroy)(Stage*),
                               size_t (*max_file_bytes)(const Stage*), Batch batch) {
        Stage* stage = nullptr;
        check(create(&stage));
        struct Guard { Stage* s; void (*destroy)(Stage*); ~Guard() { quiesce(); destroy(s); } } guard{stage, destroy};
        const size_t pitch = (max_file_bytes(stage) + 15u) & ~static_cast<size_t>(15u);
        const uint32_t status = fetch_coded_file(o, pitch, names, lets_through, [&](CodedFile& file) { return batch(stage, file.d, pitch, file.d_len); });
        if (status == 0) encodes.push_back({io_id, f->w, f->h, names.mime, names.ext});
        return status;
    }

    // a truecolour PNG of the frame by the device coder (csrc/png_encode.hip): only the file's bytes leave the device
    void write_png(const FramePtr& f, int color_type, int level, Io& o, int32_t io_id) {
        write_coded_frame(
            f, o, io_id, kPngNames, 0u, [&](ifhip_png_enc_stage** s) { return ifhip_png_enc_stage_create(s, f->w, f->h, color_type, 1); }, ifhip_png_enc_stage_destroy,
            ifhip_png_enc_stage_max_file_bytes, [&](ifhip_png_enc_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
                return ifhip_png_encode_batch_device(s, dev(f), f->bytes(), f->stride, 1, level, d_file, pitch, d_len, d_len + 1, t_job_stream);
            });
    }

    // encode: EncoderPreset::LibjpegTurbo is written as a real JPEG (codecs/mozjpeg.rs:78-160, create_classic :62-77):
    // apply_matte + forward DCT / quantisation on the device, the Huffman coder and the markers on the host
    // (csrc/jpeg_write.cpp) -- baseline, with optimize_huffman_coding libjpeg's optimal tables, with progressive its
    // standard scan script (:121-129).  The content-adaptive sampling choice
    // (evalchroma, an external crate) is not reproduced: the file uses the maximum the reference allows (:133, 4:2:0).
    // EncoderPreset::Libpng is written as a real PNG by the device coder (csrc/png_encode.hip), EncoderPreset::Pngquant as
    // a palette PNG by the device quantiser (csrc/png_quantize.hip), or losslessly where it misses minimum_quality.
    // EncoderPreset::WebPLossless is written as a real lossless WebP by the device coder (csrc/webp_encode.hip).
    // EXTENSION: every other preset writes the raw BGRA container (lodepng / lossy WebP coders are out of scope) -- "gif" too,
    // unless the context's GIF encoder is switched on (ifhip_shim_context_set_gif_encoder): then it is a GIF89a file of the device coder.
    // `shared`: other consumers still read this frame -- the matte is then applied to a private copy.
    void encode(FramePtr f, int32_t io_id, const JVal* preset, bool shared) {
        Timed t(this, "primitive_encoder");
        Io& o = output(io_id);
        if (o.out_state == OutState::Taken) raise(kArgumentInvalid, "InvalidArgument: Output buffer for io_id %d has already been taken", io_id);
        poll_cancel();
        if (anim.active) {                                                           // every frame to the "gif" nodes, frame 0 to every other encoder
            if (preset && preset->t == JVal::Str && preset->s == "gif") { collect_frame(f, io_id); return; }
            if (anim.k > 0) return;
        }
        const int coder = encode_coder(preset);
        // EncoderPreset::Mozjpeg {quality, progressive, matte} -> MozjpegEncoder::create (codecs/mozjpeg.rs:37-59): mozjpeg's own
        // defaults.  Of those the trellis quantisation is built (csrc/jpeg_trellis.hip, this project's restatement of
        // jcdctmgr.c quantize_trellis, AC only) between the raw forward stage and the device entropy coder; tables are always
        // optimised (:56) and the file always progressive (`progressive` only ever switches it on, :121-125, over defaults
        // that already are).  Annex K tables, libjpeg's standard scan script, no deringing, 4:2:0.
        const bool moz = coder == IFHIP_ENCODE_CODER_MOZJPEG;
        const JVal* classic = coder == IFHIP_ENCODE_CODER_JPEG ? preset->get("libjpeg_turbo") : moz ? preset->get("mozjpeg") : nullptr;
        if (classic) return encode_jpeg(f, o, io_id, preset, classic, moz, shared);
        if (const JVal* png = coder == IFHIP_ENCODE_CODER_PNG ? preset->get("libpng") : nullptr) return encode_png(f, o, io_id, png, shared);
        if (const JVal* pq = coder == IFHIP_ENCODE_CODER_PNGQUANT ? preset->get("pngquant") : nullptr) return encode_pngquant(f, o, io_id, pq);
        if (coder == IFHIP_ENCODE_CODER_WEBP_LOSSLESS) return encode_webp_lossless(f, o, io_id);
        if (preset && preset->t == JVal::Str && preset->s == "gif" && c->gif_encoder.load(std::memory_order_relaxed)) return encode_gif(f, o, io_id);
        if (names_webplossy(preset) && c->webp_lossy_encoder.load(std::memory_order_relaxed)) return encode_webp_lossy(f, o, io_id, preset);
        encode_raw(f, o, io_id);
    }

    // the libjpeg_turbo and mozjpeg presets: `classic` is the preset's object
    void encode_jpeg(FramePtr f, Io& o, int32_t io_id, const JVal* preset, const JVal* classic, bool moz, bool shared) {
        auto flag = [&](const char* k) { const JVal* v = classic->get(k); return v && v->t == JVal::Bool && v->b; };
        const int write_flags = moz ? (IFHIP_JPEG_PROGRESSIVE | IFHIP_JPEG_OPTIMIZE_HUFFMAN)
                                    : (flag("progressive") ? IFHIP_JPEG_PROGRESSIVE : 0) | (flag("optimize_huffman_coding") ? IFHIP_JPEG_OPTIMIZE_HUFFMAN : 0);
        const JVal* q = classic->get("quality");
        int quality = 75;                                                            // mozjpeg.rs:32 DEFAULT_QUALITY
        if (moz) check_mozjpeg_preset(preset);
        if (moz && q && q->t == JVal::Num) quality = std::min(100, static_cast<int>(q->n));   // Option<u8> -> u8::min(100, ..) (mozjpeg.rs:53)
        // Option<i32> -> `q as u8` (codecs/auto.rs:201: the value WRAPS, 300 is 44 and -5 is 251) -> u8::min(100, ..) (mozjpeg.rs:71)
        if (!moz && q && q->t == JVal::Num) {
            if (q->n != std::floor(q->n) || q->n < -2147483648.0 || q->n > 2147483647.0) raise(kInvalidJson, "InvalidJson: encode.preset.libjpeg_turbo.quality is a 32-bit integer");
            quality = std::min(100, static_cast<int>(static_cast<uint8_t>(static_cast<int32_t>(q->n))));
        }
        const JVal* m = classic->get("matte");
        const uint32_t matte = m && !m->is_null() ? parse_color(m, moz ? "encode.preset.mozjpeg.matte" : "encode.preset.libjpeg_turbo.matte") : 0xFFFFFFFFu;   // :88-92
        if (shared && f->alpha) f = clone(f);
        check(ifhip_apply_matte_batch_device(dev(f), f->bytes(), 1, f->w, f->h, f->stride, f->alpha ? 1 : 0, matte, t_job_stream));
        f->alpha = false;                                                            // :94 set_alpha_meaningful(false)
        const uint8_t hs[3] = {2, 1, 1}, vs[3] = {2, 1, 1};
        uint16_t qt2[2][64], qt3[3][64];
        ifhip_jpeg_quality_tables(quality, &qt2[0][0]);
        std::memcpy(qt3[0], qt2[0], 128); std::memcpy(qt3[1], qt2[1], 128); std::memcpy(qt3[2], qt2[1], 128);
        ifhip_jpeg_fwd_stage* st = nullptr;
        check(ifhip_jpeg_fwd_stage_create(&st, f->w, f->h, hs, vs, 1));
        std::unique_ptr<ifhip_jpeg_fwd_stage, void (*)(ifhip_jpeg_fwd_stage*)> st_guard(st, ifhip_jpeg_fwd_stage_destroy);
        uint32_t bw[3], bh[3];
        check(ifhip_jpeg_fwd_stage_block_dims(st, bw, bh));
        size_t off[4] = {0, 0, 0, 0};
        for (int k = 0; k < 3; ++k) off[k + 1] = off[k] + static_cast<size_t>(bw[k]) * bh[k] * 64u;
        int16_t* d_coef = nullptr;
        uint16_t* d_qt = nullptr;
        // (the mozjpeg preset: the raw planes of the trellis stage lie behind the quantised ones)
        hip_check(job_malloc(reinterpret_cast<void**>(&d_coef), off[3] * (moz ? 4u : 2u) + 384u), "hipMalloc(coefficients)");
        std::unique_ptr<int16_t, void (*)(int16_t*)> coef_guard(d_coef, [](int16_t* p) { job_free(p); });
        int16_t* d_raw = d_coef + off[3];
        d_qt = reinterpret_cast<uint16_t*>(d_coef + off[3] * (moz ? 2u : 1u));
        hip_check(static_cast<hipError_t>(ifhip::copy_to_device(d_qt, qt3, 384)), "upload(quant tables)");
        if (moz) {
            ifhip_jpeg_trellis_stage* ts = nullptr;
            check(ifhip_jpeg_trellis_stage_create(&ts, f->w, f->h, hs, vs, 1));
            std::unique_ptr<ifhip_jpeg_trellis_stage, void (*)(ifhip_jpeg_trellis_stage*)> ts_guard(ts, [](ifhip_jpeg_trellis_stage* q) { quiesce(); ifhip_jpeg_trellis_stage_destroy(q); });
            check(ifhip_jpeg_forward_raw_batch_device(st, dev(f), f->bytes(), f->stride, 1, d_raw + off[0], d_raw + off[1], d_raw + off[2], t_job_stream));
            check(ifhip_jpeg_trellis_batch_device(ts, d_raw + off[0], d_raw + off[1], d_raw + off[2], d_qt, IFHIP_JPEG_TRELLIS_LAMBDA_ONE, 1, d_coef + off[0],
                                                  d_coef + off[1], d_coef + off[2], t_job_stream));
        } else {
            check(ifhip_jpeg_forward_batch_device(st, dev(f), f->bytes(), f->stride, d_qt, 1, d_coef + off[0], d_coef + off[1], d_coef + off[2], t_job_stream));
        }
        poll_cancel();
        // (the mozjpeg preset goes to the device coder without the switch: that guards what older callers pinned for libjpeg_turbo)
        if (write_flags == 0 || moz || c->device_jpeg_options.load(std::memory_order_relaxed)) {
            // the preset's default (baseline, Annex K tables) -- and, where the caller switched it on
            // (ifhip_shim_context_set_device_jpeg_options), progressive / optimize_huffman_coding:
            // the device entropy coder -- only the file leaves the device.
            // First with room for a scan half the size of its coefficients (what the host path assumes too), then, for an
            // image that is denser than that, with the geometry's worst case.
            for (int attempt = 0; attempt < 2; ++attempt) {
                const size_t scan_cap = attempt == 0 ? std::max<size_t>(65536u, off[3]) : 0u;
                // A geometry the coder does not take (more than 2.58 M blocks: a `security` override above ~110 MP) or a
                // stage that cannot be allocated is not the job's failure: the host writer below codes the same file.
                ifhip_jpeg_enc_stage* es = nullptr;
                if (ifhip_jpeg_enc_stage_create(&es, f->w, f->h, 3, hs, vs, bw, bh, 1, scan_cap) != IFHIP_OK) break;
                std::unique_ptr<ifhip_jpeg_enc_stage, void (*)(ifhip_jpeg_enc_stage*)> es_guard(es, [](ifhip_jpeg_enc_stage* q) { quiesce(); ifhip_jpeg_enc_stage_destroy(q); });
                const size_t pitch = ifhip_jpeg_enc_stage_max_file_bytes_for(es, write_flags);
                if (pitch == 0) break;                                               // (the flagged forms refuse the geometry)
                CodedFile file;
                if (file.alloc(pitch, (pitch + 3u) & ~static_cast<size_t>(3u)) != hipSuccess) break;
                // (a flagged call allocates its scratch first; where that fails the host writer codes the file)
                const int erc = ifhip_jpeg_encode_flags_batch_device(es, d_coef + off[0], d_coef + off[1], d_coef + off[2], quality, write_flags, 1, file.d,
                                                                     pitch, file.d_len, file.d_len + 1, t_job_stream);
                if (erc != IFHIP_OK && write_flags != 0) break;
                check(erc);
                file.fetch(o);
                if (file.status & IFHIP_ENC_BAD_COEFFICIENT)
                    raise(kArgumentInvalid, "InvalidArgument: coefficient out of range for 8-bit JPEG (more than 11 DC / 10 AC magnitude bits)");
                if (file.status != 0) continue;
                o.written = true;
                encodes.push_back({io_id, f->w, f->h, "image/jpeg", "jpg"});
                c->device_coded_files.fetch_add(1, std::memory_order_relaxed);
                return;
            }
        }                                                                            // (not coded on the device: the host writer)
        write_jpeg_on_host(f, o, io_id, d_coef, off, bw, bh, hs, vs, quality, write_flags);
    }
    // the coefficients back to the host, Huffman coding and markers there (csrc/jpeg_write.cpp)
    void write_jpeg_on_host(const FramePtr& f, Io& o, int32_t io_id, const int16_t* d_coef, const size_t off[4], const uint32_t bw[3], const uint32_t bh[3],
                            const uint8_t hs[3], const uint8_t vs[3], int quality, int write_flags) {
        std::vector<int16_t> coef(off[3]);
        hip_check(static_cast<hipError_t>(ifhip::copy_to_host(coef.data(), d_coef, off[3] * 2u)), "download(coefficients)");
        size_t len = 0;
        o.owned.assign(std::max<size_t>(4096u, off[3]), 0);                          // a file is smaller than its coefficients: one pass
        int wrc = ifhip_jpeg_write(coef.data() + off[0], coef.data() + off[1], coef.data() + off[2], bw, bh, 3, hs, vs, f->w, f->h, quality, write_flags,
                                   o.owned.data(), o.owned.size(), &len);
        if (wrc != IFHIP_OK && len > o.owned.size()) {
            o.owned.assign(len, 0);
            wrc = ifhip_jpeg_write(coef.data() + off[0], coef.data() + off[1], coef.data() + off[2], bw, bh, 3, hs, vs, f->w, f->h, quality, write_flags,
                                   o.owned.data(), o.owned.size(), &len);
        }
        check(wrc);
        o.owned.resize(len);
        o.written = true;
        encodes.push_back({io_id, f->w, f->h, "image/jpeg", "jpg"});
        return;
    }
    void encode_png(FramePtr f, Io& o, int32_t io_id, const JVal* png, bool shared) {
        // EncoderPreset::Libpng {depth, matte, zlib_compression} (imageflow_types/src/lib.rs:751-755, codecs/auto.rs:241-268)
        // -> LibPngEncoder::write_frame (codecs/libpng_encoder.rs:43-72): the file is coded on the device
        // (csrc/png_encode.hip), only its bytes leave it.
        int color_type = -1;                                                         // by the frame's alpha, below
        if (const JVal* d = png->get("depth"); d && !d->is_null()) {
            if (d->t != JVal::Str || (d->s != "png_32" && d->s != "png_24")) raise(kInvalidJson, "InvalidJson: encode.preset.libpng.depth is \"png_32\" or \"png_24\"");
            if (d->s == "png_24") color_type = IFHIP_PNG_RGB;
        }
        int level = -1;                                                              // absent: zlib's default (6)
        if (const JVal* z = png->get("zlib_compression"); z && !z->is_null()) {
            if (z->t != JVal::Num || z->n != std::floor(z->n) || z->n < -2147483648.0 || z->n > 2147483647.0)
                raise(kInvalidJson, "InvalidJson: encode.preset.libpng.zlib_compression is a 32-bit integer");
            // i32 clamped to 0..255 (auto.rs:265); above 9 libpng is left at its default (codec_png_wrapper.c:380-387)
            const int v = static_cast<int>(std::min(255.0, std::max(0.0, z->n)));
            level = v > 9 ? -1 : v;
        }
        const JVal* m = png->get("matte");
        if (m && !m->is_null() && f->alpha) {                                       // libpng_encoder.rs:55-57, bitmaps.rs:528-541
            const uint32_t matte = parse_color(m, "encode.preset.libpng.matte");
            if (shared) f = clone(f);
            check(ifhip_apply_matte_batch_device(dev(f), f->bytes(), 1, f->w, f->h, f->stride, 1, matte, t_job_stream));
            if ((matte >> 24) == 0xFFu) f->alpha = false;                            // matte.is_opaque(): set_alpha_meaningful(false)
        } else if (m && !m->is_null()) {
            (void)parse_color(m, "encode.preset.libpng.matte");                      // (still parsed: a malformed colour is an error)
        }
        if (color_type < 0) color_type = f->alpha ? IFHIP_PNG_RGBA : IFHIP_PNG_RGB;  // codec_png_wrapper.c:402-410
        write_png(f, color_type, level, o, io_id);
        return;
    }
    void encode_pngquant(const FramePtr& f, Io& o, int32_t io_id, const JVal* pq) {
        // EncoderPreset::Pngquant {quality, minimum_quality, speed, maximum_deflate} (imageflow_types/src/lib.rs:756-761)
        // -> PngquantEncoder (codecs/pngquant.rs:35-139): quantised, dithered and written as a palette PNG on the device
        // (csrc/png_quantize.hip); no matte (codecs/auto.rs:98-110).  The three numbers are u8.
        auto u8_option = [&](const char* key) -> int {
            const JVal* v = pq->get(key);
            if (!v || v->is_null()) return -1;
            if (v->t != JVal::Num || v->n != std::floor(v->n) || v->n < 0.0 || v->n > 255.0) raise(kInvalidJson, "InvalidJson: encode.preset.pngquant.%s is an integer in 0..255", key);
            return static_cast<int>(v->n);
        };
        const int quality = u8_option("quality"), min_quality = u8_option("minimum_quality"), speed = u8_option("speed");
        bool maximum_deflate = false;
        if (const JVal* z = pq->get("maximum_deflate"); z && !z->is_null()) {
            if (z->t != JVal::Bool) raise(kInvalidJson, "InvalidJson: encode.preset.pngquant.maximum_deflate is a boolean");
            maximum_deflate = z->b;
        }
        const int level = maximum_deflate ? 9 : 6;                                    // lode.rs:162-195
        const uint32_t status = write_coded_frame(
            f, o, io_id, kPalettePngNames, IFHIP_PNG_QUALITY_TOO_LOW, [&](ifhip_png_quant_stage** s) { return ifhip_png_quant_stage_create(s, f->w, f->h, 1); },
            ifhip_png_quant_stage_destroy, ifhip_png_quant_stage_max_file_bytes, [&](ifhip_png_quant_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
                return ifhip_png_quantize_batch_device(s, dev(f), f->bytes(), f->stride, f->alpha ? 1 : 0, 1, quality, min_quality, speed, 256, 1, level, d_file, pitch,
                                                       d_len, d_len + 1, nullptr, nullptr, nullptr, t_job_stream);
            });
        // pngquant.rs:105-139: below minimum_quality the frame is written losslessly, RGBA or RGB by its alpha
        if (status == IFHIP_PNG_QUALITY_TOO_LOW) write_png(f, f->alpha ? IFHIP_PNG_RGBA : IFHIP_PNG_RGB, level, o, io_id);
        return;
    }
    void encode_webp_lossless(const FramePtr& f, Io& o, int32_t io_id) {
        // EncoderPreset::WebPLossless (imageflow_types/src/lib.rs:773, codecs/auto.rs:282-319) -> WebPEncoder::write_frame
        // (codecs/webp.rs:281-345: WebPEncodeLosslessBGRA, or ...BGR when the frame's alpha is not meaningful); no matte
        // (the reference passes None).  The file is coded on the device (csrc/webp_encode.hip), only its bytes leave it.
        // The stage is made per frame with the context's flags (ifhip_shim_context_set_webp_lossless_flags), so none outlives a change of them.
        const uint32_t flags = c->webp_lossless_flags.load(std::memory_order_relaxed);
        write_coded_frame(
            f, o, io_id, kWebpNames, 0u, [&](ifhip_webp_enc_stage** s) { return ifhip_webp_enc_stage_create_flags(s, f->w, f->h, f->alpha ? 1 : 0, 1, flags); },
            ifhip_webp_enc_stage_destroy, ifhip_webp_enc_stage_max_file_bytes, [&](ifhip_webp_enc_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
                return ifhip_webp_encode_batch_device(s, dev(f), f->bytes(), f->stride, 1, d_file, pitch, d_len, d_len + 1, t_job_stream);
            });
        return;
    }
    void encode_gif(const FramePtr& f, Io& o, int32_t io_id) {
        // EXTENSION (ifhip_shim_context_set_gif_encoder): EncoderPreset::Gif -> GifEncoder::write_frame (codecs/gif/mod.rs:385-592):
        // the alpha rule, the palette and the LZW stream on the device (csrc/gif_encode.hip), only the file leaves it.  The
        // frame itself is left as it is (the rule is applied where the pixels are read); a side above 65535 is size_16()'s
        // InvalidArgument.  A GIF decoder of the job hands on its repeat count and its last frame's delay and user-input flag.
        write_coded_frame(
            f, o, io_id, kGifNames, 0u, [&](ifhip_gif_enc_stage** s) { return ifhip_gif_enc_stage_create(s, f->w, f->h, 1); }, ifhip_gif_enc_stage_destroy,
            ifhip_gif_enc_stage_max_file_bytes, [&](ifhip_gif_enc_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
                return ifhip_gif_encode_batch_device(s, dev(f), f->bytes(), f->stride, f->alpha ? 1 : 0, 1, gif_source.seen ? gif_source.repeat : -1, gif_source.delay,
                                                     gif_source.user_input ? 1 : 0, d_file, pitch, d_len, d_len + 1, nullptr, nullptr, t_job_stream);
            });
        return;
    }
    void encode_webp_lossy(const FramePtr& f, Io& o, int32_t io_id, const JVal* preset) {
        // EXTENSION (ifhip_shim_context_set_webp_lossy_encoder): EncoderPreset::WebPLossy {quality} -> WebPEncoder::write_frame
        // (codecs/webp.rs: WebPEncodeBGRA, or ...BGR when the frame's alpha is not meaningful; quality clamped to 0..100); no matte.
        // The file is coded on the device (csrc/vp8_encode.hip), only its bytes leave it.  libwebp returns nothing for a side
        // above 16383, which the reference answers with ImageEncodingError.  The switch's value 2 adds the 4x4 luma modes.
        const float quality = check_webplossy_preset(preset);
        const uint32_t flags = c->webp_lossy_intra4.load(std::memory_order_relaxed) ? IFHIP_VP8_ENC_INTRA4 : 0u;
        if (f->w > 16383u || f->h > 16383u) raise(kInternalError, "ImageEncodingError: libwebp encoding error");
        write_coded_frame(
            f, o, io_id, kWebpNames, 0u, [&](ifhip_webp_lossy_enc_stage** s) { return ifhip_webp_lossy_enc_stage_create_flags(s, f->w, f->h, f->alpha ? 1 : 0, 1, flags); },
            ifhip_webp_lossy_enc_stage_destroy, ifhip_webp_lossy_enc_stage_max_file_bytes, [&](ifhip_webp_lossy_enc_stage* s, uint8_t* d_file, size_t pitch, uint32_t* d_len) {
                return ifhip_webp_lossy_encode_batch_device(s, dev(f), f->bytes(), f->stride, 1, quality, d_file, pitch, d_len, d_len + 1, t_job_stream);
            });
        return;
    }
    // EXTENSION: the raw BGRA container
    void encode_raw(const FramePtr& f, Io& o, int32_t io_id) {
        o.owned.assign(kRawHeader + f->bytes(), 0);
        std::memcpy(o.owned.data(), kRawMagic, 8);
        const uint32_t hdr[4] = {f->w, f->h, f->stride, f->alpha ? 1u : 0u};
        std::memcpy(o.owned.data() + 8, hdr, 16);
        { uint8_t* src = dev(f); hip_check(static_cast<hipError_t>(ifhip::copy_to_host(o.owned.data() + kRawHeader, src, f->bytes())), "download(frame)"); }
        o.written = true;
        encodes.push_back({io_id, f->w, f->h, "application/x-imageflow-bgra", "ifbgra"});
    }

    // CopyRectNodeDef::render (flow/nodes/clone_crop_fill_expand.rs:31-90)
    FramePtr copy_into_canvas(const FramePtr& in, const FramePtr& canvas, uint32_t fx, uint32_t fy, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
        if (in == canvas) raise(kGraphInvalid, "InvalidNodeConnections: Canvas and Input are the same bitmap!");
        if (in->w <= fx || in->h <= fy || in->w < static_cast<uint64_t>(fx) + w || in->h < static_cast<uint64_t>(fy) + h ||
            canvas->w < static_cast<uint64_t>(x) + w || canvas->h < static_cast<uint64_t>(y) + h)
            raise(kArgumentInvalid, "InvalidNodeParams: Invalid coordinates. Canvas is %ux%u, Input is %ux%u, Params provided: from_x=%u from_y=%u w=%u h=%u x=%u y=%u",
                  canvas->w, canvas->h, in->w, in->h, fx, fy, w, h, x, y);
        int canvas_alpha = canvas->alpha ? 1 : 0;
        check(ifhip_copy_rect_batch_device(dev(in), in->bytes(), in->w, in->h, in->stride, in->alpha ? 1 : 0, dev(canvas), canvas->bytes(),
                                           canvas->w, canvas->h, canvas->stride, &canvas_alpha, fx, fy, x, y, w, h, 1, t_job_stream));
        canvas->alpha = canvas_alpha != 0;
        canvas->compose = IFHIP_BLEND_WITH_SELF;                                       // copy_rect.rs:37
        hip_check(static_cast<hipError_t>(ifhip::wait_stream(t_job_stream)), "copy_rect");
        return canvas;
    }
    FramePtr transposed(const FramePtr& in) {
        FramePtr t = new_frame(in->h, in->w, in->alpha, 0, true);
        check(ifhip_transpose_batch_device(dev(in), in->bytes(), in->w, in->h, in->stride, t->d, t->bytes(), t->w, t->h, t->stride, 1, t_job_stream));
        return t;
    }
    FramePtr flip(const FramePtr& in, bool vertical) {
        check(vertical ? ifhip_flip_vertical_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, t_job_stream)
                       : ifhip_flip_horizontal_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, t_job_stream));
        return in;
    }
    // ApplyOrientationDef::expand (flow/nodes/rotate_flip_transpose.rs:44-66): the EXIF flag as flips and a transpose
    FramePtr apply_orientation(const FramePtr& in, int64_t flag) {
        switch (flag) {
        case 2: return flip(in, false);
        case 3: return flip(flip(in, true), false);
        case 4: return flip(in, true);
        case 5: return transposed(in);
        case 6: return flip(transposed(in), false);
        case 7: return transposed(flip(flip(in, true), false));
        case 8: return flip(transposed(in), true);
        default: return in;
        }
    }
    // DecoderDef::expand (flow/nodes/codecs_and_pointer.rs:94-107): a decode whose input carries an EXIF orientation
    // above 0 is followed by ApplyOrientation {flag}.  Flag 1 is the identity -- the frame stays a pending JPEG, so that
    // decode + resample remain one device call; the others need the bitmap.
    FramePtr decode_oriented(int32_t io_id, uint32_t hint_w, uint32_t hint_h, bool luma_spatial, bool luma_srgb) {
        FramePtr f = decode(io_id, hint_w, hint_h, luma_spatial, luma_srgb);
        const int flag = exif_flag(input(io_id));
        if (flag < 2) return f;
        Timed t(this, "apply_orientation");
        return apply_orientation(f, flag);
    }
    // ColorMatrixSrgbMutDef::mutate (flow/nodes/color.rs:20-38)
    FramePtr color_matrix(const FramePtr& in, const float m[25]) {
        check(ifhip_apply_color_matrix_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, m, t_job_stream));
        in->compose = IFHIP_BLEND_WITH_SELF;
        return in;
    }
    // ColorFilterSrgb::expand (flow/nodes/color.rs:49-83) with the matrices of :86-230
    FramePtr color_filter(const FramePtr& in, const JVal& p) {
        float m[25] = {1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1};
        auto gray = [&](float r, float g, float b) { const float v[25] = {r, r, r, 0, 0, g, g, g, 0, 0, b, b, b, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1}; std::memcpy(m, v, sizeof v); };
        std::string name;
        float a = 0.f;
        if (p.t == JVal::Str) name = p.s;
        else if (p.t == JVal::Obj && p.o.size() == 1 && p.o[0].second.t == JVal::Num) { name = p.o[0].first; a = static_cast<float>(p.o[0].second.n); }
        else raise(kInvalidJson, "InvalidJson: color_filter_srgb is a name or {name: value}");
        if (name == "sepia") { const float v[25] = {0.393f, 0.349f, 0.272f, 0, 0, 0.769f, 0.686f, 0.534f, 0, 0, 0.189f, 0.168f, 0.131f, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0}; std::memcpy(m, v, sizeof v); }
        else if (name == "grayscale_ntsc") gray(0.229f, 0.587f, 0.114f);
        else if (name == "grayscale_ry") gray(0.5f, 0.419f, 0.081f);
        else if (name == "grayscale_flat") gray(0.5f, 0.5f, 0.5f);
        else if (name == "grayscale_bt709") gray(0.2125f, 0.7154f, 0.0721f);
        else if (name == "invert") { m[0] = m[6] = m[12] = -1.f; m[20] = m[21] = m[22] = 1.f; }
        else if (name == "alpha") m[18] = a;
        else if (name == "contrast") { const float c2 = a + 1.f, t = 0.5f * (1.f - c2); m[0] = m[6] = m[12] = c2; m[20] = m[21] = m[22] = t; }
        else if (name == "brightness") m[20] = m[21] = m[22] = a;
        else if (name == "saturation") {
            const float s = std::max(a + 1.f, 0.f), c2 = 1.f - s, cr = 0.3086f * c2, cg = 0.6094f * c2, cb = 0.0820f * c2;
            const float v[25] = {cr + s, cr, cr, 0, 0, cg, cg + s, cg, 0, 0, cb, cb, cb + s, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1};
            std::memcpy(m, v, sizeof v);
        } else raise(kInvalidJson, "InvalidJson: unknown color_filter_srgb '%s'", name.c_str());
        if (name == "alpha" && !in->alpha) {                                          // EnableTransparency (enable_transparency.rs:68-95)
            check(ifhip_normalize_unused_alpha_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, 0, t_job_stream));
            in->alpha = true;
        }
        return color_matrix(in, m);
    }

    // WatermarkDef::expand (flow/nodes/watermark.rs:100-196): decode -> [crop] -> [alpha(opacity)] -> DrawImageExact
    // (Compose) onto the input frame.  As the reference, the constraint is built with `hints: None`, so the node's
    // own `hints` never reach the resampler (:121-128, :176).
    FramePtr watermark(const FramePtr& canvas, const JVal& p) {
        const int32_t io_id = static_cast<int32_t>(want_int(p, "io_id", "watermark"));
        auto opt_u32 = [&](const char* k) -> uint32_t { const JVal* v = p.get(k); return v && v->t == JVal::Num ? want_u32(p, k, "watermark") : 0u; };
        if (!(opt_u32("min_canvas_width") < canvas->w && opt_u32("min_canvas_height") < canvas->h)) return canvas;       // :109-111
        // get_bounding_box (:11-58)
        int64_t bx1 = 0, by1 = 0, bx2 = canvas->w, by2 = canvas->h;
        if (const JVal* fb = p.get("fit_box"))
            if (!fb->is_null()) {
                const JVal* margins = fb->get("image_margins") ? fb->get("image_margins") : fb->get("canvas_margins");
                const JVal* pct = fb->get("image_percentage") ? fb->get("image_percentage") : fb->get("canvas_percentage");
                if (margins) {
                    const int64_t l = want_u32(*margins, "left", "fit_box"), t = want_u32(*margins, "top", "fit_box"), r = want_u32(*margins, "right", "fit_box"), b = want_u32(*margins, "bottom", "fit_box");
                    if (!(l + r < canvas->w && t + b < canvas->h)) return canvas;
                    bx1 = l; by1 = t; bx2 = static_cast<int64_t>(canvas->w) - r; by2 = static_cast<int64_t>(canvas->h) - b;
                } else if (pct) {
                    auto num = [&](const char* k) { const JVal* v = pct->get(k); if (!v || v->t != JVal::Num) raise(kInvalidJson, "InvalidJson: fit_box.%s must be a number", k); return static_cast<float>(v->n); };
                    auto to_px = [](float percent, uint32_t size) { const float ratio = std::min(std::max(percent, 0.f), 100.f) / 100.f; return static_cast<int64_t>(std::round(ratio * static_cast<float>(size))); };
                    bx1 = to_px(num("x1"), canvas->w); by1 = to_px(num("y1"), canvas->h); bx2 = to_px(num("x2"), canvas->w); by2 = to_px(num("y2"), canvas->h);
                    if (!(bx1 < bx2 && by1 < by2)) return canvas;
                } else raise(kInvalidJson, "InvalidJson: unknown watermark fit_box");
            }
        const JVal* fm = p.get("fit_mode");
        const std::string mode = fm && fm->t == JVal::Str ? fm->s : "within";                                            // :121
        if (mode != "within" && mode != "fit" && mode != "distort" && mode != "within_crop" && mode != "fit_crop")       // WatermarkConstraintMode (lib.rs:1022-1040)
            raise(kInvalidJson, "InvalidJson: unknown watermark fit_mode '%s'", mode.c_str());
        uint32_t mw = 0, mh = 0;
        image_size(io_id, &mw, &mh, true);                                                                                // get_scaled_rotated_image_info (:128)
        float gx = 50.f, gy = 50.f;                                                                                       // obey_gravity (:69-86)
        const bool has_gravity = parse_gravity(p.get("gravity"), &gx, &gy);
        // Constraint {mode, w: box_w, h: box_h, hints: None, gravity, canvas_color: None} -> process_constraint (:121-139)
        ifhip::ConstraintLayout lay;
        std::string err;
        if (!ifhip::process_constraint(ifhip::constraint_mode_from_name(mode), static_cast<int32_t>(mw), static_cast<int32_t>(mh), bx2 - bx1, by2 - by1,
                                       has_gravity, gx, gy, &lay, &err))
            raise(kArgumentInvalid, "InvalidNodeParams: Constraint error: %s", err.c_str());                              // (the reference unwraps: a panic)
        const uint32_t w = static_cast<uint32_t>(lay.scale_w), h = static_cast<uint32_t>(lay.scale_h);
        auto gravity1d = [](float pct, int64_t inner, int64_t outer) -> int64_t {                                         // :60-67
            const float ratio = std::min(std::max(pct, 0.f), 100.f) / 100.f;
            if ((outer < inner && inner < 1) || outer < 1) raise(kArgumentInvalid, "InvalidNodeParams: Watermark fit_box does not work");
            return static_cast<int64_t>(std::round(static_cast<float>(outer - inner) * ratio));
        };
        const int64_t x1 = gravity1d(gx, w, bx2 - bx1) + bx1, y1 = gravity1d(gy, h, by2 - by1) + by1;
        if (x1 < 0 || y1 < 0) raise(kArgumentInvalid, "InvalidNodeParams: Watermark fit_box does not work");
        FramePtr mark = decode_oriented(io_id, 0, 0, false, false);
        if (lay.has_crop) {                                                                                              // :157-164
            Timed t(this, "crop_mutate");
            mark = crop_frame(mark, lay.crop[0], lay.crop[1], lay.crop[2], lay.crop[3]);
        }
        float opacity = 1.f;
        if (const JVal* o = p.get("opacity")) if (o->t == JVal::Num) opacity = std::min(std::max(static_cast<float>(o->n), 0.f), 1.f);
        if (opacity < 1.f) {                                                                                             // :166-172
            Timed t(this, "color_matrix_srgb_mut");
            JVal f; f.t = JVal::Obj;
            JVal v; v.t = JVal::Num; v.n = static_cast<double>(opacity);
            f.o.emplace_back("alpha", v);
            color_filter(mark, f);
        }
        draw_image_exact(canvas, mark, static_cast<uint32_t>(x1), static_cast<uint32_t>(y1), w, h, true, ResampleHints{});
        return canvas;
    }

    // one node: `in` is the frame of its input edge (null for source nodes), `canvas` the frame of its canvas edge
    FramePtr run_node(const std::string& name, const JVal& p, FramePtr in, FramePtr canvas, bool in_shared) {
        auto need_input = [&] { if (!in) raise(kGraphInvalid, "GraphInvalid: node '%s' has no input frame", name.c_str()); };
        auto need_canvas = [&] { if (!canvas) raise(kGraphInvalid, "InvalidNodeConnections: node '%s' needs a canvas edge", name.c_str()); };
        poll_cancel();                                                                // execution_engine.rs:502
        if (name == "draw_image_exact") {                                             // s::Node::DrawImageExact (lib.rs:1328-1336)
            need_input(); need_canvas();
            const JVal* blend = p.get("blend");
            bool compose = true;
            if (blend && blend->t == JVal::Str) { if (blend->s == "overwrite") compose = false; else if (blend->s != "compose") raise(kInvalidJson, "InvalidJson: blend is compose or overwrite"); }
            draw_image_exact(canvas, in, want_u32(p, "x", "draw_image_exact"), want_u32(p, "y", "draw_image_exact"), want_u32(p, "w", "draw_image_exact"),
                             want_u32(p, "h", "draw_image_exact"), compose, parse_hints(p.get("hints"), "draw_image_exact"));
            return canvas;
        }
        if (name == "copy_rect_to_canvas") {
            need_input(); need_canvas();
            Timed t(this, "copy_rect_to_canvas");
            return copy_into_canvas(in, canvas, want_u32(p, "from_x", name.c_str()), want_u32(p, "from_y", name.c_str()), want_u32(p, "w", name.c_str()),
                                    want_u32(p, "h", name.c_str()), want_u32(p, "x", name.c_str()), want_u32(p, "y", name.c_str()));
        }
        if (canvas) raise(kGraphInvalid, "InvalidNodeConnections: node '%s' does not take a canvas edge", name.c_str());
        if (name == "decode") {
            uint32_t hw = 0, hh = 0;
            bool spatial = false, gamma = false;
            const int32_t io_id = static_cast<int32_t>(want_int(p, "io_id", "decode"));
            Io& src = input(io_id);
            if (src.told) { hw = src.told_w; hh = src.told_h; spatial = src.told_spatial; gamma = src.told_gamma; }
            if (const JVal* cmds = p.get("commands")) {
                if (cmds->t == JVal::Arr) {
                    for (const JVal& cmd : cmds->a) {
                        if (cmd.t == JVal::Str && cmd.s == "discard_color_profile") {
                            src.told_discard_profile = true;
                        } else if (cmd.t == JVal::Str && cmd.s == "ignore_color_profile_errors") {
                            src.told_ignore_profile_errors = true;
                        } else if (cmd.t == JVal::Str && cmd.s == "convert_color_profile") {  // EXTENSION: colour management for this input
                            src.told_convert_profile = true;
                        } else if (const JVal* j = cmd.get("select_frame")) {                // s::DecoderCommand::SelectFrame(i32): a GIF input acts on it
                            tell_select_frame(src, *j);
                        } else if (const JVal* j = cmd.get("webp_decoder_hints")) {          // s::WebPDecoderHints {width, height}
                            tell_webp_hint(src, *j);
                        } else if (const JVal* j = cmd.get("jpeg_downscale_hints")) {        // s::JpegIDCTDownscaleHints
                            hw = want_u32(*j, "width", "jpeg_downscale_hints"); hh = want_u32(*j, "height", "jpeg_downscale_hints");
                            if (const JVal* b = j->get("scale_luma_spatially")) spatial = b->t == JVal::Bool && b->b;
                            if (const JVal* b = j->get("gamma_correct_for_srgb_during_spatial_luma_scaling")) gamma = b->t == JVal::Bool && b->b;
                        }
                    }
                }
            }
            anim.in_decode_node = true;                                              // (a watermark's or a command_string's own decode does not animate)
            FramePtr f = decode_oriented(io_id, hw, hh, spatial, gamma);
            anim.in_decode_node = false;
            return f;
        }
        if (name == "create_canvas") {
            Timed t(this, "create_canvas");
            const JVal* fmt = p.get("format");
            const std::string f = fmt && fmt->t == JVal::Str ? fmt->s : "bgra_32";
            if (f != "bgra_32" && f != "bgr_32") raise(kActionNotSupported, "ActionNotSupported: create_canvas format %s", f.c_str());
            return new_frame(want_u32(p, "w", "create_canvas"), want_u32(p, "h", "create_canvas"), f == "bgra_32", parse_color(p.get("color"), "create_canvas.color"), true,
                             !keyword_transparent(p.get("color")));
        }
        if (name == "command_string") return command_string(p, in, in_shared);
        need_input();
        if (name == "resample_2d") return resample(in, want_u32(p, "w", "resample_2d"), want_u32(p, "h", "resample_2d"), p.get("hints"));
        if (name == "constrain") return constrain(in, p);
        if (name == "watermark") return watermark(in, p);
        if (name == "encode") { encode(in, static_cast<int32_t>(want_int(p, "io_id", "encode")), p.get("preset"), in_shared); return in; }
        if (name == "round_image_corners") {                                          // s::Node::RoundImageCorners {radius, background_color}
            const JVal* r = p.get("radius");
            const JVal* bg = p.get("background_color");
            if (!bg || bg->is_null()) raise(kInvalidJson, "InvalidJson: round_image_corners.background_color is required");
            float radii[4] = {0, 0, 0, 0};
            int mode = -1;
            auto num = [&](const JVal* v, const char* what) -> float {
                if (!v || v->t != JVal::Num) raise(kInvalidJson, "InvalidJson: round_image_corners.radius.%s is a number", what);
                return static_cast<float>(v->n);
            };
            if (r && r->t == JVal::Str && r->s == "circle") mode = IFHIP_ROUND_CORNERS_CIRCLE;
            else if (r && r->t == JVal::Obj && r->o.size() == 1) {                     // RoundCornersMode (lib.rs:1254-1268)
                const std::string& key = r->o[0].first;
                const JVal& v = r->o[0].second;
                if (key == "percentage" || key == "pixels") {
                    mode = key == "percentage" ? IFHIP_ROUND_CORNERS_PERCENTAGE : IFHIP_ROUND_CORNERS_PIXELS;
                    radii[0] = radii[1] = radii[2] = radii[3] = num(&v, key.c_str());
                } else if (key == "percentage_custom" || key == "pixels_custom") {
                    mode = key == "percentage_custom" ? IFHIP_ROUND_CORNERS_PERCENTAGE_CUSTOM : IFHIP_ROUND_CORNERS_PIXELS_CUSTOM;
                    radii[0] = num(v.get("top_left"), "top_left"); radii[1] = num(v.get("top_right"), "top_right");
                    radii[2] = num(v.get("bottom_right"), "bottom_right"); radii[3] = num(v.get("bottom_left"), "bottom_left");
                }
            }
            if (mode < 0) raise(kInvalidJson, "InvalidJson: round_image_corners.radius is {percentage|pixels: n}, \"circle\" or {percentage_custom|pixels_custom: {top_left, top_right, bottom_right, bottom_left}}");
            return round_corners(in, mode, radii, parse_color(bg, "round_image_corners.background_color"));
        }
        if (name == "white_balance_histogram_area_threshold_srgb") {                  // s::Node::WhiteBalanceHistogramAreaThresholdSrgb {threshold: Option<f32>}
            const JVal* th = p.get("threshold");
            if (th && !th->is_null() && th->t != JVal::Num) raise(kInvalidJson, "InvalidJson: white_balance_histogram_area_threshold_srgb.threshold is a number or null");
            return white_balance(in, th && th->t == JVal::Num ? static_cast<float>(th->n) : 0.006f);
        }
        if (name == "watermark_red_dot") {                                            // flow/nodes/watermark_red_dot.rs:26-40: FillRect over the last 3x3 pixels
            if (!(in->w > 3 && in->h > 3)) return in;
            char text[160];
            std::snprintf(text, sizeof text, "{\"x1\":%u,\"y1\":%u,\"x2\":%u,\"y2\":%u,\"color\":{\"srgb\":{\"hex\":\"FF0000\"}}}", in->w - 3, in->h - 3, in->w, in->h);
            return run_node("fill_rect", parse_json(reinterpret_cast<const uint8_t*>(text), std::strlen(text)), in, nullptr, in_shared);
        }
        if (name == "crop_whitespace") {                                              // s::Node::CropWhitespace {threshold: u32, percent_padding: f32}
            const int64_t thr = want_int(p, "threshold", "crop_whitespace");
            if (thr < 0 || thr > 0xFFFFFFFFll) raise(kInvalidJson, "InvalidJson: crop_whitespace.threshold out of range");
            const JVal* pp = p.get("percent_padding");
            if (!pp || pp->t != JVal::Num) raise(kInvalidJson, "InvalidJson: crop_whitespace.percent_padding is a number");
            return crop_whitespace(in, static_cast<uint32_t>(thr), static_cast<float>(pp->n), in_shared);
        }
        Timed t(this, name == "fill_rect" ? "fill_rect_mutate" : name == "crop" ? "crop_mutate" : name == "flip_v" ? "flip_vertical_mutate" : name == "flip_h" ? "flip_vertical_mutate" /* sic: rotate_flip_transpose.rs:206 */
                      : name == "color_matrix_srgb" || name == "color_filter_srgb" ? "color_matrix_srgb_mut" : name == "expand_canvas" || name == "region" || name == "region_percent" ? "expand_canvas" : name == "transpose" ? "transpose_mut"
                      : name == "rotate_90" ? "rotate_90" : name == "rotate_180" ? "rotate_180" : name == "rotate_270" ? "rotate_270" : name == "apply_orientation" ? "apply_orientation" : "node");
        if (name == "fill_rect") {                                                    // clone_crop_fill_expand.rs:107-137
            in->compose = IFHIP_BLEND_WITH_SELF;                                      // :112: set before the fill, so matte canvases accept sub-rects
            {   // the node's own check (:114-127): an empty rectangle is an error HERE (fill_rectangle itself lets one pass)
                const uint32_t x1 = want_u32(p, "x1", name.c_str()), y1 = want_u32(p, "y1", name.c_str()), x2 = want_u32(p, "x2", name.c_str()), y2 = want_u32(p, "y2", name.c_str());
                if (x2 <= x1 || y2 <= y1 || static_cast<int32_t>(x1) < 0 || static_cast<int32_t>(y1) < 0 || x2 > in->w || y2 > in->h)
                    raise(kArgumentInvalid, "InvalidCoordinates: Invalid coordinates for %ux%u bitmap: fill_rect x1=%u y1=%u x2=%u y2=%u", in->w, in->h, x1, y1, x2, y2);
            }
            check(ifhip_fill_rect_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, in->compose, want_u32(p, "x1", name.c_str()),
                                               want_u32(p, "y1", name.c_str()), want_u32(p, "x2", name.c_str()), want_u32(p, "y2", name.c_str()),
                                               parse_color(p.get("color"), "fill_rect.color"), t_job_stream));
            return in;
        }
        if (name == "expand_canvas") {                                                // :224-262
            const uint32_t l = want_u32(p, "left", "expand_canvas"), t2 = want_u32(p, "top", "expand_canvas"), r = want_u32(p, "right", "expand_canvas"),
                           b = want_u32(p, "bottom", "expand_canvas"), color = parse_color(p.get("color"), "expand_canvas.color");
            return expand_frame(in, l, t2, r, b, color, keyword_transparent(p.get("color")));
        }
        if (name == "crop") {                                                         // :519-541 (materialised: a copy)
            const uint32_t x1 = want_u32(p, "x1", "crop"), y1 = want_u32(p, "y1", "crop"), x2 = want_u32(p, "x2", "crop"), y2 = want_u32(p, "y2", "crop");
            FramePtr cv = crop_frame(in, x1, y1, x2, y2);
            if (in_shared) { cv->compose = IFHIP_BLEND_WITH_SELF; cv->matte = 0; }    // CROP is MutProtect (clone_crop_fill_expand.rs:6): a window onto the Clone
            return cv;
        }
        if (name == "region" || name == "region_percent") {                            // :263-452
            // RegionPercent rewrites itself into Region with pixel corners (get_coords :265-286: f32 arithmetic, round half
            // away from zero, a side the percentages collapse gets one pixel), Region into Crop + ExpandCanvas -- or into a
            // plain CreateCanvas of the parent's format when the rectangle misses the frame altogether (:409-421)
            int64_t x1, y1, x2, y2;
            const uint32_t color = parse_color(p.get("background_color"), "region.background_color");
            if (name == "region_percent") {
                auto pct = [&](const char* k) -> float {
                    const JVal* v = p.get(k);
                    if (!v || v->t != JVal::Num) raise(kInvalidJson, "InvalidJson: region_percent.%s is a number", k);
                    return static_cast<float>(v->n);
                };
                const float l = pct("x1"), t2 = pct("y1"), r = pct("x2"), b = pct("y2");
                if (b <= t2 || r <= l) raise(kArgumentInvalid, "InvalidNodeParams: Invalid coordinates: %g,%g %g,%g should describe the top-left and bottom-right corners of the region in percentages. Not a rectangle.", l, t2, r, b);
                auto px = [](uint32_t side, float pc) -> int64_t {                    // `(side as f32 * pc / 100f32).round() as i32` (saturating)
                    const float v = std::round(static_cast<float>(side) * pc / 100.0f);
                    return v != v ? 0 : v >= 2147483648.0f ? INT32_MAX : v <= -2147483648.0f ? INT32_MIN : static_cast<int64_t>(v);
                };
                x1 = px(in->w, l); y1 = px(in->h, t2); x2 = px(in->w, r); y2 = px(in->h, b);
                if (x2 < x1) x2 = x1 + 1;                                             // sic: `<`, equal corners fall through to Region's own check
                if (y2 < y1) y2 = y1 + 1;
            } else {
                auto i32 = [&](const char* k) -> int64_t {
                    const int64_t v = want_int(p, k, "region");
                    if (v < INT32_MIN || v > INT32_MAX) raise(kInvalidJson, "InvalidJson: region.%s is a 32-bit integer", k);
                    return v;
                };
                x1 = i32("x1"); y1 = i32("y1"); x2 = i32("x2"); y2 = i32("y2");
            }
            if (y2 <= y1 || x2 <= x1) raise(kArgumentInvalid, "InvalidNodeParams: Invalid coordinates: %lld,%lld %lld,%lld should describe the top-left and bottom-right corners of the region in pixels. Not a rectangle.",
                                            static_cast<long long>(x1), static_cast<long long>(y1), static_cast<long long>(x2), static_cast<long long>(y2));
            const int64_t iw = in->w, ih = in->h;
            check_size(sec.max_frame_size, "max_frame_size", static_cast<uint64_t>(x2 - x1), static_cast<uint64_t>(y2 - y1));
            if (x1 >= iw || y1 >= ih || x2 <= 0 || y2 <= 0)                           // nothing of the input inside: a canvas of the colour
                return new_frame(static_cast<uint32_t>(x2 - x1), static_cast<uint32_t>(y2 - y1), in->alpha, color, true, !keyword_transparent(p.get("background_color")));
            const uint32_t cx1 = static_cast<uint32_t>(std::min(iw, std::max<int64_t>(0, x1))), cy1 = static_cast<uint32_t>(std::min(ih, std::max<int64_t>(0, y1)));
            const uint32_t cx2 = static_cast<uint32_t>(std::min(iw, std::max<int64_t>(0, x2))), cy2 = static_cast<uint32_t>(std::min(ih, std::max<int64_t>(0, y2)));
            const uint32_t el = static_cast<uint32_t>(std::max<int64_t>(0, -x1)), et = static_cast<uint32_t>(std::max<int64_t>(0, -y1));
            const uint32_t er = static_cast<uint32_t>(std::max<int64_t>(0, x2 - iw)), eb = static_cast<uint32_t>(std::max<int64_t>(0, y2 - ih));
            FramePtr part = in;
            if (in_shared || cx1 != 0 || cy1 != 0 || cx2 != in->w || cy2 != in->h) {  // Crop (a full-frame crop is the frame -- unless the frame has other readers: CROP is MutProtect, and copy_rectangle below normalises its input's unused alpha in place)
                part = new_frame(cx2 - cx1, cy2 - cy1, in->alpha, 0, true);
                copy_into_canvas(in, part, cx1, cy1, cx2 - cx1, cy2 - cy1, 0, 0);
            }
            // ExpandCanvas, also by nothing: CreateCanvas of the colour + CopyRectToCanvas (:231-255)
            FramePtr cv = new_frame(part->w + el + er, part->h + et + eb, (color >> 24) == 255 ? part->alpha : true, color, true, !keyword_transparent(p.get("background_color")));
            return copy_into_canvas(part, cv, 0, 0, part->w, part->h, el, et);
        }
        if (name == "color_matrix_srgb") {                                            // s::Node::ColorMatrixSrgb {matrix: [[f32;5];5]}
            const JVal* mj = p.get("matrix");
            float m[25];
            if (!mj || mj->t != JVal::Arr || mj->a.size() != 5) raise(kInvalidJson, "InvalidJson: color_matrix_srgb.matrix is 5 rows of 5 numbers");
            for (int r = 0; r < 5; ++r) {
                const JVal& row = mj->a[static_cast<size_t>(r)];
                if (row.t != JVal::Arr || row.a.size() != 5) raise(kInvalidJson, "InvalidJson: color_matrix_srgb.matrix is 5 rows of 5 numbers");
                for (int k = 0; k < 5; ++k) { if (row.a[static_cast<size_t>(k)].t != JVal::Num) raise(kInvalidJson, "InvalidJson: color_matrix_srgb.matrix is 5 rows of 5 numbers"); m[r * 5 + k] = static_cast<float>(row.a[static_cast<size_t>(k)].n); }
            }
            return color_matrix(in, m);
        }
        if (name == "color_filter_srgb") return color_filter(in, p);
        if (name == "flip_v") return flip(in, true);
        if (name == "flip_h") return flip(in, false);
        if (name == "transpose") return transposed(in);
        if (name == "rotate_90") return flip(transposed(in), false);                  // rotate_flip_transpose.rs:51-66
        if (name == "rotate_180") return flip(flip(in, true), false);
        if (name == "rotate_270") return flip(transposed(in), true);
        if (name == "apply_orientation") return apply_orientation(in, want_int(p, "flag", "apply_orientation"));
        raise(kActionNotSupported, "ActionNotSupported: node '%s' is outside the pixel hot path this library replaces", name.c_str());
    }

    static void node_of(const JVal& n, std::string* name, const JVal** params) {
        if (n.t == JVal::Str) { *name = n.s; static const JVal kNull; *params = &kNull; return; }
        if (n.t != JVal::Obj || n.o.size() != 1) raise(kInvalidJson, "InvalidJson: a node is {\"name\": {params}}");
        *name = n.o[0].first;
        *params = &n.o[0].second;
    }
    static bool mutates_input(const std::string& nm) {
        return nm == "fill_rect" || nm == "watermark_red_dot" || nm == "flip_v" || nm == "flip_h" || nm == "rotate_180" || nm == "color_matrix_srgb" || nm == "color_filter_srgb" ||
               nm == "apply_orientation" || nm == "watermark" || nm == "round_image_corners" || nm == "white_balance_histogram_area_threshold_srgb";
    }

    // EncoderPreset::Mozjpeg's quality is an Option<u8>: the reference refuses the message when it is deserialised, before any
    // node runs -- so every encode node's mozjpeg preset is looked at before the first node runs, and again where it is used
    static void check_mozjpeg_preset(const JVal* preset) {
        const JVal* moz = preset ? preset->get("mozjpeg") : nullptr;
        const JVal* q = moz ? moz->get("quality") : nullptr;
        if (q && q->t == JVal::Num && (q->n != std::floor(q->n) || q->n < 0.0 || q->n > 255.0))
            raise(kInvalidJson, "InvalidJson: encode.preset.mozjpeg.quality is an integer 0..255");
    }
    // EncoderPreset::WebPLossy is a struct variant with a required f32: the bare string, a missing or a non-numeric quality do
    // not deserialise.  Looked at only where the context's lossy WebP encoder is on; -> the quality.
    static bool names_webplossy(const JVal* preset) {
        return preset && ((preset->t == JVal::Str && preset->s == "webplossy") || (preset->t == JVal::Obj && preset->get("webplossy")));
    }
    static float check_webplossy_preset(const JVal* preset) {
        const JVal* lossy = preset->t == JVal::Obj ? preset->get("webplossy") : nullptr;
        const JVal* q = lossy && lossy->t == JVal::Obj ? lossy->get("quality") : nullptr;
        if (!q || q->t != JVal::Num) raise(kInvalidJson, "InvalidJson: encode.preset.webplossy.quality is a number");
        return static_cast<float>(q->n);
    }
    void check_encode_node(const JVal& n) {
        if (n.t != JVal::Obj || n.o.size() != 1 || n.o[0].first != "encode") return;
        const JVal* preset = n.o[0].second.get("preset");
        if (encode_coder(preset) == IFHIP_ENCODE_CODER_MOZJPEG) check_mozjpeg_preset(preset);
        if (names_webplossy(preset) && c->webp_lossy_encoder.load(std::memory_order_relaxed)) (void)check_webplossy_preset(preset);
    }


    // ---- animated GIFs (EXTENSION ifhip_shim_context_set_gif_animation) ---------------------------------------------------------------
    // The reference re-runs the job for every frame of an animated source (GifDecoder::has_more_frames -> ctx.set_more_frames,
    // codecs/gif/mod.rs:207-305, flow/nodes/codecs_and_pointer.rs:168) and GifEncoder::write_frame appends frame frame_ix to one
    // file (:429-521).  Here: the source's screens are decoded ONCE (ifhip::gif_decode_all_parsed_device: one replay for all of
    // them), run_framewise runs once per frame with the animated decode node yielding screen k, every "gif" encode node
    // collects its frame k into one device block, and behind the last frame the block is coded in ONE call
    // (ifhip_gif_encode_animation_device) -- an animation's frames are a ready-made batch.  Every other encoder takes frame 0.
    struct AnimSource {
        uint8_t* d = nullptr;                    // n screens, h * stride bytes each
        uint32_t w = 0, h = 0, stride = 0;
        ~AnimSource() { job_free(d); }
    };
    struct AnimCollect {
        uint8_t* d = nullptr;                    // n frames, h * stride bytes each
        ifhip_gif_enc_stage* stage = nullptr;
        uint32_t w = 0, h = 0, stride = 0;
        bool alpha = false;
        ~AnimCollect() { job_free(d); if (stage) { quiesce(); ifhip_gif_enc_stage_destroy(stage); } }
    };
    struct Anim {
        bool active = false, in_decode_node = false;
        uint32_t n = 0, k = 0;
        int repeat = 0;
        uint64_t pixels = 0;                     // decoded screens + collected frames so far (check_total_pixels)
        std::vector<uint32_t> delays;
        std::vector<uint8_t> user_input;
        std::map<int32_t, std::unique_ptr<AnimSource>> sources;
        std::map<int32_t, std::unique_ptr<AnimCollect>> collects;
    } anim;

    void add_animation_pixels(uint64_t pixels_per_frame) {
        anim.pixels += pixels_per_frame * anim.n;
        if (sec.has_max_total_file_pixels && anim.pixels > sec.max_total_file_pixels)
            raise(kArgumentInvalid, "SizeLimitExceeded: GIF total decoded pixels (%u frames x %llu pixels, %llu in the job) exceeds max_total_file_pixels %llu", anim.n,
                  static_cast<unsigned long long>(pixels_per_frame), static_cast<unsigned long long>(anim.pixels), static_cast<unsigned long long>(sec.max_total_file_pixels));
    }
    // a `decode` node whose input animates: a GIF of more than one frame that no select_frame was told to (-> its frame count)
    uint32_t animated_frames_of(const JVal& params) {
        const JVal* id = params.get("io_id");
        if (!id || id->t != JVal::Num) return 0;
        auto it = c->io.find(static_cast<int32_t>(id->n));
        if (it == c->io.end() || it->second.is_output || !is_gif(it->second) || it->second.told_frame) return 0;
        if (const JVal* cmds = params.get("commands"))
            if (cmds->t == JVal::Arr)
                for (const JVal& cmd : cmds->a) if (cmd.t == JVal::Obj && cmd.get("select_frame")) return 0;
        uint32_t n = 0;
        if (ifhip_gif_frame_count(it->second.in, it->second.in_len, &n, nullptr, nullptr, 0) != IFHIP_OK) return 0;   // (a file the walk refuses is the one-frame path's to report)
        return n > 1u ? n : 0u;
    }
    // The animated decodes of a job that have a "gif" encode node downstream: io_id -> frame count; empty: the job does not animate.
    std::vector<std::pair<int32_t, uint32_t>> animation_plan(const JVal& fw) {
        std::vector<std::pair<int32_t, uint32_t>> found;
        auto is_gif_encode = [](const std::string& name, const JVal& p) {
            const JVal* preset = p.get("preset");
            return name == "encode" && preset && preset->t == JVal::Str && preset->s == "gif";
        };
        auto add = [&](const JVal& p, uint32_t n) {
            const int32_t id = static_cast<int32_t>(p.get("io_id")->n);
            for (const auto& f : found) if (f.first == id) return;
            found.push_back({id, n});
        };
        std::string name;
        const JVal* params;
        if (const JVal* steps = fw.get("steps")) {
            if (steps->t != JVal::Arr) return found;
            for (size_t i = 0; i < steps->a.size(); ++i) {
                node_of(steps->a[i], &name, &params);
                if (name != "decode") continue;
                const uint32_t n = animated_frames_of(*params);
                if (!n) continue;
                const JVal* source = params;
                for (size_t j = i + 1; j < steps->a.size(); ++j) {                       // downstream: up to the next node that starts a frame of its own
                    node_of(steps->a[j], &name, &params);
                    if (name == "decode" || name == "create_canvas") break;
                    if (is_gif_encode(name, *params)) { add(*source, n); break; }
                }
            }
            return found;
        }
        const JVal* graph = fw.get("graph");
        const JVal *nodes = graph ? graph->get("nodes") : nullptr, *edges = graph ? graph->get("edges") : nullptr;
        if (!nodes || nodes->t != JVal::Obj || !edges || edges->t != JVal::Arr) return found;
        std::map<int64_t, const JVal*> by_id;
        std::multimap<int64_t, int64_t> parents;
        for (const auto& kv : nodes->o) by_id[std::atoll(kv.first.c_str())] = &kv.second;
        for (const JVal& e : edges->a) {
            const JVal *from = e.get("from"), *to = e.get("to");
            if (from && to && from->t == JVal::Num && to->t == JVal::Num) parents.insert({static_cast<int64_t>(to->n), static_cast<int64_t>(from->n)});
        }
        for (const auto& kv : by_id) {
            node_of(*kv.second, &name, &params);
            if (!is_gif_encode(name, *params)) continue;
            std::vector<int64_t> todo{kv.first};
            std::map<int64_t, bool> seen;
            while (!todo.empty()) {                                                      // every ancestor, over input and canvas edges
                const int64_t id = todo.back();
                todo.pop_back();
                if (seen[id] || !by_id.count(id)) continue;
                seen[id] = true;
                node_of(*by_id[id], &name, &params);
                if (name == "decode") if (const uint32_t n = animated_frames_of(*params)) add(*params, n);
                auto range = parents.equal_range(id);
                for (auto it = range.first; it != range.second; ++it) todo.push_back(it->second);
            }
        }
        return found;
    }
    // every screen of one animated source, decoded and composed once
    void decode_animation_source(int32_t io_id, bool first) {
        Timed t(this, "primitive_decoder");
        Io& in = input(io_id);
        ifhip::GifParsed P;
        check(ifhip::parse_gif_header(in.in, in.in_len, &P));
        check_size(sec.max_decode_size, "max_decode_size", P.w, P.h);
        check_size(sec.max_frame_size, "max_frame_size", P.w, P.h);
        check(ifhip::parse_gif_all(in.in, in.in_len, &P));
        auto refuse = [&](uint32_t status) {
            if (status == IFHIP_GIF_DEC_FRAME_TOO_LARGE) raise(kArgumentInvalid, "SizeLimitExceeded: %s (io_id %d)", ifhip::gif_status_text(status), io_id);
            raise(kImageMalformed, "ImageMalformed: GIF decoding error: %s (io_id %d, status %u)", ifhip::gif_status_text(status), io_id, status);
        };
        if (P.status) refuse(P.status);
        add_animation_pixels(static_cast<uint64_t>(P.w) * P.h);                        // before anything is allocated
        auto src = std::make_unique<AnimSource>();
        src->w = P.w; src->h = P.h; src->stride = ifhip_stride_for_width(P.w);
        const size_t pitch = static_cast<size_t>(P.h) * src->stride;
        hip_check(job_malloc(reinterpret_cast<void**>(&src->d), pitch * anim.n + 64), "hipMalloc(screens)");
        hip_check(hipMemsetAsync(src->d, 0, pitch * anim.n + 64, t_job_stream), "hipMemset(screens)");
        const uint32_t status = decoded_status("decode(gif)", [&](uint32_t* d_status) { return ifhip::gif_decode_all_parsed_device(P, src->d, pitch, src->stride, d_status, t_job_stream); });
        if (status) refuse(status);
        if (first) {                                                                    // frame k's delay and user-input flag are the source frame's
            anim.repeat = P.repeat < 0 ? 0 : P.repeat;                                  // (no NETSCAPE2.0 block: get_repeat's Infinite, mod.rs:167-170)
            for (const ifhip::GifFrameInfo& f : P.frames) { anim.delays.push_back(f.delay); anim.user_input.push_back(f.user_input ? 1u : 0u); }
        }
        anim.sources[io_id] = std::move(src);
    }
    // what the animated decode node hands on in run k: a frame of its own (nodes may write into it) holding screen k
    FramePtr animated_screen(int32_t io_id) {
        const AnimSource& src = *anim.sources[io_id];
        FramePtr f = new_frame(src.w, src.h, true, 0, false);
        hip_check(hipMemcpyAsync(f->d, src.d + static_cast<size_t>(anim.k) * f->bytes(), f->bytes(), hipMemcpyDeviceToDevice, t_job_stream), "copy(screen)");
        decodes.push_back({io_id, src.w, src.h, "image/gif", "gif"});
        return f;
    }
    // a "gif" encode node in run k: its input joins the node's block
    void collect_frame(const FramePtr& f, int32_t io_id) {
        std::unique_ptr<AnimCollect>& slot = anim.collects[io_id];
        if (anim.k == 0) {
            if (slot) raise(kArgumentInvalid, "InvalidArgument: io_id %d is written by two encode nodes", io_id);
            slot = std::make_unique<AnimCollect>();
            check(ifhip_gif_enc_stage_create(&slot->stage, f->w, f->h, std::min(anim.n, 32u)));   // (size_16(): a side above 65535 is refused here)
            add_animation_pixels(static_cast<uint64_t>(f->w) * f->h);                  // before the block is allocated
            slot->w = f->w; slot->h = f->h; slot->stride = f->stride; slot->alpha = f->alpha;
            hip_check(job_malloc(reinterpret_cast<void**>(&slot->d), f->bytes() * anim.n + 64), "hipMalloc(collected frames)");
            encodes.push_back({io_id, f->w, f->h, "image/gif", "gif"});
        }
        if (!slot || slot->w != f->w || slot->h != f->h || slot->stride != f->stride || slot->alpha != f->alpha)
            raise(kArgumentInvalid, "InvalidArgument: frame %u reaches the GIF encoder of io_id %d as %ux%u, frame 0 was %ux%u", anim.k, io_id, f->w, f->h, slot ? slot->w : 0u,
                  slot ? slot->h : 0u);
        hip_check(hipMemcpyAsync(slot->d + static_cast<size_t>(anim.k) * f->bytes(), dev(f), f->bytes(), hipMemcpyDeviceToDevice, t_job_stream), "copy(collected frame)");
    }
    void write_animations() {
        for (auto& kv : anim.collects) {
            Timed t(this, "primitive_encoder");
            AnimCollect& a = *kv.second;
            Io& o = output(kv.first);
            size_t capacity = 0;
            check(ifhip_gif_enc_stage_max_animation_bytes(a.stage, anim.n, &capacity));
            const size_t pitch = (capacity + 15u) & ~static_cast<size_t>(15u);
            const size_t image_bytes = static_cast<size_t>(a.h) * a.stride;
            fetch_coded_file(o, pitch, kGifNames, 0u, [&](CodedFile& file) {
                return ifhip_gif_encode_animation_device(a.stage, a.d, image_bytes, a.stride, a.alpha ? 1 : 0, anim.n, anim.repeat, anim.delays.data(), anim.user_input.data(), file.d,
                                                         capacity, file.d_len, file.d_len + 1, t_job_stream);
            });
        }
    }
    // a job: once, or -- where the animation path applies -- once per frame of the animated sources
    void run_job(const JVal& fw) {
        if (!c->gif_animation.load(std::memory_order_relaxed) || !c->gif_encoder.load(std::memory_order_relaxed)) return run_framewise(fw);
        const std::vector<std::pair<int32_t, uint32_t>> plan = animation_plan(fw);
        if (plan.empty()) return run_framewise(fw);
        for (const auto& p : plan)                                                       // (mod.rs:253-258: a decoder that has run out of frames while the job goes on)
            if (p.second != plan[0].second)
                raise(kInternalError, "InvalidOperation: read_frame was called without a frame available (io_id %d has %u frames, io_id %d has %u)", p.first, p.second,
                      plan[0].first, plan[0].second);
        anim.active = true;
        anim.n = plan[0].second;
        for (size_t i = 0; i < plan.size(); ++i) decode_animation_source(plan[i].first, i == 0);
        size_t decoded = 0;
        for (anim.k = 0; anim.k < anim.n; ++anim.k) {
            poll_cancel();                                                               // between frames
            run_framewise(fw);
            if (anim.k == 0) decoded = decodes.size();
            else decodes.erase(decodes.begin() + static_cast<std::ptrdiff_t>(decoded), decodes.end());   // one record per decode node, as a one-frame job has
        }
        write_animations();
    }

    void run_framewise(const JVal& fw) {
        if (const JVal* steps = fw.get("steps")) {
            if (steps->t != JVal::Arr) raise(kInvalidJson, "InvalidJson: framewise.steps must be an array");
            for (const JVal& n : steps->a) check_encode_node(n);
            FramePtr cur;
            for (const JVal& n : steps->a) {
                std::string name;
                const JVal* params;
                node_of(n, &name, &params);
                lazy_decode = true;                                                    // a chain: every frame has one consumer
                cur = run_node(name, *params, cur, nullptr, false);
            }
            return;
        }
        const JVal* graph = fw.get("graph");
        if (!graph) raise(kInvalidJson, "InvalidJson: framewise needs steps or graph");
        const JVal *nodes = graph->get("nodes"), *edges = graph->get("edges");
        if (!nodes || nodes->t != JVal::Obj || !edges || edges->t != JVal::Arr) raise(kInvalidJson, "InvalidJson: graph needs nodes{} and edges[]");
        std::map<int64_t, const JVal*> node_by_id;
        std::map<int64_t, int64_t> parent, canvas_parent;                              // EdgeKind::Input / EdgeKind::Canvas
        for (const auto& kv : nodes->o) node_by_id[std::atoll(kv.first.c_str())] = &kv.second;
        for (const JVal& e : edges->a) {
            const int64_t from = want_int(e, "from", "edge"), to = want_int(e, "to", "edge");
            const JVal* kind = e.get("kind");
            const bool is_canvas = kind && kind->t == JVal::Str && kind->s == "canvas";
            if (!kind || kind->t != JVal::Str || (kind->s != "input" && !is_canvas)) raise(kInvalidJson, "InvalidJson: edge kind is input or canvas");
            if (!node_by_id.count(from) || !node_by_id.count(to)) raise(kGraphInvalid, "GraphInvalid: edge names a missing node");
            auto& slot = is_canvas ? canvas_parent : parent;
            if (slot.count(to)) raise(kGraphInvalid, "GraphInvalid: node %lld has two %s edges", static_cast<long long>(to), is_canvas ? "canvas" : "input");
            slot[to] = from;
        }
        for (const auto& kv : nodes->o) check_encode_node(kv.second);
        std::map<int64_t, FramePtr> done;
        std::map<int64_t, int> state;                                                  // 1 = on the stack (cycle check)
        // nodes that mutate a parent's frame in place (their input, or the canvas they draw on) must not see a frame
        // another consumer still needs: every such node with a shared parent works on its own copy
        std::map<int64_t, int> consumers;
        for (const auto& kv : parent) ++consumers[kv.second];
        for (const auto& kv : canvas_parent) ++consumers[kv.second];
        // "shared" is a property of the FRAME, not of the edge: a node that disappears (a resample_2d that has nothing to do, a
        // watermark on too small a canvas: delete_node_and_snap_together) hands its input on, and its consumer then reads a
        // frame the disappeared node's siblings still need
        std::map<const Frame*, bool> frame_shared;
        std::function<FramePtr(int64_t)> eval = [&](int64_t id) -> FramePtr {
            auto it = done.find(id);
            if (it != done.end()) return it->second;
            if (state[id] == 1) raise(kGraphInvalid, "GraphInvalid: cycle through node %lld", static_cast<long long>(id));
            state[id] = 1;
            std::string name;
            const JVal* params;
            node_of(*node_by_id[id], &name, &params);
            FramePtr in, canvas;
            bool in_shared = false;
            auto pit = parent.find(id);
            if (pit != parent.end()) {
                in = eval(pit->second);
                in_shared = in && frame_shared[in.get()];
                if (in && in_shared && mutates_input(name)) { in = clone(in, true); in_shared = false; }
            }
            auto cit = canvas_parent.find(id);
            if (cit != canvas_parent.end()) {
                canvas = eval(cit->second);
                if (canvas && frame_shared[canvas.get()]) canvas = clone(canvas);
            }
            const FramePtr given = in;
            lazy_decode = consumers[id] == 1;
            FramePtr out = run_node(name, *params, in, canvas, in_shared);
            if (out) frame_shared[out.get()] = consumers[id] > 1 || (out == given && in_shared);
            state[id] = 2;
            done[id] = out;
            return out;
        };
        for (const auto& kv : node_by_id) eval(kv.first);
    }
};

// Build001.io (imageflow_types/src/lib.rs:1433-1456, 1577-1581): placeholder / output_buffer need the buffers registered
// through the ABI; bytes_hex and base_64 carry the bytes inline.
void add_io_from_json(imageflow_context* c, const JVal& ios) {
    if (ios.t != JVal::Arr) raise(kInvalidJson, "InvalidJson: io must be an array");
    for (const JVal& o : ios.a) {
        const int32_t id = static_cast<int32_t>(want_int(o, "io_id", "io"));
        const JVal* dir = o.get("direction");
        const JVal* io = o.get("io");
        if (!dir || dir->t != JVal::Str || !io) raise(kInvalidJson, "InvalidJson: io entries need direction and io");
        const bool out = dir->s == "out";
        if (io->t == JVal::Str && io->s == "placeholder") {
            if (!c->io.count(id)) raise(kArgumentInvalid, "InvalidArgument: io_id %d is a placeholder but no buffer was added for it", id);
            continue;
        }
        if (c->io.count(id)) raise(kArgumentInvalid, "InvalidArgument: io_id %d is already in use", id);
        Io e;
        e.is_output = out;
        if (io->t == JVal::Str && (io->s == "output_buffer" || io->s == "output_base_64")) {
            if (!out) raise(kInvalidJson, "InvalidJson: %s on an input", io->s.c_str());
            e.out_base64 = io->s == "output_base_64";
        } else if (const JVal* arr = io->get("byte_array")) {                          // IoEnum::ByteArray(Vec<u8>)
            if (out || arr->t != JVal::Arr) raise(kInvalidJson, "InvalidJson: bad byte_array");
            e.owned.reserve(arr->a.size());
            for (const JVal& v : arr->a) {
                if (v.t != JVal::Num || v.n < 0 || v.n > 255 || v.n != std::floor(v.n)) raise(kInvalidJson, "InvalidJson: byte_array holds integers 0..255");
                e.owned.push_back(static_cast<uint8_t>(v.n));
            }
            e.in_len = e.owned.size();
        }
        else if (const JVal* hex = io->get("bytes_hex")) {
            if (out || hex->t != JVal::Str || (hex->s.size() & 1)) raise(kInvalidJson, "InvalidJson: bad bytes_hex");
            for (size_t i = 0; i < hex->s.size(); i += 2) e.owned.push_back(static_cast<uint8_t>(std::strtoul(hex->s.substr(i, 2).c_str(), nullptr, 16)));
            e.in_len = e.owned.size();
        } else if (const JVal* b64 = io->get("base_64")) {
            if (out || b64->t != JVal::Str) raise(kInvalidJson, "InvalidJson: bad base_64");
            uint32_t acc = 0;
            int bits = 0;
            for (unsigned char ch : b64->s) {
                int v = ch >= 'A' && ch <= 'Z' ? ch - 'A' : ch >= 'a' && ch <= 'z' ? ch - 'a' + 26 : ch >= '0' && ch <= '9' ? ch - '0' + 52 : ch == '+' ? 62 : ch == '/' ? 63 : -1;
                if (v < 0) continue;
                acc = (acc << 6) | static_cast<uint32_t>(v); bits += 6;
                if (bits >= 8) { bits -= 8; e.owned.push_back(static_cast<uint8_t>(acc >> bits)); }
            }
            e.in_len = e.owned.size();
        } else raise(kActionNotSupported, "ActionNotSupported: io kind (this shim: placeholder, output_buffer, output_base_64, bytes_hex, base_64, byte_array)");
        auto& slot = c->io[id] = std::move(e);
        if (!slot.is_output) slot.in = slot.owned.data();
    }
}

// s::ResultBytes (imageflow_types/src/lib.rs): "elsewhere" for output buffers, {"base_64": ...} for IoEnum::OutputBase64
std::string result_bytes(const Job& job, int32_t io_id) {
    auto it = job.c->io.find(io_id);
    if (it == job.c->io.end() || !it->second.out_base64) return "\"elsewhere\"";
    static const char kB64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    const std::vector<uint8_t>& b = it->second.owned;
    std::string o = "{\"base_64\": \"";
    o.reserve(o.size() + (b.size() + 2) / 3 * 4 + 4);
    for (size_t i = 0; i < b.size(); i += 3) {
        const uint32_t n = (static_cast<uint32_t>(b[i]) << 16) | (i + 1 < b.size() ? static_cast<uint32_t>(b[i + 1]) << 8 : 0u) | (i + 2 < b.size() ? b[i + 2] : 0u);
        o.push_back(kB64[(n >> 18) & 63]); o.push_back(kB64[(n >> 12) & 63]);
        o.push_back(i + 1 < b.size() ? kB64[(n >> 6) & 63] : '='); o.push_back(i + 2 < b.size() ? kB64[n & 63] : '=');
    }
    return o + "\"}";
}

std::string job_result_json(const Job& job, const char* key) {
    std::string s = "{\n  \"code\": 200,\n  \"success\": true,\n  \"message\": \"OK\",\n  \"data\": {\n    \"" + std::string(key) + "\": {\n      \"encodes\": [";
    for (size_t i = 0; i < job.encodes.size(); ++i) {
        const EncodeRecord& e = job.encodes[i];
        s += std::string(i ? "," : "") + "\n        {\"preferred_mime_type\": \"" + e.mime + "\", \"preferred_extension\": \"" + e.ext + "\", \"io_id\": " +
             std::to_string(e.io_id) + ", \"w\": " + std::to_string(e.w) + ", \"h\": " + std::to_string(e.h) + ", \"bytes\": " + result_bytes(job, e.io_id) + "}";
    }
    s += "\n      ],\n      \"decodes\": [";
    for (size_t i = 0; i < job.decodes.size(); ++i) {
        const DecodeRecord& d = job.decodes[i];
        s += std::string(i ? "," : "") + "\n        {\"preferred_mime_type\": \"" + d.mime + "\", \"preferred_extension\": \"" + d.ext + "\", \"io_id\": " +
             std::to_string(d.io_id) + ", \"w\": " + std::to_string(d.w) + ", \"h\": " + std::to_string(d.h) + "}";
    }
    // s::BuildPerformance {frames: [FramePerformance {nodes: [NodePerf {wall_microseconds, name}], wall_microseconds,
    // overhead_microseconds}]} (imageflow_types/src/lib.rs:1999-2016), filled as Engine::execute_many does
    // (flow/execution_engine.rs:179-199: nodes sorted by cost, largest first).  `gpu_microseconds` is an added field:
    // the time the device spent between the node's first and last launch (hipEvents).
    std::vector<NodePerf> nodes = job.perf;
    std::stable_sort(nodes.begin(), nodes.end(), [](const NodePerf& a, const NodePerf& b) { return a.wall_ns > b.wall_ns; });
    uint64_t total_node_ns = 0;
    for (const NodePerf& n : job.perf) total_node_ns += n.wall_ns;
    const int64_t total_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - job.t_start).count();
    s += "\n      ],\n      \"performance\": {\"frames\": [{\"nodes\": [";
    for (size_t i = 0; i < nodes.size(); ++i)
        s += std::string(i ? ", " : "") + "{\"wall_microseconds\": " + std::to_string(static_cast<uint64_t>(std::llround(static_cast<double>(nodes[i].wall_ns) / 1000.0))) +
             ", \"name\": \"" + nodes[i].name + "\", \"gpu_microseconds\": " + std::to_string(static_cast<uint64_t>(std::llround(static_cast<double>(nodes[i].gpu_ms) * 1000.0))) + "}";
    s += "], \"wall_microseconds\": " + std::to_string(static_cast<uint64_t>(std::llround(static_cast<double>(total_ns) / 1000.0))) +
         ", \"overhead_microseconds\": " + std::to_string(static_cast<int64_t>(std::llround(static_cast<double>(total_ns - static_cast<int64_t>(total_node_ns)) / 1000.0))) + "}]}\n    }\n  }\n}";
    return s;
}

// ExecutionSecurity overrides a job may carry (imageflow_core/src/context.rs:640-653)
void parse_security(const JVal* sec, Security* out) {
    if (!sec || sec->t != JVal::Obj) return;
    auto limit = [&](const char* key, SizeLimit* l) {
        const JVal* v = sec->get(key);
        if (!v || v->t != JVal::Obj) return;
        l->w = want_u32(*v, "w", key); l->h = want_u32(*v, "h", key);
        const JVal* mp = v->get("megapixels");
        if (!mp || mp->t != JVal::Num) raise(kInvalidJson, "InvalidJson: %s.megapixels must be a number", key);
        l->megapixels = static_cast<float>(mp->n);
    };
    limit("max_decode_size", &out->max_decode_size);
    limit("max_frame_size", &out->max_frame_size);
    if (const JVal* v = sec->get("max_total_file_pixels"))                 // (context.rs:659-661: a value given replaces the context's, null keeps it)
        if (v->t == JVal::Num && v->n >= 0 && v->n < 18446744073709551616.0) { out->has_max_total_file_pixels = true; out->max_total_file_pixels = static_cast<uint64_t>(v->n); }
}

[[noreturn]] void abort_null_context() {                          // imageflow_abi/src/lib.rs:309-325
    fprintf(stderr, "Null context pointer provided. Terminating process.\n");
    std::abort();
}
#define CTX_OR_ABORT(c) do { if (!(c)) abort_null_context(); } while (0)

}  // namespace

// ==================================================================================================================
extern "C" {

bool imageflow_abi_compatible(uint32_t major, uint32_t minor) { return major == IMAGEFLOW_ABI_VER_MAJOR && minor <= IMAGEFLOW_ABI_VER_MINOR; }
uint32_t imageflow_abi_version_major(void) { return IMAGEFLOW_ABI_VER_MAJOR; }
uint32_t imageflow_abi_version_minor(void) { return IMAGEFLOW_ABI_VER_MINOR; }

struct imageflow_context* imageflow_context_create(uint32_t major, uint32_t minor) {       // lib.rs:430
    if (!imageflow_abi_compatible(major, minor)) return nullptr;
    try {
        imageflow_context* c = new imageflow_context;
        if (g_spread_contexts.load(std::memory_order_relaxed)) {
            const std::vector<int>& devs = usable_devices();
            if (!devs.empty()) c->device.store(devs[g_context_counter.fetch_add(1, std::memory_order_relaxed) % devs.size()], std::memory_order_relaxed);
        }
        return c;
    } catch (...) { return nullptr; }
}
bool imageflow_context_begin_terminate(struct imageflow_context* c) { CTX_OR_ABORT(c); return true; }
void imageflow_context_destroy(struct imageflow_context* c) { delete c; }

bool imageflow_context_has_error(struct imageflow_context* c) { CTX_OR_ABORT(c); std::lock_guard<std::mutex> lk(c->mu); return c->err_cat != kOk; }
int32_t imageflow_context_error_code(struct imageflow_context* c) { CTX_OR_ABORT(c); std::lock_guard<std::mutex> lk(c->mu); return c->err_cat; }
int32_t imageflow_context_error_as_exit_code(struct imageflow_context* c) { CTX_OR_ABORT(c); std::lock_guard<std::mutex> lk(c->mu); return exit_code(c->err_cat); }
int32_t imageflow_context_error_as_http_code(struct imageflow_context* c) { CTX_OR_ABORT(c); std::lock_guard<std::mutex> lk(c->mu); return http_code(c->err_cat); }
// OutwardErrorBuffer::recoverable / try_clear (imageflow_core/src/errors.rs:953-969) over FlowError::recoverable, which
// is `false` for every error today (:656-658): "recoverable" is true only while there is no error, and an error, once
// set, is never cleared -- a caller that wants to go on creates a new context.
bool imageflow_context_error_recoverable(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return c->err_cat == kOk;
}
bool imageflow_context_error_try_clear(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    std::lock_guard<std::mutex> lk(c->mu);
    return c->err_cat == kOk;
}
// lib.rs:744: print the error to stderr and exit with its exit code; returns false when there is none
bool imageflow_context_print_and_exit_if_error(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    int cat;
    std::string msg;
    { std::lock_guard<std::mutex> lk(c->mu); cat = c->err_cat; msg = c->err_msg; }
    if (cat == kOk) return false;
    fprintf(stderr, "%s\n", msg.c_str());
    std::exit(exit_code(cat));
}
// lib.rs:878: the one call meant for another thread while a job runs -- it takes no lock
void imageflow_context_request_cancellation(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    c->cancel.store(true, std::memory_order_relaxed);
}
// Context::request_cancellation_after_n_polls[_remaining] (context.rs:96-104,167-172; debug builds of the reference): the
// hook its own test_job_with_cancellation_at_every_point uses (imageflow_abi/src/lib.rs:1669-1743)
void ifhip_shim_request_cancellation_after_n_polls(struct imageflow_context* c, int64_t polls) {
    CTX_OR_ABORT(c);
    c->poll_countdown.store(polls, std::memory_order_seq_cst);
}
int ifhip_shim_process_constraint(const char* mode, int32_t source_w, int32_t source_h, int64_t w, int64_t h, int has_gravity, float gravity_x,
                                  float gravity_y, uint32_t* crop, int32_t* scale_to, uint32_t* pad, int32_t* canvas, int* flags) {
    if (!mode || !crop || !scale_to || !pad || !canvas || !flags) return 2;
    const int m = ifhip::constraint_mode_from_name(mode);
    if (m < 0) return 2;
    ifhip::ConstraintLayout l;
    std::string err;
    if (!ifhip::process_constraint(m, source_w, source_h, w, h, has_gravity != 0, gravity_x, gravity_y, &l, &err)) return 1;
    std::memcpy(crop, l.crop, sizeof l.crop);
    std::memcpy(pad, l.pad, sizeof l.pad);
    scale_to[0] = l.scale_w; scale_to[1] = l.scale_h;
    canvas[0] = l.canvas_w; canvas[1] = l.canvas_h;
    *flags = (l.has_crop ? 1 : 0) | (l.has_pad ? 2 : 0);
    return 0;
}
int64_t ifhip_shim_cancellation_polls_remaining(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    return c->poll_countdown.load(std::memory_order_seq_cst);
}
int64_t ifhip_shim_fused_decode_resamples(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    return c->fused_decode_resamples.load(std::memory_order_relaxed);
}
int64_t ifhip_shim_coalesced_decodes(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    return c->coalesced_decodes.load(std::memory_order_relaxed);
}
// Contexts over the node's GPUs (see DeviceScope): enable != 0 -> contexts created from now on take devices round-robin
void ifhip_shim_spread_contexts(int enable) { g_spread_contexts.store(enable ? 1 : 0, std::memory_order_relaxed); }
// bind one context to a device ordinal (-1: follow the calling thread again); false and an error on the context when the
// ordinal is not a usable device
bool ifhip_shim_context_set_device(struct imageflow_context* c, int ordinal) {
    CTX_OR_ABORT(c);
    const std::vector<int>& devs = usable_devices();
    if (ordinal != -1 && std::find(devs.begin(), devs.end(), ordinal) == devs.end()) {
        std::lock_guard<std::mutex> lk(c->mu);
        c->set_error(kArgumentInvalid, "InvalidArgument: device ordinal " + std::to_string(ordinal) + " is not a usable gfx950 device");
        return false;
    }
    c->device.store(ordinal, std::memory_order_relaxed);
    return true;
}
// EXTENSION: colour management for every input of the context's jobs (see Job::color_plan_for); off by default.  Jobs written
// for the reference run unmodified with it.  discard_color_profile still wins.
// EXTENSION: the "gif" preset of `encode` writes a GIF on the device (see Job::encode); off by default, where the preset
// stays the raw-container tap it has always been.
bool ifhip_shim_context_set_gif_encoder(struct imageflow_context* c, int on) {
    CTX_OR_ABORT(c);
    c->gif_encoder.store(on != 0, std::memory_order_relaxed);
    return true;
}
// EXTENSION: animated GIFs pass through jobs (see Job::run_job); off by default, and without the GIF encoder's switch it changes nothing
bool ifhip_shim_context_set_gif_animation(struct imageflow_context* c, int on) {
    CTX_OR_ABORT(c);
    c->gif_animation.store(on != 0, std::memory_order_relaxed);
    return true;
}
// EXTENSION: lossy WebP inputs (`VP8 `, with or without `ALPH`) are decoded (see Job::decode_webp); off by default, where they
// stay ImageTypeNotSupported in the words they always had.
bool ifhip_shim_context_set_webp_lossy_decoder(struct imageflow_context* c, int on) {
    CTX_OR_ABORT(c);
    c->webp_lossy_decoder.store(on != 0, std::memory_order_relaxed);
    return true;
}
// EXTENSION: the "webplossy" preset of `encode` writes a lossy WebP on the device (see Job::encode_webp_lossy); off by default,
// where the preset stays the raw-container tap it has always been.  2: on, with the sixteen 4x4 luma modes (IFHIP_VP8_ENC_INTRA4).
bool ifhip_shim_context_set_webp_lossy_encoder(struct imageflow_context* c, int on) {
    CTX_OR_ABORT(c);
    c->webp_lossy_intra4.store(on == 2, std::memory_order_relaxed);
    c->webp_lossy_encoder.store(on != 0, std::memory_order_relaxed);
    return true;
}
// EXTENSION: the stage flags of the "webplossless" preset's coder (see Job::encode_webp_lossless); 0 by default.  An unknown bit is refused.
bool ifhip_shim_context_set_webp_lossless_flags(struct imageflow_context* c, uint32_t flags) {
    CTX_OR_ABORT(c);
    if (flags & ~IFHIP_WEBP_ENC_COLOR_INDEXING) return false;
    c->webp_lossless_flags.store(flags, std::memory_order_relaxed);
    return true;
}
bool ifhip_shim_context_set_color_management(struct imageflow_context* c, int on) {
    CTX_OR_ABORT(c);
    c->color_management.store(on != 0, std::memory_order_relaxed);
    return true;
}
// EXTENSION: the libjpeg_turbo preset's progressive / optimize_huffman_coding files are entropy-coded on the device
// (ifhip_jpeg_encode_flags_batch_device) instead of by the host writer; off by default.  The files are the same bytes.
bool ifhip_shim_context_set_device_jpeg_options(struct imageflow_context* c, int on) {
    CTX_OR_ABORT(c);
    c->device_jpeg_options.store(on != 0, std::memory_order_relaxed);
    return true;
}
int ifhip_shim_context_device(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    return c->device.load(std::memory_order_relaxed);
}
int64_t ifhip_shim_device_coded_files(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    return c->device_coded_files.load(std::memory_order_relaxed);
}
bool imageflow_context_error_write_to_buffer(struct imageflow_context* c, char* buffer, size_t buffer_length, size_t* bytes_written) {   // lib.rs:684
    CTX_OR_ABORT(c);
    if (!buffer || buffer_length == 0 || (buffer_length >> (sizeof(size_t) * 8 - 1))) { if (bytes_written) *bytes_written = 0; return false; }
    std::lock_guard<std::mutex> lk(c->mu);
    const std::string& m = c->err_msg;
    static const char kTrunc[] = "\n[truncated]\n";
    bool whole = m.size() + 1 <= buffer_length;
    size_t n;
    if (whole) { n = m.size(); std::memcpy(buffer, m.data(), n); }
    else {
        const size_t t = sizeof kTrunc - 1;
        const size_t keep = buffer_length > t + 1 ? buffer_length - 1 - t : 0;
        std::memcpy(buffer, m.data(), keep);
        const size_t tn = std::min(t, buffer_length - 1 - keep);
        std::memcpy(buffer + keep, kTrunc, tn);
        n = keep + tn;
    }
    buffer[n] = 0;
    if (bytes_written) *bytes_written = n;
    return whole;
}

bool imageflow_context_add_input_buffer(struct imageflow_context* c, int32_t io_id, const uint8_t* buffer, size_t len, imageflow_lifetime lifetime) {   // lib.rs:1137
    CTX_OR_ABORT(c);
    std::lock_guard<std::mutex> lk(c->mu);
    if (!buffer) { c->set_error(kArgumentInvalid, "NullArgument: The argument 'buffer' is null."); return false; }
    if (len >> (sizeof(size_t) * 8 - 1)) { c->set_error(kArgumentInvalid, "InvalidArgument: buffer_byte_count has its leading bit set"); return false; }
    if (c->io.count(io_id)) { c->set_error(kArgumentInvalid, "InvalidArgument: io_id " + std::to_string(io_id) + " is already in use"); return false; }
    Io e;
    if (lifetime == imageflow_lifetime_lifetime_outlives_context) { e.in = buffer; e.in_len = len; }
    else { e.owned.assign(buffer, buffer + len); e.in_len = len; }
    auto& slot = c->io[io_id] = std::move(e);
    if (lifetime != imageflow_lifetime_lifetime_outlives_context) slot.in = slot.owned.data();
    return true;
}
bool imageflow_context_add_output_buffer(struct imageflow_context* c, int32_t io_id) {       // lib.rs:1224
    CTX_OR_ABORT(c);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->io.count(io_id)) { c->set_error(kArgumentInvalid, "InvalidArgument: io_id " + std::to_string(io_id) + " is already in use"); return false; }
    Io e;
    e.is_output = true;
    c->io[io_id] = std::move(e);
    return true;
}
bool imageflow_context_get_output_buffer_by_id(struct imageflow_context* c, int32_t io_id, const uint8_t** result_buffer, size_t* result_buffer_length) {   // lib.rs:1272
    CTX_OR_ABORT(c);
    std::lock_guard<std::mutex> lk(c->mu);
    if (!result_buffer || !result_buffer_length) { c->set_error(kArgumentInvalid, "NullArgument: result pointers are null"); return false; }
    auto it = c->io.find(io_id);
    if (it == c->io.end() || !it->second.is_output) { c->set_error(kArgumentInvalid, "InvalidArgument: io_id " + std::to_string(io_id) + " is not an output buffer"); return false; }
    if (it->second.out_state == OutState::Taken) { c->set_error(kArgumentInvalid, "InvalidArgument: Output buffer for io_id " + std::to_string(io_id) + " has already been taken"); return false; }
    it->second.out_state = OutState::Lent;                          // codecs/mod.rs:602-626: a lent pointer blocks take()
    *result_buffer = it->second.owned.data();
    *result_buffer_length = it->second.owned.size();
    return true;
}
// lib.rs:1335: the bytes move out of the context into a heap block the caller frees with imageflow_buffer_free
bool imageflow_context_take_output_buffer(struct imageflow_context* c, int32_t io_id, uint8_t** result_buffer, size_t* result_buffer_length) {
    CTX_OR_ABORT(c);
    std::lock_guard<std::mutex> lk(c->mu);
    if (!result_buffer) { c->set_error(kArgumentInvalid, "NullArgument: The argument 'result_buffer' is null."); return false; }
    if (!result_buffer_length) { c->set_error(kArgumentInvalid, "NullArgument: The argument 'result_buffer_length' is null."); return false; }
    auto it = c->io.find(io_id);
    if (it == c->io.end() || !it->second.is_output) { c->set_error(kArgumentInvalid, "InvalidArgument: io_id " + std::to_string(io_id) + " is not an output buffer"); return false; }
    Io& o = it->second;
    if (o.out_state == OutState::Lent) { c->set_error(kArgumentInvalid, "InvalidArgument: Cannot take output buffer for io_id " + std::to_string(io_id) + ": a raw pointer was already lent out"); return false; }   // codecs/mod.rs:565-571
    if (o.out_state == OutState::Taken) { c->set_error(kArgumentInvalid, "InvalidArgument: Output buffer for io_id " + std::to_string(io_id) + " has already been taken"); return false; }   // :572-578
    uint8_t* p = static_cast<uint8_t*>(std::malloc(o.owned.size() ? o.owned.size() : 1));
    if (!p) { c->set_error(kOutOfMemory, "AllocationFailed: output buffer"); return false; }
    std::memcpy(p, o.owned.data(), o.owned.size());
    *result_buffer = p;
    *result_buffer_length = o.owned.size();
    std::vector<uint8_t>().swap(o.owned);
    o.out_state = OutState::Taken;
    return true;
}
// lib.rs:1385: NULL is a no-op; always true.  (`length` is what Rust's Box<[u8]> needs to rebuild the slice; malloc'd here.)
bool imageflow_buffer_free(uint8_t* buffer, size_t /*length*/) {
    std::free(buffer);
    return true;
}

const struct imageflow_json_response* imageflow_context_send_json(struct imageflow_context* c, const char* method, const uint8_t* json_buffer, size_t json_buffer_size) {   // lib.rs:944
    CTX_OR_ABORT(c);
    std::lock_guard<std::mutex> lk(c->mu);                         // operations serialise per context (lib.rs:13-33)
    if (!method) { c->set_error(kArgumentInvalid, "NullArgument: The argument 'method' is null."); return nullptr; }
    if (!json_buffer) { c->set_error(kArgumentInvalid, "NullArgument: The argument 'json_buffer' is null."); return nullptr; }
    if (json_buffer_size >> (sizeof(size_t) * 8 - 1)) { c->set_error(kArgumentInvalid, "InvalidArgument: Argument `json_buffer_size` likely came from a negative integer."); return nullptr; }
    try {
        const std::string m = method;
        if (m == "v1/get_version_info")
            return respond(c, 200, std::string("{\n  \"code\": 200,\n  \"success\": true,\n  \"message\": \"OK\",\n  \"data\": {\n    \"version_info\": {\"long_version_string\": \"") +
                                       ifhip_version() + " (libimageflow ABI subset " + std::to_string(IMAGEFLOW_ABI_VER_MAJOR) + "." + std::to_string(IMAGEFLOW_ABI_VER_MINOR) + ")\"}\n  }\n}");
        const bool build = m == "v1/build" || m == "v0.1/build", execute = m == "v1/execute" || m == "v0.1/execute";
        const bool tell = m == "v1/tell_decoder" || m == "v0.1/tell_decoder", scaled_info = m == "v1/get_scaled_image_info";
        if (!build && !execute && !tell && !scaled_info && m != "v1/get_image_info" && m != "v0.1/get_image_info") {
            c->set_error(kArgumentInvalid, "InvalidMessageEndpoint: " + m);
            return respond(c, 404, "{\n  \"success\": \"false\",\n  \"code\": 404,\n  \"message\": \"Endpoint name not understood\"}");   // json/mod.rs:158-168
        }
        if (json_buffer_size > 64u * 1024u * 1024u) raise(kArgumentInvalid, "SizeLimitExceeded: JSON payload exceeds max_json_bytes");   // ExecutionSecurity::max_json_bytes
        const JVal root = parse_json(json_buffer, json_buffer_size);
        if (root.t != JVal::Obj) raise(kInvalidJson, "InvalidJson: the message must be an object");
        // the context's device, then the job's stream and the promise its frees rest on (every release is preceded by quiesce())
        DeviceScope on_device(c->device.load(std::memory_order_relaxed));
        StreamLease lease;
        ifhip::QuiescedScope quiet;
        struct InFlight { InFlight() { g_jobs_in_flight.fetch_add(1, std::memory_order_relaxed); } ~InFlight() { g_jobs_in_flight.fetch_sub(1, std::memory_order_relaxed); } } in_flight;
        Job job{c};
        job.poll_cancel();
        if (tell) {                                                  // v1/tell_decoder {io_id, command} (json/endpoints/v1.rs:365-371)
            Io& in = job.input(static_cast<int32_t>(want_int(root, "io_id", "tell_decoder")));
            const JVal* cmd = root.get("command");
            if (!cmd) raise(kInvalidJson, "InvalidJson: tell_decoder needs a command");
            if (cmd->t == JVal::Obj && cmd->get("jpeg_downscale_hints")) {           // s::DecoderCommand::JpegDownscaleHints
                const JVal& j = *cmd->get("jpeg_downscale_hints");
                in.told = true;
                in.told_w = want_u32(j, "width", "jpeg_downscale_hints"); in.told_h = want_u32(j, "height", "jpeg_downscale_hints");
                const JVal* b = j.get("scale_luma_spatially");
                in.told_spatial = b && b->t == JVal::Bool && b->b;
                b = j.get("gamma_correct_for_srgb_during_spatial_luma_scaling");
                in.told_gamma = b && b->t == JVal::Bool && b->b;
            } else if (cmd->t == JVal::Str && cmd->s == "discard_color_profile") {
                in.told_discard_profile = true;                                      // the samples as they are; wins over colour management
            } else if (cmd->t == JVal::Obj && cmd->get("webp_decoder_hints")) {      // s::DecoderCommand::WebPDecoderHints: kept with the input
                tell_webp_hint(in, *cmd->get("webp_decoder_hints"));
            } else if (cmd->t == JVal::Obj && cmd->get("select_frame")) {            // s::DecoderCommand::SelectFrame: kept with the input
                tell_select_frame(in, *cmd->get("select_frame"));
            } else if (cmd->t == JVal::Str && cmd->s == "ignore_color_profile_errors") {
                in.told_ignore_profile_errors = true;                                // acted on where colour management is switched on
            } else if (cmd->t == JVal::Str && cmd->s == "convert_color_profile") {   // EXTENSION: colour management for this input
                in.told_convert_profile = true;
            } else {
                raise(kInvalidJson, "InvalidJson: unknown decoder command");
            }
            return respond(c, 200, "{\n  \"code\": 200,\n  \"success\": true,\n  \"message\": \"OK\",\n  \"data\": {}\n}");                 // TellDecoderV1Response {} (v1.rs:177)
        }
        if (!build && !execute) {                                    // get_image_info / get_scaled_image_info {io_id}: header facts only
            Io& in = job.input(static_cast<int32_t>(want_int(root, "io_id", "get_image_info")));
            if (Job::is_png(in)) {                                   // LibPngDecoder: scaled = unscaled, no EXIF (libpng_decoder.rs:36-56)
                ifhip_png_file_info pi;
                check(ifhip_png_info(in.in, in.in_len, &pi));
                return respond(c, 200, "{\n  \"code\": 200,\n  \"success\": true,\n  \"message\": \"OK\",\n  \"data\": {\n    \"image_info\": {\"preferred_mime_type\": \"image/png\", "
                                       "\"preferred_extension\": \"png\", \"image_width\": " + std::to_string(pi.width) + ", \"image_height\": " + std::to_string(pi.height) +
                                       ", \"frame_decodes_into\": \"" + (pi.alpha_used ? "bgra_32" : "bgr_32") + "\"}\n  }\n}");
            }
            if (Job::is_webp(in)) {                                  // WebPDecoder: the features of the file, no EXIF orientation (webp.rs:130-179)
                ifhip::WebpParsed P;
                Job::walk_webp(in, &P, c->webp_lossy_decoder.load(std::memory_order_relaxed));
                return respond(c, 200, "{\n  \"code\": 200,\n  \"success\": true,\n  \"message\": \"OK\",\n  \"data\": {\n    \"image_info\": {\"preferred_mime_type\": \"image/webp\", "
                                       "\"preferred_extension\": \"webp\", \"image_width\": " + std::to_string(P.w) + ", \"image_height\": " + std::to_string(P.h) +
                                       ", \"frame_decodes_into\": \"" + (P.has_alpha ? "bgra_32" : "bgr_32") + "\"}\n  }\n}");
            }
            if (Job::is_gif(in)) {                                   // GifDecoder::get_unscaled_image_info: no frame read yet (gif/mod.rs:181-194)
                ifhip::GifParsed P;
                check(ifhip::parse_gif_header(in.in, in.in_len, &P));
                return respond(c, 200, "{\n  \"code\": 200,\n  \"success\": true,\n  \"message\": \"OK\",\n  \"data\": {\n    \"image_info\": {\"preferred_mime_type\": \"image/gif\", "
                                       "\"preferred_extension\": \"gif\", \"image_width\": " + std::to_string(P.w) + ", \"image_height\": " + std::to_string(P.h) +
                                       ", \"frame_decodes_into\": \"bgra_32\", \"lossless\": false, \"multiple_frames\": false}\n  }\n}");
            }
            uint32_t w = 0, h = 0, bw[3], bh[3], ri = 0;
            int nc = 0;
            uint8_t hs[3], vs[3];
            uint16_t qt[192];
            int progressive = 0;
            (void)ri;
            check(ifhip_jpeg_frame_info(in.in, in.in_len, &w, &h, &nc, hs, vs, bw, bh, qt, &progressive));
            if (scaled_info && in.told && in.told_w > 0 && in.told_h > 0 && (w > in.told_w || h > in.told_h))   // MzDec::apply_downscaling on the told hints (:588-618)
                for (uint32_t i = 1; i < 8; ++i) {
                    if (i == 7) continue;
                    const uint32_t sw = static_cast<uint32_t>((static_cast<uint64_t>(w) * i + 7) / 8), sh = static_cast<uint32_t>((static_cast<uint64_t>(h) * i + 7) / 8);
                    if (sw >= in.told_w && sh >= in.told_h) { w = sw; h = sh; break; }
                }
            {   // get_unscaled_rotated_image_info / get_scaled_rotated_image_info (v1.rs:288,352 -> context.rs:486-501)
                const int flag = Job::exif_flag(in);
                if (flag >= 5 && flag <= 8) std::swap(w, h);
            }
            return respond(c, 200, "{\n  \"code\": 200,\n  \"success\": true,\n  \"message\": \"OK\",\n  \"data\": {\n    \"image_info\": {\"preferred_mime_type\": \"image/jpeg\", "
                                   "\"preferred_extension\": \"jpg\", \"image_width\": " + std::to_string(w) + ", \"image_height\": " + std::to_string(h) +
                                   ", \"frame_decodes_into\": \"bgr_32\"}\n  }\n}");
        }
        if (build) { if (const JVal* bc = root.get("builder_config")) parse_security(bc->get("security"), &job.sec); }
        else parse_security(root.get("security"), &job.sec);
        if (build) if (const JVal* ios = root.get("io")) add_io_from_json(c, *ios);
        const JVal* fw = root.get("framewise");
        if (!fw || fw->t != JVal::Obj) raise(kInvalidJson, "InvalidJson: missing framewise");
        job.run_job(*fw);
        job.settle_perf(true);
        return respond(c, 200, job_result_json(job, build ? "build_result" : "job_result"));
    } catch (const FlowErr& e) {
        return respond_error(c, e.cat, e.msg);
    } catch (const std::bad_alloc&) {
        return respond_error(c, kOutOfMemory, "AllocationFailed: host memory");
    } catch (const std::exception& e) {                              // the catch_unwind of lib.rs:973-1017
        c->set_error(kInternalError, std::string("InternalError: ") + e.what());
        return nullptr;
    }
}

bool imageflow_json_response_read(struct imageflow_context* c, const struct imageflow_json_response* r, int64_t* status, const uint8_t** buf, size_t* len) {   // lib.rs:783
    CTX_OR_ABORT(c);
    if (!r) { std::lock_guard<std::mutex> lk(c->mu); c->set_error(kArgumentInvalid, "NullArgument: The argument response_in is null."); return false; }
    if (status) *status = r->r.status;
    if (buf) *buf = reinterpret_cast<const uint8_t*>(r->r.json.data());
    if (len) *len = r->r.json.size();
    return true;
}
bool imageflow_json_response_destroy(struct imageflow_context* c, struct imageflow_json_response* r) {   // lib.rs:842
    CTX_OR_ABORT(c);
    if (!r) return true;
    std::lock_guard<std::mutex> lk(c->mu);
    for (auto it = c->responses.begin(); it != c->responses.end(); ++it)
        if (it->get() == r) { c->responses.erase(it); return true; }
    return false;
}

void* imageflow_context_memory_allocate(struct imageflow_context* c, size_t bytes, const char* /*filename*/, int32_t /*line*/) {   // lib.rs:1424
    CTX_OR_ABORT(c);
    std::lock_guard<std::mutex> lk(c->mu);
    if (bytes >> (sizeof(size_t) * 8 - 1)) { c->set_error(kArgumentInvalid, "InvalidArgument: bytes has its leading bit set"); return nullptr; }
    try {
        c->allocations.emplace_back(new uint8_t[bytes ? bytes : 1]());
        return c->allocations.back().get();
    } catch (...) { c->set_error(kOutOfMemory, "AllocationFailed"); return nullptr; }
}
bool imageflow_context_memory_free(struct imageflow_context* c, void* p, const char* /*filename*/, int32_t /*line*/) {   // lib.rs:1484
    CTX_OR_ABORT(c);
    if (!p) return true;
    std::lock_guard<std::mutex> lk(c->mu);
    for (auto it = c->allocations.begin(); it != c->allocations.end(); ++it)
        if (it->get() == p) { c->allocations.erase(it); return true; }
    return false;
}

// the coder `encode` picks for a preset given as JSON text; -1 when the text is no JSON (include/imageflow_hip.h)
int ifhip_encode_preset_coder(const char* preset_json, size_t len) {
    if (!preset_json) return -1;
    try {
        const JVal v = parse_json(reinterpret_cast<const uint8_t*>(preset_json), len);
        return encode_coder(&v);
    } catch (...) { return -1; }
}

}  // extern "C"
