// shim_decode.cpp -- the decode stage of the ABI shim's job interpreter (Job, shim_job.hpp): what kind of file an input is, its
// header facts, the JPEG / PNG / WebP / GIF / raw-container decodes into frames in HBM, the colour-management step behind
// them, and the coalescer that turns the JPEG decodes of different threads into one device call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/imageflow_hip_jpeg_progressive.h"   // the device entropy decoder of progressive files (jpeg_progressive_decode.hip)
#include "color_link.hpp"      // a GRAY or LUT-based profile as a link (color_link.cpp; the kernels: color_link.hip)
#include "color_profile.hpp"   // a colour profile as a conversion plan (color_profile.cpp; the kernel: color_profile.hip)
#include "png_read.hpp"         // the PNG chunk walk and the device decode of a walked file (png_read.cpp, png_decode.hip)
#include "gif_read.hpp"         // the container walk and the device decode of a GIF (gif_read.cpp, gif_decode.hip)
#include "vp8_read.hpp"         // the host stage and the device decode of a lossy WebP (vp8_read.cpp, vp8_decode.hip)
#include "webp_read.hpp"        // the RIFF walk, the prepare and the device decode of a lossless WebP (webp_read.cpp, webp_decode.hip)
#include "shim_job.hpp"

namespace ifshim {
namespace {

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

// Progressive / multi-scan files: entropy decoding on the host (csrc/jpeg_read.cpp), planes uploaded, everything else as usual
std::shared_ptr<DecodedBatch> decode_on_host(Job& j, const Io& in, bool polled = false) {
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
    if (!polled) j.poll_cancel();                                  // (polled: the device path's poll was this decode's)
    check(ifhip_jpeg_read_coefficients_host(in.in, in.in_len, host[0].data(), host[1].data(), host[2].data(), qt));
    for (int k = 0; k < 3; ++k) {
        hip_check(job_malloc(reinterpret_cast<void**>(&b->coef[k]), host[k].size() * 2u), "hipMalloc(coefficients)");
        hip_check(static_cast<hipError_t>(ifhip::copy_to_device(b->coef[k], host[k].data(), host[k].size() * 2u)), "upload(coefficients)");
    }
    hip_check(job_malloc(reinterpret_cast<void**>(&b->d_qt), sizeof qt), "hipMalloc(qt)");
    hip_check(static_cast<hipError_t>(ifhip::copy_to_device(b->d_qt, qt, sizeof qt)), "upload(qt)");
    return b;
}

// EXTENSION (ifhip_shim_context_set_device_progressive_decoder): a progressive file's scans on the device -- prepare on this
// job's thread, one upload, the batch call with n = 1 on the job's stream (csrc/jpeg_progressive_decode.hip); the planes never
// leave HBM.  nullptr: the front end refuses the file (*polled stays false), or its status word is not 0 (*polled: the
// decoder's cancellation point has been passed) -- the caller asks the host reader, whose verdict stands.
std::shared_ptr<DecodedBatch> decode_progressive_on_device(Job& j, const Io& in, bool* polled) {
    ifhip_jpeg_progressive_prepared* p = nullptr;
    if (ifhip_jpeg_progressive_prepare(&p, in.in, in.in_len) != IFHIP_OK) return nullptr;
    struct Guard { ifhip_jpeg_progressive_prepared* p; ~Guard() { ifhip_jpeg_progressive_prepared_destroy(p); } } guard{p};
    auto b = std::make_shared<DecodedBatch>();
    uint16_t qt[192];
    check(ifhip_jpeg_progressive_prepared_info(p, &b->w, &b->h, &b->ncomp, b->hs, b->vs, b->bw, b->bh, qt, nullptr, nullptr, nullptr));
    size_t bytes[3];
    for (int k = 0; k < 3; ++k) {
        b->per_image[k] = static_cast<size_t>(b->bw[k]) * b->bh[k] * 64u;
        bytes[k] = b->per_image[k] * 2u;
        hip_check(job_malloc(reinterpret_cast<void**>(&b->coef[k]), std::max<size_t>(b->per_image[k], 64u) * 2u), "hipMalloc(coefficients)");
        if (k >= b->ncomp) hip_check(static_cast<hipError_t>(ifhip::zero_device(b->coef[k], 128u)), "clear(coefficients)");   // (as the host path uploads them)
    }
    hip_check(job_malloc(reinterpret_cast<void**>(&b->d_qt), sizeof qt + 16u), "hipMalloc(qt)");       // the tables, then the status word
    uint32_t* d_status = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(b->d_qt) + sizeof qt);
    hip_check(static_cast<hipError_t>(ifhip::copy_to_device(b->d_qt, qt, sizeof qt)), "upload(qt)");
    j.poll_cancel();                                               // the decoder's cancellation point, as decode_on_host's
    *polled = true;
    const ifhip_jpeg_progressive_prepared* files[1] = {p};
    int16_t* c0[1] = {b->coef[0]}, *c1[1] = {b->ncomp > 1 ? b->coef[1] : nullptr}, *c2[1] = {b->ncomp > 2 ? b->coef[2] : nullptr};
    check(ifhip_jpeg_progressive_decode_batch_device(files, 1, c0, c1, c2, bytes, d_status, t_job_stream));
    uint32_t word = 0;
    hip_check(hipMemcpyAsync(&word, d_status, sizeof word, hipMemcpyDeviceToHost, t_job_stream), "download(status)");
    hip_check(static_cast<hipError_t>(ifhip::wait_stream(t_job_stream)), "download(status)");
    if (word) return nullptr;                                      // (the planes go back to the cache with `b`)
    return b;
}

}  // namespace

bool Job::is_png(const Io& in) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
    return in.in_len >= 8 && std::memcmp(in.in, sig, 8) == 0;
}
bool Job::is_webp(const Io& in) {                                  // codecs/mod.rs:130-131: RIFF....WEBP, 12 bytes
    return in.in_len >= 12 && std::memcmp(in.in, "RIFF", 4) == 0 && std::memcmp(in.in + 8, "WEBP", 4) == 0;
}
// "GIF87a" / "GIF89a" and a logical screen with pixels.  A GIF8?a buffer whose screen is 0 x 0 describes no canvas to
// decode into and stays ImageTypeNotSupported (known difference: the reference reports a GIF decoding error)
bool Job::is_gif(const Io& in) {
    return in.in_len >= 13 && (std::memcmp(in.in, "GIF87a", 6) == 0 || std::memcmp(in.in, "GIF89a", 6) == 0) && (in.in[6] | in.in[7]) && (in.in[8] | in.in[9]);
}
// the walk of a WebP input for a decode: a lossy file is ImageTypeNotSupported (known difference: the reference decodes it)
// unless the context's lossy decoder is switched on (ifhip_shim_context_set_webp_lossy_decoder): then P->lossless tells the two apart
void Job::walk_webp(const Io& in, ifhip::WebpParsed* P, bool lossy_decoder) {
    int rc = ifhip::parse_webp_for_decode(in.in, in.in_len, P);
    if (rc == IFHIP_METHOD_NOT_IMPLEMENTED && lossy_decoder) rc = ifhip::parse_webp_lossy_for_decode(in.in, in.in_len, P);
    if (rc == IFHIP_METHOD_NOT_IMPLEMENTED) raise(kImageTypeNotSupported, "%s", ifhip_last_error_message());
    check(rc);
}
// What get_unscaled_unrotated_image_info tells build_auto_encoder_details about an input (codecs/auto.rs:1059-1079): the
// format, `lossless` and `multiple_frames`.  A PNG is lossless unless it has a palette (libpng_decoder.rs:49), a WebP where it
// has a VP8L image chunk, a GIF animates with more than one frame; the raw BGRA container (and anything unknown) is no source.
ifsel::Source Job::source_facts(int32_t io_id) {
    ifsel::Source s;
    auto it = c->io.find(io_id);
    if (it == c->io.end() || it->second.is_output) return s;
    const Io& in = it->second;
    if (in.in_len >= kRawHeader && std::memcmp(in.in, kRawMagic, 8) == 0) return s;
    if (is_png(in)) {
        s.kind = ifsel::kSourcePng;
        s.lossless = !(in.in_len > 25 && in.in[25] == 3);                      // IHDR's colour type
    } else if (is_gif(in)) {
        s.kind = ifsel::kSourceGif;
        uint32_t n = 0;
        s.animated = ifhip_gif_frame_count(in.in, in.in_len, &n, nullptr, nullptr, 0) == IFHIP_OK && n > 1u;
    } else if (is_webp(in)) {
        s.kind = ifsel::kSourceWebp;
        ifhip::WebpParsed P;
        s.lossless = ifhip::parse_webp(in.in, in.in_len, &P) == IFHIP_OK && P.lossless;
    } else if (in.in_len >= 2 && in.in[0] == 0xFF && in.in[1] == 0xD8) {
        s.kind = ifsel::kSourceJpeg;
    }
    return s;
}
// MzDec::get_exif_rotation_flag (mozjpeg_decoder.rs:290-292): the EXIF orientation tag of a JPEG input, -1 = none
// (a PNG has none: LibPngDecoder::get_exif_rotation_flag is None, libpng_decoder.rs:54-56)
int Job::exif_flag(const Io& in) {
    int flag = -1;
    if (in.in_len >= 4 && in.in[0] == 0xFF && in.in[1] == 0xD8) (void)ifhip_jpeg_exif_orientation(in.in, in.in_len, &flag);
    return flag;
}
// header facts of an input (get_scaled_rotated_image_info's part that watermark / command_string need); `rotated`:
// Context::swap_dimensions_by_exif (context.rs:486-501) -- flags 5..8 swap width and height
void Job::image_size(int32_t io_id, uint32_t* w, uint32_t* h, bool rotated) {
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

// ---- colour management: codecs/cms.rs::transform_to_srgb, EXTENSION -- off unless the caller switches it on ------------
// A source that is not sRGB (kind 2 of the three classifiers) and was not told discard_color_profile.  Off (the default):
// the refusal, as ever.  On (ifhip_shim_context_set_color_management, or the decoder command "convert_color_profile"):
// the plan of csrc/color_profile.cpp from the ICC bytes (`icc` non-null) or from gAMA + cHRM (`gama_chrm`: gAMA, then the
// eight cHRM values, x 100000), true = apply it to the decoded frame.  A profile of a kind that is not converted here keeps
// the refusal; a malformed one is ErrorKind::ColorProfileError (category ImageMalformed, errors.rs:241), which
// ignore_color_profile_errors swallows as the reference does for every failure of its transform
// (mozjpeg_decoder.rs:409-415, libpng_decoder.rs:376-382): the samples stay as they are.
void Job::color_plan_for(int32_t io_id, const Io& in, const char* what, const char* reference_line, const uint8_t* icc, size_t icc_len,
                         const uint32_t* gama_chrm, bool frame_is_gray, ColorRoute* route) {
    if (!c->color_management.load(std::memory_order_relaxed) && !in.told_convert_profile)
        raise(kActionNotSupported, "ActionNotSupported: io_id %d %s; this build has no colour management%s%s%s.  Tell the decoder "
              "\"discard_color_profile\" to decode the samples as they are, or keep the file on the reference.  (Conversion to sRGB on the device is an "
              "extension that is off by default: ifhip_shim_context_set_color_management, or the decoder command \"convert_color_profile\", switches it on.)",
              io_id, what, reference_line ? " (the reference converts such frames to sRGB, " : "", reference_line ? reference_line : "", reference_line ? ")" : "");
    ifhip::ColorPlanResult r;
    if (icc) r = ifhip::color_plan_from_icc(icc, icc_len, &route->plan);
    else {
        double xy[8];
        for (int k = 0; k < 8; ++k) xy[k] = gama_chrm[1 + k] / 100000.0;
        r = ifhip::color_plan_from_gamma_primaries(gama_chrm[0] / 100000.0, xy, &route->plan);
    }
    if (r.status == IFHIP_COLOR_PLANNED) { route->convert = true; return; }
    // EXTENSION ifhip_shim_context_set_color_profile_kinds: the second route, for what the planner turns away.  The profile's
    // colour space picks the flag: GRAY profiles (a table) under _GRAY, everything else that may carry A2B0 under _LUT
    const uint32_t kinds = c->color_profile_kinds.load(std::memory_order_relaxed);
    const bool gray_space = icc && icc_len >= 20u && std::memcmp(icc + 16, "GRAY", 4) == 0;
    const bool linked = icc && r.status == IFHIP_COLOR_NOT_CONVERTIBLE && (kinds & (gray_space ? IFHIP_COLOR_KIND_GRAY : IFHIP_COLOR_KIND_LUT)) != 0u;
    if (linked) {
        const char* reason = "";
        int status = r.status;
        route->link = color_link_for(icc, icc_len, frame_is_gray, &status, &reason);
        if (route->link) { route->convert = true; return; }
        if (!std::strstr(reason, "without A2B0")) { r.status = status; r.reason = reason; }     // (a matrix/TRC profile: the planner's own reason stands)
    }
    if (r.status == IFHIP_COLOR_NOT_CONVERTIBLE) {
        if (linked)
            raise(kActionNotSupported, "ActionNotSupported: io_id %d %s, and the profile is %s: %s (matrix/TRC RGB profiles, gAMA + cHRM%s%s are converted; "
                  "CMYK, %s%scurves that lift black on the matrix route are not).  Tell the decoder \"discard_color_profile\" to decode the samples as they are, or keep the "
                  "file on the reference.", io_id, what, ifhip::color_plan_status_text(r.status), r.reason,
                  (kinds & IFHIP_COLOR_KIND_GRAY) ? ", GRAY profiles with a tone curve" : "", (kinds & IFHIP_COLOR_KIND_LUT) ? ", RGB profiles with A2B0" : "",
                  (kinds & IFHIP_COLOR_KIND_GRAY) ? "" : "GRAY, ", (kinds & IFHIP_COLOR_KIND_LUT) ? "" : "Lab and LUT-based profiles, ");
        raise(kActionNotSupported, "ActionNotSupported: io_id %d %s, and the profile is %s: %s (matrix/TRC RGB profiles and gAMA + cHRM are converted; GRAY, "
              "CMYK, Lab and LUT-based profiles and curves that lift black are not).  Tell the decoder \"discard_color_profile\" to decode the samples as they are, or keep the file on "
              "the reference.", io_id, what, ifhip::color_plan_status_text(r.status), r.reason);
    }
    if (in.told_ignore_profile_errors) return;
    raise(kImageMalformed, "ColorProfileError: the colour profile of io_id %d is %s: %s.  Tell the decoder \"ignore_color_profile_errors\" to decode the "
          "samples as they are.", io_id, ifhip::color_plan_status_text(r.status), r.reason);
}
// The context's link for these profile bytes: from its cache, or built now (host only; the device copy is made by the first
// launch).  Null: *status and *reason say why.
std::shared_ptr<ifhip_color_link> Job::color_link_for(const uint8_t* icc, size_t icc_len, bool frame_is_gray, int* status, const char** reason) {
    uint64_t hash = 1469598103934665603ull;                                     // FNV-1a
    for (size_t i = 0; i < icc_len; ++i) hash = (hash ^ icc[i]) * 1099511628211ull;
    ColorLinkCache& cache = c->color_links;
    std::lock_guard<std::mutex> lock(cache.mu);
    for (ColorLinkCache::Entry& e : cache.entries)
        if (e.hash == hash && e.len == icc_len && e.gray == frame_is_gray) { e.used = ++cache.clock; *status = IFHIP_COLOR_PLANNED; return e.link; }
    ifhip_color_link* raw = nullptr;
    *status = ifhip_color_link_from_icc(icc, icc_len, frame_is_gray ? 1 : 0, &raw);
    if (*status != IFHIP_COLOR_PLANNED || !raw) {                               // the builder once more for its reason: it gives up before it samples
        ifhip::ColorLink none;
        const ifhip::ColorPlanResult r = ifhip::color_link_from_icc(icc, icc_len, frame_is_gray, &none);
        *status = r.status == IFHIP_COLOR_PLANNED ? IFHIP_COLOR_MALFORMED : r.status;
        *reason = r.status == IFHIP_COLOR_PLANNED ? "the link could not be allocated" : r.reason;
        return nullptr;
    }
    c->color_links_built.fetch_add(1, std::memory_order_relaxed);
    std::shared_ptr<ifhip_color_link> link(raw, ifhip_color_link_free);
    if (cache.entries.size() >= ColorLinkCache::kMax) {
        size_t oldest = 0;
        for (size_t i = 1; i < cache.entries.size(); ++i)
            if (cache.entries[i].used < cache.entries[oldest].used) oldest = i;
        cache.entries.erase(cache.entries.begin() + static_cast<std::ptrdiff_t>(oldest));
    }
    cache.entries.push_back({hash, icc_len, frame_is_gray, link, ++cache.clock});
    return link;
}
// in place, on the job's stream, behind the decode that filled the frame; the plan is copied by the launch, the link outlives
// it (the cache's share, and ifhip_color_link_free's wait for the device)
void Job::convert_to_srgb(const FramePtr& f, const ColorRoute& route) {
    if (route.link) check(ifhip_color_link_transform_batch_device(dev(f), f->bytes(), 1, f->w, f->h, f->stride, route.link.get(), t_job_stream));
    else check(ifhip_color_transform_batch_device(dev(f), f->bytes(), 1, f->w, f->h, f->stride, &route.plan, t_job_stream));
}

// LibPngDecoder::read_frame (codecs/libpng_decoder.rs:82-104 -> c_components/lib/codec_png_wrapper.c:131-246) on the device:
// the host walks the chunks, the IDAT stream is inflated, un-filtered and expanded to BGRA by csrc/png_decode.hip.  The
// JPEG downscale hints do not apply (tell_decoder accepts and ignores them, libpng_decoder.rs:58-80).
FramePtr Job::decode_png(int32_t io_id, Io& in) {
    ifhip::PngParsed P;                                                           // ONE walk over the chunks: the facts and where the IDAT payloads lie
    check(ifhip::parse_png(in.in, in.in_len, &P, true));                          // a bad CRC, a malformed critical chunk: ImageMalformed
    check_size(sec.max_decode_size, "max_decode_size", P.w, P.h);                 // on the header, before anything is staged
    // The colour policy of the JPEG path below (DESIGN 8 "Colour management"): the reference transforms a frame whose iCCP,
    // or gAMA + cHRM, is not sRGB (libpng_decoder.rs:340-383); so does this build once switched on, else it refuses -- never
    // other colours.
    ColorRoute route;
    if (!in.told_discard_profile && P.color_kind == 2) {
        static const uint8_t kNoProfile = 0;                                      // an iCCP that did not inflate: zero bytes of profile, malformed
        uint32_t gama_chrm[9] = {P.gama};
        std::memcpy(gama_chrm + 1, P.chrm, sizeof P.chrm);
        color_plan_for(io_id, in, P.has_iccp ? "carries an embedded ICC profile that is not sRGB" : "carries gAMA and cHRM chunks that do not describe sRGB",
                       "codecs/libpng_decoder.rs:376", P.has_iccp ? (P.icc.empty() ? &kNoProfile : P.icc.data()) : nullptr, P.icc.size(), gama_chrm,
                       P.color_type == 0u || P.color_type == 4u, &route);
    }
    if (P.inflated > 0x7FFF0000ull) raise(kImageMalformed, "ImageMalformed: LibPNG error: the image data of io_id %d would inflate beyond 2^31 bytes", io_id);
    FramePtr f = new_frame(P.w, P.h, P.alpha_used, 0, true);                      // (max_frame_size inside)
    const ifhip::PngParsed* parsed = &P;
    const size_t bytes = f->bytes();
    const uint32_t status = decoded_status("decode(png)", [&](uint32_t* d_status) { return ifhip::png_decode_parsed_device(&parsed, 1, &f->d, &bytes, &f->stride, d_status, t_job_stream); });
    if (status) raise(kImageMalformed, "ImageMalformed: LibPNG error: %s (io_id %d, status %u)", ifhip::png_status_text(status), io_id, status);
    if (route.convert) convert_to_srgb(f, route);
    decodes.push_back({io_id, P.w, P.h, "image/png", "png"});
    return f;
}

// WebPDecoder::read_frame (codecs/webp.rs:162-248 -> WebPDecode, MODE_BGRA) on the device for a lossless file: the host walks
// the container and prepares the stream, the token loop and the inverse transforms run in csrc/webp_decode.hip.  The JPEG
// downscale hints are accepted and ignored; a told WebP hint that differs from the file's size would need libwebp's
// decode-time rescaler (webp.rs:181-188), which is not built.
FramePtr Job::decode_webp(int32_t io_id, Io& in) {
    ifhip::WebpParsed P;
    walk_webp(in, &P, c->webp_lossy_decoder.load(std::memory_order_relaxed));
    check_size(sec.max_decode_size, "max_decode_size", P.w, P.h);                 // on the header, before anything is staged
    ColorRoute route;
    if (!in.told_discard_profile && P.color_kind == 2)
        color_plan_for(io_id, in, "carries an embedded ICC profile that is not sRGB", nullptr, P.icc, P.icc_len, nullptr, false, &route);
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
    if (route.convert) convert_to_srgb(f, route);
    decodes.push_back({io_id, P.w, P.h, "image/webp", "webp"});
    return f;
}

// GifDecoder::read_frame (codecs/gif/mod.rs:207-298) on the device: the host walks the container up to the selected frame
// (csrc/gif_read.cpp), the LZW streams of frames 0..N are decoded and the frames composed with their disposal by
// csrc/gif_decode.hip; frame N's screen enters the graph as bgra_32 with meaningful alpha.  The limits come first, on the
// header (mod.rs:55-85: max_decode_size, else max_frame_size, on the logical screen).  GIF carries neither EXIF nor a
// colour profile; the JPEG and WebP hints are accepted and ignored.
FramePtr Job::decode_gif(int32_t io_id, Io& in) {
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
FramePtr Job::decode(int32_t io_id, uint32_t hint_w, uint32_t hint_h, bool luma_spatial, bool luma_srgb) {
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
    ColorRoute route;
    {   // MzDec::read_frame transforms the frame to sRGB whenever the file carries an ICC profile (mozjpeg_decoder.rs:370-420)
        // unless the decoder was told discard_color_profile (:88-91).  A profile that is not sRGB itself would come out with
        // other colours than the reference's: the job is refused -- loudly -- unless colour management is switched on, and
        // then the frame is converted behind its decode (a profile that IS sRGB: the reference's transform is the identity up
        // to its rounding).
        int kind = 0;
        std::vector<uint8_t> icc;
        if (!in.told_discard_profile && ifhip::jpeg_icc_profile(in.in, in.in_len, &kind, &icc) == IFHIP_OK && kind == 2) {
            uint32_t fw = 0, fh = 0, bw[3], bh[3];                                    // a one-component file is a grey frame (mozjpeg_decoder.rs:387-404)
            int nc = 0, progressive = 0;
            uint8_t hs3[3], vs3[3];
            uint16_t qt[192];
            const bool gray = ifhip_jpeg_frame_info(in.in, in.in_len, &fw, &fh, &nc, hs3, vs3, bw, bh, qt, &progressive) == IFHIP_OK && nc == 1;
            color_plan_for(io_id, in, "carries an embedded ICC profile that is not sRGB", "codecs/mozjpeg_decoder.rs:409", icc.data(), icc.size(), nullptr, gray, &route);
        }
    }
    // the entropy stage: this file, together with whatever other threads' jobs want decoded right now (DecodeCoalescer)
    DecodeRequest rq;
    const int prc = ifhip_jpeg_entropy_prepare(&rq.prepared, in.in, in.in_len);          // parse, un-stuff, pack, tables: on this job's thread
    struct PreparedGuard { ifhip_jpeg_prepared* p; ~PreparedGuard() { ifhip_jpeg_prepared_destroy(p); } } prepared_guard{rq.prepared};
    if (prc == IFHIP_METHOD_NOT_IMPLEMENTED) {
        // not a single-scan baseline file: progressive (what the reference's mozjpeg preset writes) or multi-scan -- the scans
        // are decoded on the host as MzDec does (libjpeg's jdphuff.c), the pixel stage behind them stays on the GPU
        bool polled = false;
        if (c->device_progressive_decoder.load(std::memory_order_relaxed)) {
            rq.batch = decode_progressive_on_device(*this, in, &polled);
            (rq.batch ? c->progressive_device_decodes : c->progressive_fallbacks).fetch_add(1, std::memory_order_relaxed);
        }
        if (!rq.batch) rq.batch = decode_on_host(*this, in, polled);
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
    if (route.convert) convert_to_srgb(f, route);
    {   // Context::get_image_decodes reports get_unscaled_rotated_image_info (context.rs:519-538)
        const int flag = exif_flag(in);
        const bool swap = flag >= 5 && flag <= 8;
        decodes.push_back({io_id, swap ? h : w, swap ? w : h, "image/jpeg", "jpg"});
    }
    return f;
}

}  // namespace ifshim
