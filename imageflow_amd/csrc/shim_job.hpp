// shim_job.hpp -- what a job of the ABI shim (abi_shim.cpp) works on: frames in HBM, the limits, the io table, the context,
// the records of a job's result, the parsed resample hints, and the interpreter itself: `Job`, declared here with its members
// in shim_interp.cpp, shim_decode.cpp, shim_nodes.cpp and shim_encode.cpp.
#pragma once
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/imageflow_abi_subset.h"
#include "../../include/imageflow_hip.h"
#include "../../include/imageflow_hip_color_link.h"
#include "common.hpp"           // the library's per-job memory cache and thread stream (devmem.cpp)
#include "encoder_select.hpp"   // which coder the presets `auto` and `format` come to (encoder_select.cpp; host only)
#include "shim_json.hpp"
#include "shim_runtime.hpp"

namespace ifshim {

// ---- frames in HBM ---------------------------------------------------------------------------------------------
// A decoded JPEG whose pixel stage has not run: when the frame's one consumer is a resample, decode and resample run as ONE
// device call (ifhip_jpeg_decode_resample_batch_device: no decoded BGRA bitmap in HBM); any other consumer gets the bitmap
// through Job::dev(), which runs the pixel stage then.
// The coefficient planes and quantisation tables of one entropy-decoded BATCH of files (one geometry): jobs of different
// threads whose decodes were coalesced into one device call each hold a share and read their own image's part.
struct DecodedBatch {
    int16_t* coef[3] = {nullptr, nullptr, nullptr};      // [n][bh_c][bw_c][64]
    size_t per_image[3] = {0, 0, 0};                     // int16 elements per image and component
    uint16_t* d_qt = nullptr;                            // [n][3][64]
    uint32_t w = 0, h = 0, bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};
    int ncomp = 0;
    uint8_t hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1};
    // the last share goes when its job ends -- every job waits for its own stream before it lets go (quiesce), the
    // batch's decode itself was complete before any share was handed out
    // (... and on an error path between the decode's launch and its wait this destructor IS the wait: the planes may not
    // go back to the cache with the decode still writing them)
    ~DecodedBatch() {
        quiesce();
        for (int16_t* p : coef) if (p) (void)ifhip::cached_free(p);
        if (d_qt) (void)ifhip::cached_free(d_qt);
    }
};
struct PendingJpeg {
    ifhip_jpeg_stage* st = nullptr;
    int16_t* coef[3] = {nullptr, nullptr, nullptr};      // this image's planes inside `batch`
    uint16_t* d_qt = nullptr;
    std::shared_ptr<DecodedBatch> batch;
    ~PendingJpeg() {
        quiesce();
        if (st) ifhip_jpeg_stage_destroy(st);
        ifhip::QuiescedScope q;                          // (a job thread has one already; a share that dies elsewhere: see above)
        batch.reset();
    }
};
struct Frame {                                   // graphics/bitmaps.rs Bitmap: BGRA8, 64-byte row stride
    uint8_t* d = nullptr;                        // (null while `pending`: read it through Job::dev())
    uint32_t w = 0, h = 0, stride = 0;
    bool alpha = false;
    int compose = IFHIP_REPLACE_SELF;
    uint32_t matte = 0;
    std::unique_ptr<PendingJpeg> pending;
    size_t bytes() const { return static_cast<size_t>(h) * stride; }
    ~Frame() { job_free(d); }
};
using FramePtr = std::shared_ptr<Frame>;

// ExecutionSecurity (imageflow_types/src/lib.rs:1199-1236): the two limits that bound what this library allocates;
// defaults = sane_defaults(), a job may override them with `security` (v1/execute) / `builder_config.security` (v1/build)
struct SizeLimit { uint32_t w, h; float megapixels; };
struct Security {
    SizeLimit max_decode_size{12000, 12000, 100.f};
    SizeLimit max_frame_size{10000, 10000, 100.f};
    // Option<u64>, sane_defaults() 400 megapixels (lib.rs:1212-1235): frame count x width x height of an animation
    // (GifDecoder::check_total_pixels, codecs/gif/mod.rs:103-118).  Read by the animation path alone.
    bool has_max_total_file_pixels = true;
    uint64_t max_total_file_pixels = 400000000ull;
};
// Engine::validate_frame_size (flow/execution_engine.rs:286-325); ErrorKind::SizeLimitExceeded -> ArgumentInvalid
inline void check_size(const SizeLimit& lim, const char* what, uint64_t w, uint64_t h) {
    if (w > lim.w) raise(kArgumentInvalid, "SizeLimitExceeded: Frame width %llu exceeds %s.w %u", static_cast<unsigned long long>(w), what, lim.w);
    if (h > lim.h) raise(kArgumentInvalid, "SizeLimitExceeded: Frame height %llu exceeds %s.h %u", static_cast<unsigned long long>(h), what, lim.h);
    const float mp = static_cast<float>(w) * static_cast<float>(h) / 1000000.f;
    if (mp > lim.megapixels) raise(kArgumentInvalid, "SizeLimitExceeded: Frame megapixels %f exceeds %s.megapixels %f", static_cast<double>(mp), what, static_cast<double>(lim.megapixels));
}

constexpr char kRawMagic[8] = {'I', 'F', 'B', 'G', 'R', 'A', '1', '\0'};
constexpr size_t kRawHeader = 8 + 16;

// ---- context -----------------------------------------------------------------------------------------------------
// Output buffers: Ready -> (get_output_buffer_by_id) Lent -> stays Lent; Ready -> (take_output_buffer) Taken
// (CodecInstanceContainer, imageflow_core/src/codecs/mod.rs:421-436,560-626)
enum class OutState { Ready, Lent, Taken };
struct Io {
    bool is_output = false;
    const uint8_t* in = nullptr;
    size_t in_len = 0;
    std::vector<uint8_t> owned;                  // copied inputs (lifetime_outlives_function_call) / output bytes
    bool written = false;
    OutState out_state = OutState::Ready;
    // v1/tell_decoder {jpeg_downscale_hints} (Context::tell_decoder -> MzDec::tell_decoder, mozjpeg_decoder.rs:560-586): kept
    // with the input until its decoder runs; a decode node's own `commands` are told after these and win
    bool out_base64 = false;                     // IoEnum::OutputBase64: the job result carries the bytes as {"base_64": ...}
    bool told = false;
    uint32_t told_w = 0, told_h = 0;
    bool told_spatial = false, told_gamma = false;
    bool told_discard_profile = false;           // DecoderCommand::DiscardColorProfile (mozjpeg_decoder.rs:88-91)
    bool told_ignore_profile_errors = false;     // DecoderCommand::IgnoreColorProfileErrors (:93-96): a profile that fails leaves the samples as they are
    bool told_convert_profile = false;           // EXTENSION "convert_color_profile": this input is converted to sRGB (Job::color_plan_for)
    // DecoderCommand::WebPDecoderHints (codecs/webp.rs:181-188): the size libwebp's rescaler would decode to; acted on by a WebP input only
    bool told_webp = false;
    uint32_t told_webp_w = 0, told_webp_h = 0;
    // DecoderCommand::SelectFrame (codecs/gif/mod.rs:200-205): the frame a GIF input hands on; the other decoders ignore it
    bool told_frame = false;
    int32_t told_frame_n = 0;
};
// select_frame: an integer (s::DecoderCommand::SelectFrame(i32))
inline void tell_select_frame(Io& in, const JVal& j) {
    if (j.t != JVal::Num || !(j.n >= -2147483648.0 && j.n <= 2147483647.0)) return;
    in.told_frame = true;
    in.told_frame_n = static_cast<int32_t>(j.n);
}
// webp_decoder_hints is accepted whatever it holds, as it was before a WebP input could act on it: only a hint that
// carries both sizes is kept with the input
inline void tell_webp_hint(Io& in, const JVal& j) {
    const JVal* w = j.get("width");
    const JVal* h = j.get("height");
    if (!w || !h || w->t != JVal::Num || h->t != JVal::Num || !(w->n >= 0 && w->n <= 4294967295.0) || !(h->n >= 0 && h->n <= 4294967295.0)) return;
    in.told_webp = true;
    in.told_webp_w = static_cast<uint32_t>(w->n); in.told_webp_h = static_cast<uint32_t>(h->n);
}
struct Response {
    int64_t status;
    std::string json;
};
}  // namespace ifshim

namespace ifshim {
// The colour links of one context (csrc/color_link.hip), as the reference caches its lcms2 transforms by a hash of the profile
// (codecs/lcms2_transform.rs:124-136).  At most kMax entries, the least recently used goes; a job keeps its links alive by the
// shared pointers it holds.  Freed with the context.
struct ColorLinkCache {
    static constexpr size_t kMax = 8;
    struct Entry { uint64_t hash; size_t len; bool gray; std::shared_ptr<ifhip_color_link> link; uint64_t used; };
    std::mutex mu;
    std::vector<Entry> entries;
    uint64_t clock = 0;
};
}  // namespace ifshim

struct imageflow_json_response {                 // opaque to callers; read through imageflow_json_response_read
    ifshim::Response r;
};
struct imageflow_context {
    std::mutex mu;
    std::map<int32_t, ifshim::Io> io;
    int err_cat = ifshim::kOk;
    std::string err_msg;
    std::vector<std::unique_ptr<imageflow_json_response>> responses;
    std::vector<std::unique_ptr<uint8_t[]>> allocations;
    // CancellationToken (imageflow_core/src/context.rs:50-131): a flag another thread may set while a job holds `mu`,
    // and the reference's debug-build poll countdown ("cancel at the n-th poll", :96-104) as a test hook
    std::atomic<bool> cancel{false};
    std::atomic<int64_t> poll_countdown{INT64_MAX};
    std::atomic<int64_t> fused_decode_resamples{0};
    std::atomic<int64_t> device_coded_files{0};          // JPEG outputs whose entropy coding ran on the device (diagnostic)
    std::atomic<int64_t> coalesced_decodes{0};           // decodes of this context that shared their device call with another thread's job
    std::atomic<int> device{-1};                         // device ordinal its jobs run on; -1: the calling thread's current device
    std::atomic<bool> device_jpeg_options{false};        // EXTENSION ifhip_shim_context_set_device_jpeg_options: progressive / optimised tables coded on the device
    std::atomic<bool> gif_animation{false};              // EXTENSION ifhip_shim_context_set_gif_animation: animated GIFs run once per frame into one file
    std::atomic<bool> gif_encoder{false};                // EXTENSION ifhip_shim_context_set_gif_encoder: the "gif" preset writes a GIF on the device
    std::atomic<bool> webp_lossy_decoder{false};         // EXTENSION ifhip_shim_context_set_webp_lossy_decoder: lossy WebP inputs are decoded on the device
    std::atomic<bool> device_progressive_decoder{false}; // EXTENSION ifhip_shim_context_set_device_progressive_decoder: progressive JPEG scans are entropy-decoded on the device
    std::atomic<int64_t> progressive_device_decodes{0};  // ... decodes of this context that took that path,
    std::atomic<int64_t> progressive_fallbacks{0};       // ... and those that went back to the host reader (a refused script, a nonzero status word)
    std::atomic<bool> webp_lossy_intra4{false};          // ... with IFHIP_VP8_ENC_INTRA4 (the switch's value 2)
    std::atomic<uint32_t> webp_lossless_flags{0};        // EXTENSION ifhip_shim_context_set_webp_lossless_flags: the stage flags of the "webplossless" preset's coder
    std::atomic<bool> webp_lossy_encoder{false};         // EXTENSION ifhip_shim_context_set_webp_lossy_encoder: the "webplossy" preset writes a lossy WebP on the device
    std::atomic<bool> encoder_selection{false};          // EXTENSION ifhip_shim_context_set_encoder_selection: the presets `auto` / `format` and the querystring's output keys pick a coder
    std::atomic<bool> color_management{false};           // EXTENSION ifhip_shim_context_set_color_management: every input is converted to sRGB
    std::atomic<uint32_t> color_profile_kinds{0};        // EXTENSION ifhip_shim_context_set_color_profile_kinds: IFHIP_COLOR_KIND_GRAY | _LUT profiles are converted too
    std::atomic<int64_t> color_links_built{0};           // ... links built from profile bytes by this context's jobs (a cached link is not built again)
    ifshim::ColorLinkCache color_links;                  // ... the links, by a hash of the profile's bytes and the grey flag
    bool cancellation_requested() {
        if (cancel.load(std::memory_order_relaxed)) return true;
        if (poll_countdown.load(std::memory_order_relaxed) == INT64_MAX) return false;
        return poll_countdown.fetch_sub(1, std::memory_order_relaxed) < 1;
    }
    void set_error(int cat, const std::string& m) { if (err_cat == ifshim::kOk) { err_cat = cat; err_msg = m; } }   // first error sticks
};

namespace ifhip { struct WebpParsed; }           // webp_read.hpp: the walk of a WebP input (Job::walk_webp)

namespace ifshim {

// ---- the job interpreter ---------------------------------------------------------------------------------------
struct EncodeRecord { int32_t io_id; uint32_t w, h; const char* mime; const char* ext; };
using DecodeRecord = EncodeRecord;
struct NodePerf { const char* name; uint64_t wall_ns; float gpu_ms; hipEvent_t e0, e1; };   // s::NodePerf (imageflow_types/src/lib.rs:1999-2002); e0/e1: read at the job's end
struct ResampleHints {                                                        // s::ResampleHints (lib.rs:925-933), parsed
    bool has_sharpen = false;
    float sharpen = 0.f;
    int down = IFHIP_FILTER_ROBIDOUX, up = IFHIP_FILTER_GINSENG, space = IFHIP_SPACE_LINEAR;   // scale_render.rs:257-261,278-279
    bool has_bg = false, bg_keyword_transparent = false;
    uint32_t bg = 0;
    enum When { kDefault, kSizeDiffers, kSizeDiffersOrSharpen, kAlways } resample_when = kDefault;
    enum SWhen { kSAlways, kSDown, kSUp, kSSizeDiffers } sharpen_when = kSAlways;
};

// One job of a context: the state every stage shares, and the members that cross the files they are defined in --
// shim_interp.cpp (the core, run_node, the graph walk, the animation loop), shim_decode.cpp, shim_nodes.cpp, shim_encode.cpp.
struct Job {
    imageflow_context* c;
    std::vector<EncodeRecord> encodes;
    std::vector<DecodeRecord> decodes;
    std::vector<NodePerf> perf;
    Security sec;
    std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    bool lazy_decode = false;                                        // the decode node being run has exactly one consumer
    struct GifSource { bool seen; int repeat; uint32_t delay; bool user_input; } gif_source{false, -1, 0u, false};   // of the first GIF the job decoded
    bool has_source_io = false;                                      // the job's source (find_source, once per job): what an `auto` / `format` encode takes its cues from
    int32_t source_io = 0;

    // one executed primitive: wall clock as the reference's per-node cost (execution_engine.rs:506-538) plus the time
    // the device spent on it (hipEvents on the stream every node of this interpreter launches on)
    // A node's performance record: wall time on the host and, between two hipEvents on the job's stream, the device's time.
    // The node does NOT wait for the device when it ends -- its launches stay in flight while the host prepares the next
    // node's; the events are read once, at the job's end (settle_perf).  (Until round 5 every node ended in
    // hipEventSynchronize: 4 host/device round trips per job and, under the runtime's default spinning wait, one busy host
    // core per job in flight -- profiles/r5_abi_jobs_host_cpu.txt.)
    struct Timed {
        Job* j; const char* name; std::chrono::steady_clock::time_point t0; hipEvent_t e0 = nullptr, e1 = nullptr;
        Timed(Job* job, const char* n);
        ~Timed();
    };

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
        std::map<int32_t, bool> selected_gif;    // the outputs whose `auto` / `format` encode comes to GIF (decided before the first frame)
    } anim;

    // shim_interp.cpp
    void poll_cancel();
    void settle_perf(bool read);
    ~Job();
    FramePtr new_frame(uint32_t w, uint32_t h, bool alpha, uint32_t fill_color32 = 0, bool zero = true, int matte_canvas = -1);
    uint8_t* dev(const FramePtr& f);
    FramePtr clone(const FramePtr& in, bool clone_node = false);
    Io& input(int32_t id);
    Io& output(int32_t id);
    FramePtr run_node(const std::string& name, const JVal& p, FramePtr in, FramePtr canvas, bool in_shared);
    static void node_of(const JVal& n, std::string* name, const JVal** params);
    static bool mutates_input(const std::string& nm);
    void add_animation_pixels(uint64_t pixels_per_frame);
    uint32_t animated_frames_of(const JVal& params);
    std::vector<std::pair<int32_t, uint32_t>> animation_plan(const JVal& fw);
    void decode_animation_source(int32_t io_id, bool first);
    FramePtr animated_screen(int32_t io_id);
    void find_source(const JVal& fw);
    void run_job(const JVal& fw);
    void run_framewise(const JVal& fw);

    // shim_decode.cpp
    static bool is_png(const Io& in);
    static bool is_webp(const Io& in);
    static bool is_gif(const Io& in);
    static void walk_webp(const Io& in, ifhip::WebpParsed* P, bool lossy_decoder);
    static int exif_flag(const Io& in);
    void image_size(int32_t io_id, uint32_t* w, uint32_t* h, bool rotated = false);
    struct ColorRoute {                                              // how a decoded frame comes to sRGB: not at all, by a plan, or by a link
        bool convert = false;
        ifhip_color_plan plan;
        std::shared_ptr<ifhip_color_link> link;                      // set: the link converts, the plan is not filled
    };
    void color_plan_for(int32_t io_id, const Io& in, const char* what, const char* reference_line, const uint8_t* icc, size_t icc_len,
                        const uint32_t* gama_chrm, bool frame_is_gray, ColorRoute* route);
    std::shared_ptr<ifhip_color_link> color_link_for(const uint8_t* icc, size_t icc_len, bool frame_is_gray, int* status, const char** reason);
    void convert_to_srgb(const FramePtr& f, const ColorRoute& route);
    FramePtr decode_png(int32_t io_id, Io& in);
    FramePtr decode_webp(int32_t io_id, Io& in);
    FramePtr decode_gif(int32_t io_id, Io& in);
    FramePtr decode(int32_t io_id, uint32_t hint_w, uint32_t hint_h, bool luma_spatial, bool luma_srgb);
    ifsel::Source source_facts(int32_t io_id);
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

    // shim_nodes.cpp
    static ResampleHints parse_hints(const JVal* hints, const char* node);
    void draw_image_exact(const FramePtr& canvas, const FramePtr& in, uint32_t x, uint32_t y, uint32_t w, uint32_t h, bool compose, const ResampleHints& hi);
    FramePtr resample(const FramePtr& in, uint32_t w, uint32_t h, const JVal* hints_json);
    FramePtr constrain(const FramePtr& in, const JVal& p);
    FramePtr crop_frame(const FramePtr& in, uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2);
    FramePtr crop_whitespace(const FramePtr& in, uint32_t threshold, float percent_padding, bool in_shared);
    FramePtr round_corners(const FramePtr& in, int mode, const float radii[4], uint32_t color);
    FramePtr white_balance(const FramePtr& in, float threshold);
    FramePtr expand_frame(const FramePtr& in, uint32_t l, uint32_t t2, uint32_t r, uint32_t b, uint32_t color, bool color_is_keyword_transparent);
    FramePtr command_string(const JVal& p, FramePtr in, bool in_shared = false);
    FramePtr copy_into_canvas(const FramePtr& in, const FramePtr& canvas, uint32_t fx, uint32_t fy, uint32_t w, uint32_t h, uint32_t x, uint32_t y);
    FramePtr transposed(const FramePtr& in);
    FramePtr flip(const FramePtr& in, bool vertical);
    FramePtr apply_orientation(const FramePtr& in, int64_t flag);
    FramePtr decode_oriented(int32_t io_id, uint32_t hint_w, uint32_t hint_h, bool luma_spatial, bool luma_srgb);
    FramePtr color_matrix(const FramePtr& in, const float m[25]);
    FramePtr color_filter(const FramePtr& in, const JVal& p);
    FramePtr watermark(const FramePtr& canvas, const JVal& p);
    FramePtr node_decode(const JVal& p);
    FramePtr node_round_image_corners(const JVal& p, const FramePtr& in);
    FramePtr node_crop_whitespace(const JVal& p, const FramePtr& in, bool in_shared);
    FramePtr node_fill_rect(const std::string& name, const JVal& p, const FramePtr& in);
    FramePtr node_region(const std::string& name, const JVal& p, const FramePtr& in, bool in_shared);
    FramePtr node_color_matrix_srgb(const JVal& p, const FramePtr& in);

    // shim_encode.cpp
    void write_png(const FramePtr& f, int color_type, int level, Io& o, int32_t io_id);
    void encode(FramePtr f, int32_t io_id, const JVal* preset, bool shared);
    void encode_jpeg(FramePtr f, Io& o, int32_t io_id, const JVal* preset, const JVal* classic, bool moz, bool shared);
    void encode_png(FramePtr f, Io& o, int32_t io_id, const JVal* png, bool shared);
    void encode_pngquant(const FramePtr& f, Io& o, int32_t io_id, const JVal* pq);
    void encode_webp_lossless(const FramePtr& f, Io& o, int32_t io_id);
    void encode_gif(const FramePtr& f, Io& o, int32_t io_id);
    void encode_webp_lossy(const FramePtr& f, Io& o, int32_t io_id, const JVal* preset);
    void encode_raw(const FramePtr& f, Io& o, int32_t io_id);
    void encode_selected(FramePtr f, Io& o, int32_t io_id, const JVal* preset, bool shared);
    FramePtr matted(FramePtr f, const ifsel::Resolved& r, bool shared);
    void check_encode_node(const JVal& n);
    void collect_frame(const FramePtr& f, int32_t io_id);
    void write_animations();
};

}  // namespace ifshim
