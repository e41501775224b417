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
// This file is the C entry points, the io table read from a job's JSON and the JSON of a result.  Beside it: shim_errors.hpp
// (the error categories and the exception a refusal travels in), shim_json.hpp / .cpp (the JSON reader and the parameter
// readers of the nodes: no GPU runtime, tests/shim_json_check.cpp runs them under the host sanitizers), shim_runtime.hpp /
// .cpp (a job's stream and device, its device memory, the timing events), shim_job.hpp (frames, limits, the io table, the
// context, the records of a result, and the interpreter `Job`) and Job's members by stage: shim_decode.cpp (inputs into
// frames, the decode coalescer), shim_nodes.cpp (the pixel nodes), shim_encode.cpp (frames into files) and shim_interp.cpp
// (run_node, the walk over steps or a graph, the animation loop), all in namespace ifshim.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/imageflow_abi_subset.h"
#include "../../include/imageflow_hip.h"
#include "common.hpp"           // the library's per-job memory cache and thread stream (devmem.cpp)
#include "gif_read.hpp"         // the container walk of a GIF (get_image_info)
#include "webp_read.hpp"        // the RIFF walk of a WebP (get_image_info)
#include "layout.hpp"           // imageflow_riapi's constraint layout (ifhip_shim_process_constraint)
#include "shim_job.hpp"          // frames, limits, Io, the context, the records, Job; with it shim_json.hpp (JVal, parse_json, the parameter readers),
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
// EXTENSION: progressive JPEG inputs are entropy-decoded on the device (see Job::decode_jpeg); off by default, where they are
// decoded by the host reader as ever.  The getter: decodes that took the device path, and (*fell_back) those that came back.
bool ifhip_shim_context_set_device_progressive_decoder(struct imageflow_context* c, int on) {
    CTX_OR_ABORT(c);
    c->device_progressive_decoder.store(on != 0, std::memory_order_relaxed);
    return true;
}
int64_t ifhip_shim_device_progressive_decodes(struct imageflow_context* c, int64_t* fell_back) {
    CTX_OR_ABORT(c);
    if (fell_back) *fell_back = c->progressive_fallbacks.load(std::memory_order_relaxed);
    return c->progressive_device_decodes.load(std::memory_order_relaxed);
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
// EXTENSION: GRAY profiles on grey frames and LUT-based RGB profiles are converted too, by a colour link (see Job::color_plan_for);
// 0 by default.  Acts only where colour management acts.  An unknown bit is refused.  The getter: links built from profile
// bytes by this context's jobs -- a profile met again is served from the context's cache.
bool ifhip_shim_context_set_color_profile_kinds(struct imageflow_context* c, uint32_t flags) {
    CTX_OR_ABORT(c);
    if (flags & ~(IFHIP_COLOR_KIND_GRAY | IFHIP_COLOR_KIND_LUT)) return false;
    c->color_profile_kinds.store(flags, std::memory_order_relaxed);
    return true;
}
int64_t ifhip_shim_color_links_built(struct imageflow_context* c) {
    CTX_OR_ABORT(c);
    return c->color_links_built.load(std::memory_order_relaxed);
}
// EXTENSION: the libjpeg_turbo preset's progressive / optimize_huffman_coding files are entropy-coded on the device
// (ifhip_jpeg_encode_flags_batch_device) instead of by the host writer; off by default.  The files are the same bytes.
// EXTENSION: the presets `auto` and `format` of `encode`, and the output keys of a command_string's querystring, come to the
// coder the reference would pick (see Job::encode_selected, csrc/encoder_select.cpp); off by default, where both presets stay
// the raw-container tap and the keys stay refused.
bool ifhip_shim_context_set_encoder_selection(struct imageflow_context* c, int on) {
    CTX_OR_ABORT(c);
    c->encoder_selection.store(on != 0, std::memory_order_relaxed);
    return true;
}
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
