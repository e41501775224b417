// shim_interp.cpp -- the core of the ABI shim's job interpreter (Job, shim_job.hpp): cancellation, the nodes' performance
// records, frames and the io table; run_node, which names a node's primitive and hands it to its stage (shim_decode.cpp,
// shim_nodes.cpp, shim_encode.cpp); the walk over `steps` or a `graph`; and the frame loop of an animated GIF.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "gif_read.hpp"         // the container walk and the device decode of a GIF (gif_read.cpp, gif_decode.hip)
#include "shim_job.hpp"

namespace ifshim {

// return_if_cancelled! (imageflow_core/src/errors.rs:124-140; polled in Engine::graph_execute before every node,
// execution_engine.rs:502, at every bitmap borrow, context.rs:389-401, and inside the codecs)
void Job::poll_cancel() {
    if (c->cancellation_requested()) raise(kOperationCancelled, "OperationCancelled: the job was cancelled");
}

Job::Timed::Timed(Job* job, const char* n) : j(job), name(n), t0(std::chrono::steady_clock::now()) {
    const int dev = j->c->device.load(std::memory_order_relaxed);
    e0 = timing_events().take(dev); e1 = timing_events().take(dev);
    if (!e0 || !e1 || hipEventRecord(e0, t_job_stream) != hipSuccess) {
        (void)hipGetLastError();
        timing_events().give(dev, e0); timing_events().give(dev, e1);
        e0 = e1 = nullptr;
    }
}
Job::Timed::~Timed() {
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
// the device times of the nodes, once the job's stream has drained; `read` false (a failed job): the events just go back
void Job::settle_perf(bool read) {
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
Job::~Job() { settle_perf(false); }

// matte_canvas: the frame is CreateCanvas' result for a colour other than the enum value Transparent (-1: decide by the
// colour's alpha, for callers that have no JSON colour)
FramePtr Job::new_frame(uint32_t w, uint32_t h, bool alpha, uint32_t fill_color32, bool zero, int matte_canvas) {
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
uint8_t* Job::dev(const FramePtr& f) {
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
// clone_node: the Clone node MutProtect puts before a mutating node whose parent has other children (definitions.rs:
// 320-341) = CreateCanvas(Transparent, parent.fmt) + CopyRectToCanvas (clone_crop_fill_expand.rs:151-175), which leaves
// the copy in BlendWithSelf (copy_rect.rs:37); otherwise a private copy of this interpreter's that keeps the frame's state
FramePtr Job::clone(const FramePtr& in, bool clone_node) {
    FramePtr c2 = new_frame(in->w, in->h, in->alpha, 0, false);
    hip_check(hipMemcpyAsync(c2->d, dev(in), in->bytes(), hipMemcpyDeviceToDevice, t_job_stream), "clone");
    if (clone_node) c2->compose = IFHIP_BLEND_WITH_SELF;
    else { c2->compose = in->compose; c2->matte = in->matte; }
    return c2;
}

Io& Job::input(int32_t id) {
    auto it = c->io.find(id);
    if (it == c->io.end() || it->second.is_output) raise(kArgumentInvalid, "InvalidArgument: io_id %d is not a registered input", id);
    return it->second;
}
Io& Job::output(int32_t id) {
    auto it = c->io.find(id);
    if (it == c->io.end() || !it->second.is_output) raise(kArgumentInvalid, "InvalidArgument: io_id %d is not a registered output", id);
    return it->second;
}

// one node: `in` is the frame of its input edge (null for source nodes), `canvas` the frame of its canvas edge
FramePtr Job::run_node(const std::string& name, const JVal& p, FramePtr in, FramePtr canvas, bool in_shared) {
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
    if (name == "decode") return node_decode(p);
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
    if (name == "round_image_corners") return node_round_image_corners(p, in);
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
    if (name == "crop_whitespace") return node_crop_whitespace(p, in, in_shared);
    Timed t(this, name == "fill_rect" ? "fill_rect_mutate" : name == "crop" ? "crop_mutate" : name == "flip_v" ? "flip_vertical_mutate" : name == "flip_h" ? "flip_vertical_mutate" /* sic: rotate_flip_transpose.rs:206 */
                  : name == "color_matrix_srgb" || name == "color_filter_srgb" ? "color_matrix_srgb_mut" : name == "expand_canvas" || name == "region" || name == "region_percent" ? "expand_canvas" : name == "transpose" ? "transpose_mut"
                  : name == "rotate_90" ? "rotate_90" : name == "rotate_180" ? "rotate_180" : name == "rotate_270" ? "rotate_270" : name == "apply_orientation" ? "apply_orientation" : "node");
    if (name == "fill_rect") return node_fill_rect(name, p, in);
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
    if (name == "region" || name == "region_percent") return node_region(name, p, in, in_shared);
    if (name == "color_matrix_srgb") return node_color_matrix_srgb(p, in);
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

void Job::node_of(const JVal& n, std::string* name, const JVal** params) {
    if (n.t == JVal::Str) { *name = n.s; static const JVal kNull; *params = &kNull; return; }
    if (n.t != JVal::Obj || n.o.size() != 1) raise(kInvalidJson, "InvalidJson: a node is {\"name\": {params}}");
    *name = n.o[0].first;
    *params = &n.o[0].second;
}
bool Job::mutates_input(const std::string& nm) {
    return nm == "fill_rect" || nm == "watermark_red_dot" || nm == "flip_v" || nm == "flip_h" || nm == "rotate_180" || nm == "color_matrix_srgb" || nm == "color_filter_srgb" ||
           nm == "apply_orientation" || nm == "watermark" || nm == "round_image_corners" || nm == "white_balance_histogram_area_threshold_srgb";
}

void Job::add_animation_pixels(uint64_t pixels_per_frame) {
    anim.pixels += pixels_per_frame * anim.n;
    if (sec.has_max_total_file_pixels && anim.pixels > sec.max_total_file_pixels)
        raise(kArgumentInvalid, "SizeLimitExceeded: GIF total decoded pixels (%u frames x %llu pixels, %llu in the job) exceeds max_total_file_pixels %llu", anim.n,
              static_cast<unsigned long long>(pixels_per_frame), static_cast<unsigned long long>(anim.pixels), static_cast<unsigned long long>(sec.max_total_file_pixels));
}
// a `decode` node whose input animates: a GIF of more than one frame that no select_frame was told to (-> its frame count)
uint32_t Job::animated_frames_of(const JVal& params) {
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
std::vector<std::pair<int32_t, uint32_t>> Job::animation_plan(const JVal& fw) {
    std::vector<std::pair<int32_t, uint32_t>> found;
    const bool gif_on = c->gif_encoder.load(std::memory_order_relaxed), selection = c->encoder_selection.load(std::memory_order_relaxed);
    // With encoder selection on, an `auto` / `format` encode -- a node's preset, or what a command_string's querystring makes
    // (one without a decode of its own) -- that comes to GIF is a "gif" node too.  The GIF outcomes are `format: gif`, `keep` on a
    // GIF source and auto-selection on an animated source, which returns GIF before it looks at the frame (auto.rs:1154-1159):
    // all known here, before the first frame, from the preset and the job's source (Job::find_source).  *selected_io: the
    // output of such an encode, for the caller to mark once an animated decode is known to feed it.
    auto is_gif_encode = [&](const std::string& name, const JVal& p, int32_t* selected_io, bool* is_selected) {
        *is_selected = false;
        const JVal* preset = p.get("preset");
        if (name == "encode" && preset && preset->t == JVal::Str && preset->s == "gif") return gif_on;
        if (!selection) return false;
        const ifsel::Source src = has_source_io ? source_facts(source_io) : ifsel::Source();
        int64_t io_id = 0;
        JVal made;
        if (name == "encode" && ifsel::names_selection(preset)) io_id = want_int(p, "io_id", "encode");
        else if (name == "command_string" && p.get("encode") && p.get("encode")->t == JVal::Num && !(p.get("decode") && p.get("decode")->t == JVal::Num)) {
            const JVal* value = p.get("value");
            ifhip::Ir4Instructions qs;
            std::string err;
            if (!value || value->t != JVal::Str || ifhip::parse_querystring(value->s, &qs, &err, true) != ifhip::kQsOk) return false;   // (the node itself answers)
            const std::string json = ifsel::preset_json_of(qs.out);
            made = parse_json(reinterpret_cast<const uint8_t*>(json.data()), json.size());
            preset = &made;
            io_id = want_int(p, "encode", "command_string");
        } else return false;
        if (!ifsel::resolves_to_gif_without_frame(ifsel::read_preset(*preset), src)) return false;
        *selected_io = static_cast<int32_t>(io_id);
        *is_selected = true;
        return true;
    };
    auto add = [&](const JVal& p, uint32_t n) {
        const int32_t id = static_cast<int32_t>(p.get("io_id")->n);
        for (const auto& f : found) if (f.first == id) return;
        found.push_back({id, n});
    };
    std::string name;
    const JVal* params;
    int32_t selected_io = 0;
    bool is_selected = false;
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
                if (!is_gif_encode(name, *params, &selected_io, &is_selected)) continue;   // (every one of them: a selected encode is marked as it is found)
                add(*source, n);
                if (is_selected) anim.selected_gif[selected_io] = true;
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
        if (!is_gif_encode(name, *params, &selected_io, &is_selected)) continue;
        bool animated_ancestor = false;
        std::vector<int64_t> todo{kv.first};
        std::map<int64_t, bool> seen;
        while (!todo.empty()) {                                                      // every ancestor, over input and canvas edges
            const int64_t id = todo.back();
            todo.pop_back();
            if (seen[id] || !by_id.count(id)) continue;
            seen[id] = true;
            node_of(*by_id[id], &name, &params);
            if (name == "decode") if (const uint32_t n = animated_frames_of(*params)) { add(*params, n); animated_ancestor = true; }
            auto range = parents.equal_range(id);
            for (auto it = range.first; it != range.second; ++it) todo.push_back(it->second);
        }
        if (is_selected && animated_ancestor) anim.selected_gif[selected_io] = true;   // (a selected encode a still source feeds takes frame 0, as in steps)
    }
    return found;
}
// The input an `auto` / `format` encode takes its cues from (the first of the reference's decoder_io_ids, auto.rs:1055-1066),
// found ONCE per job, before any node runs: the first node in step order -- of a graph, the node of the lowest id -- that
// decodes an input: a `decode`, or a `command_string` with a decode of its own.  A watermark's input is never it.
void Job::find_source(const JVal& fw) {
    auto decodes_io = [&](const JVal& n) {
        std::string name;
        const JVal* p;
        node_of(n, &name, &p);
        const JVal* id = name == "decode" ? p->get("io_id") : name == "command_string" ? p->get("decode") : nullptr;
        if (!id || id->t != JVal::Num) return false;
        has_source_io = true;
        source_io = static_cast<int32_t>(id->n);
        return true;
    };
    if (const JVal* steps = fw.get("steps")) {
        if (steps->t == JVal::Arr) for (const JVal& n : steps->a) if (decodes_io(n)) return;
        return;
    }
    const JVal* graph = fw.get("graph");
    const JVal* nodes = graph ? graph->get("nodes") : nullptr;
    if (!nodes || nodes->t != JVal::Obj) return;
    std::map<int64_t, const JVal*> by_id;
    for (const auto& kv : nodes->o) by_id[std::atoll(kv.first.c_str())] = &kv.second;
    for (const auto& kv : by_id) if (decodes_io(*kv.second)) return;
}
// every screen of one animated source, decoded and composed once
void Job::decode_animation_source(int32_t io_id, bool first) {
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
FramePtr Job::animated_screen(int32_t io_id) {
    const AnimSource& src = *anim.sources[io_id];
    FramePtr f = new_frame(src.w, src.h, true, 0, false);
    hip_check(hipMemcpyAsync(f->d, src.d + static_cast<size_t>(anim.k) * f->bytes(), f->bytes(), hipMemcpyDeviceToDevice, t_job_stream), "copy(screen)");
    decodes.push_back({io_id, src.w, src.h, "image/gif", "gif"});
    return f;
}
// a job: once, or -- where the animation path applies -- once per frame of the animated sources
void Job::run_job(const JVal& fw) {
    if (c->encoder_selection.load(std::memory_order_relaxed)) find_source(fw);
    // (the "gif" preset collects frames where the GIF encoder is on, an `auto` / `format` preset where encoder selection is)
    if (!c->gif_animation.load(std::memory_order_relaxed) || !(c->gif_encoder.load(std::memory_order_relaxed) || c->encoder_selection.load(std::memory_order_relaxed)))
        return run_framewise(fw);
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

void Job::run_framewise(const JVal& fw) {
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

}  // namespace ifshim
