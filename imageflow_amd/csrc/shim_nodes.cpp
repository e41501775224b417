// shim_nodes.cpp -- the pixel nodes of the ABI shim's job interpreter (Job, shim_job.hpp): resample / constrain / command_string,
// crop, expand, region, fill, flips and transposes, colour matrices, round corners, white balance and watermark, each over
// the ifhip_* entry points on frames that stay in HBM; and the parameter reading of the nodes that run_node (shim_interp.cpp)
// only dispatches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "layout.hpp"           // imageflow_riapi's constraint layout (constrain / watermark)
#include "querystring.hpp"      // imageflow_riapi's querystring: Instructions, their expansion into nodes (command_string)
#include "shim_job.hpp"

namespace ifshim {
namespace {

// Resample plans are shared by all jobs of the process (ifhip::cached_plan).  A plan dropped from the cache while a job still
// holds it is destroyed by that job's thread, behind the wait for the thread's stream -- which is the job's (StreamLease).
std::shared_ptr<ifhip_resample_plan> shared_plan(uint32_t in_w, uint32_t in_h, uint32_t w, uint32_t h, int filter, float sharpen) {
    std::shared_ptr<ifhip_resample_plan> plan;
    check(ifhip::cached_plan(in_w, in_h, w, h, filter, sharpen, &plan));
    return plan;
}

float gated_sharpen(const ResampleHints& hi, uint32_t w, uint32_t h, uint32_t in_w, uint32_t in_h) {   // scale_render.rs:55-65, 263-274
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
void constrain_params(const JVal& p, const char* node, std::string* mode, bool* has_w, bool* has_h, int64_t* tw, int64_t* th) {
    const JVal* jm = p.get("mode");
    *mode = jm && jm->t == JVal::Str ? jm->s : "";
    const JVal *jw = p.get("w"), *jh = p.get("h");
    *has_w = jw && jw->t == JVal::Num; *has_h = jh && jh->t == JVal::Num;
    *tw = *has_w ? want_u32(p, "w", node) : 0; *th = *has_h ? want_u32(p, "h", node) : 0;
}
// ConstraintGravity (imageflow_types lib.rs:1054-1061): "center" | {"percentage": {x, y}} -> false for centre / absent
bool parse_gravity(const JVal* g, float* gx, float* gy) {
    if (!g || g->is_null() || (g->t == JVal::Str && g->s == "center")) return false;
    const JVal* pc = g->get("percentage");
    const JVal *jx = pc ? pc->get("x") : nullptr, *jy = pc ? pc->get("y") : nullptr;
    if (!jx || !jy || jx->t != JVal::Num || jy->t != JVal::Num) raise(kInvalidJson, "InvalidJson: gravity is \"center\" or {\"percentage\":{x,y}}");
    *gx = static_cast<float>(jx->n); *gy = static_cast<float>(jy->n);
    return true;
}

}  // namespace

ResampleHints Job::parse_hints(const JVal* hints, const char* node) {
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

// DrawImageDef::render (flow/nodes/scale_render.rs:221-320): the one caller of the hot path.  compose = the
// node's `blend` (None = Compose).
void Job::draw_image_exact(const FramePtr& canvas, const FramePtr& in, uint32_t x, uint32_t y, uint32_t w, uint32_t h, bool compose, const ResampleHints& hi) {
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
FramePtr Job::resample(const FramePtr& in, uint32_t w, uint32_t h, const JVal* hints_json) {
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
FramePtr Job::constrain(const FramePtr& in, const JVal& p) {
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
// Crop (clone_crop_fill_expand.rs:519-541), materialised as a copy that keeps the parent's state
FramePtr Job::crop_frame(const FramePtr& in, uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2) {
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
FramePtr Job::crop_whitespace(const FramePtr& in, uint32_t threshold, float percent_padding, bool in_shared) {
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
FramePtr Job::round_corners(const FramePtr& in, int mode, const float radii[4], uint32_t color) {
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
FramePtr Job::white_balance(const FramePtr& in, float threshold) {
    Timed t(this, "white_balance_srgb_mut");
    check(ifhip_white_balance_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, threshold, nullptr, t_job_stream));
    return in;
}
// ExpandCanvas (:224-262): CreateCanvas of the colour (Bgra32 unless the colour is opaque) + CopyRectToCanvas
FramePtr Job::expand_frame(const FramePtr& in, uint32_t l, uint32_t t2, uint32_t r, uint32_t b, uint32_t color, bool color_is_keyword_transparent) {
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
FramePtr Job::command_string(const JVal& p, FramePtr in, bool in_shared) {
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
    // (with the context's encoder selection on, the output keys are read as the reference reads them instead of refused)
    const bool selection = c->encoder_selection.load(std::memory_order_relaxed);
    answer(ifhip::parse_querystring(value->s, &qs, &err, selection));
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
        // With the context's encoder selection on (ifhip_shim_context_set_encoder_selection) none of that applies: the output
        // keys make the preset calculate_encoder_preset makes (encoder.rs:31-68) -- `auto` under format=auto or a `qp`, else
        // `format`, `keep` where no format is named -- and Job::encode resolves it as the reference does.
        const int q = qs.jpeg_quality >= 0 ? qs.jpeg_quality : qs.quality;
        if (selection) {
            const std::string json = ifsel::preset_json_of(qs.out);
            const JVal preset = parse_json(reinterpret_cast<const uint8_t*>(json.data()), json.size());
            encode(out, static_cast<int32_t>(want_int(p, "encode", "command_string")), &preset, false);
        } else if (qs.jpeg_out || q >= 0) {
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

// CopyRectNodeDef::render (flow/nodes/clone_crop_fill_expand.rs:31-90)
FramePtr Job::copy_into_canvas(const FramePtr& in, const FramePtr& canvas, uint32_t fx, uint32_t fy, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
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
FramePtr Job::transposed(const FramePtr& in) {
    FramePtr t = new_frame(in->h, in->w, in->alpha, 0, true);
    check(ifhip_transpose_batch_device(dev(in), in->bytes(), in->w, in->h, in->stride, t->d, t->bytes(), t->w, t->h, t->stride, 1, t_job_stream));
    return t;
}
FramePtr Job::flip(const FramePtr& in, bool vertical) {
    check(vertical ? ifhip_flip_vertical_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, t_job_stream)
                   : ifhip_flip_horizontal_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, t_job_stream));
    return in;
}
// ApplyOrientationDef::expand (flow/nodes/rotate_flip_transpose.rs:44-66): the EXIF flag as flips and a transpose
FramePtr Job::apply_orientation(const FramePtr& in, int64_t flag) {
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
FramePtr Job::decode_oriented(int32_t io_id, uint32_t hint_w, uint32_t hint_h, bool luma_spatial, bool luma_srgb) {
    FramePtr f = decode(io_id, hint_w, hint_h, luma_spatial, luma_srgb);
    const int flag = exif_flag(input(io_id));
    if (flag < 2) return f;
    Timed t(this, "apply_orientation");
    return apply_orientation(f, flag);
}
// ColorMatrixSrgbMutDef::mutate (flow/nodes/color.rs:20-38)
FramePtr Job::color_matrix(const FramePtr& in, const float m[25]) {
    check(ifhip_apply_color_matrix_batch_device(dev(in), in->bytes(), 1, in->w, in->h, in->stride, m, t_job_stream));
    in->compose = IFHIP_BLEND_WITH_SELF;
    return in;
}
// ColorFilterSrgb::expand (flow/nodes/color.rs:49-83) with the matrices of :86-230
FramePtr Job::color_filter(const FramePtr& in, const JVal& p) {
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
FramePtr Job::watermark(const FramePtr& canvas, const JVal& p) {
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

// ---- the nodes whose parameters run_node (shim_interp.cpp) does not read itself: `name`, `p`, `in`, `in_shared` are run_node's ----
// the decode node: what the input was told, then the node's own `commands`
FramePtr Job::node_decode(const JVal& p) {
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
// s::Node::RoundImageCorners {radius, background_color}
FramePtr Job::node_round_image_corners(const JVal& p, const FramePtr& in) {
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
// s::Node::CropWhitespace {threshold: u32, percent_padding: f32}
FramePtr Job::node_crop_whitespace(const JVal& p, const FramePtr& in, bool in_shared) {
    const int64_t thr = want_int(p, "threshold", "crop_whitespace");
    if (thr < 0 || thr > 0xFFFFFFFFll) raise(kInvalidJson, "InvalidJson: crop_whitespace.threshold out of range");
    const JVal* pp = p.get("percent_padding");
    if (!pp || pp->t != JVal::Num) raise(kInvalidJson, "InvalidJson: crop_whitespace.percent_padding is a number");
    return crop_whitespace(in, static_cast<uint32_t>(thr), static_cast<float>(pp->n), in_shared);
}
// FillRect (clone_crop_fill_expand.rs:107-137)
FramePtr Job::node_fill_rect(const std::string& name, const JVal& p, const FramePtr& in) {
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
// Region / RegionPercent (clone_crop_fill_expand.rs:263-452)
FramePtr Job::node_region(const std::string& name, const JVal& p, const FramePtr& in, bool in_shared) {
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
// s::Node::ColorMatrixSrgb {matrix: [[f32;5];5]}
FramePtr Job::node_color_matrix_srgb(const JVal& p, const FramePtr& in) {
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

}  // namespace ifshim
