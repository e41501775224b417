// Constraint layout (see layout.hpp).  A restatement of the parts of imageflow_riapi that `process_constraint` runs for
// the nine ConstraintMode values: AspectRatio (sizing.rs:14-222), Layout and its steps (sizing.rs:267-471), the step
// programs per (mode, scale) pair (ir4/layout.rs:160-283), target size (:105-139), gravity (:673-698), results (:334-412).
// Integer and f64 / f32 arithmetic in the reference's order, so that a size that rounds at .5 rounds the same way.
// The querystring's own layout (ir4_crop_and_layout) runs the same step programs, plus the UpscaleCanvas rows that no
// ConstraintMode reaches, behind get_precrop / get_initial_copy_window (:47-61, :700-775) and get_wh_from_all (:63-91).
#include "layout.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace ifhip {
namespace {

struct LayoutErr { std::string text; };

struct AR {                                            // sizing::AspectRatio: w, h >= 1
    int32_t w, h;
    double ratio() const { return static_cast<double>(w) / static_cast<double>(h); }          // :44-46
    bool aspect_wider_than(const AR& other) const { return other.ratio() > ratio(); }         // :54-56
    bool exceeds_any(const AR& o) const { return w > o.w || h > o.h; }                         // :200-202
};
std::string dbg(const AR& a) { return std::to_string(a.w) + "x" + std::to_string(a.h); }

AR create(int64_t w, int64_t h) {                      // AspectRatio::create (:35-42)
    if (w < 1 || h < 1) throw LayoutErr{"InvalidDimensions { w: " + std::to_string(w) + ", h: " + std::to_string(h) + " }"};
    return AR{static_cast<int32_t>(w), static_cast<int32_t>(h)};
}

enum BoxKind { kInner, kOuter };

// AspectRatio::proportional (:118-181) with rounding_loss_based_on_target_width / _height (:81-115)
int32_t proportional(const AR& self, int32_t basis, bool basis_is_width, const AR* target) {
    double snap_amount = 1.0 - 2.220446049250313e-16;                                          // 1f64 - f64::EPSILON
    const double ratio = self.ratio();
    if (target) {
        if (!basis_is_width) {
            const double target_x_to_self_x = static_cast<double>(target->w) / static_cast<double>(self.w);
            const double rounded_y = std::round(static_cast<double>(self.h) * target_x_to_self_x);
            snap_amount = std::fabs(static_cast<double>(target->w) - rounded_y * ratio);
        } else {
            const double target_y_to_self_y = static_cast<double>(target->h) / static_cast<double>(self.h);
            const double rounded_x = std::round(static_cast<double>(self.w) * target_y_to_self_y);
            snap_amount = std::fabs(static_cast<double>(target->h) - rounded_x / ratio);
        }
    }
    const int32_t snap_a = basis_is_width ? self.h : self.w;
    const int32_t snap_b = target ? (basis_is_width ? target->h : target->w) : snap_a;
    const double f = basis_is_width ? static_cast<double>(basis) / ratio : ratio * static_cast<double>(basis);
    const double delta_a = f - static_cast<double>(snap_a), delta_b = f - static_cast<double>(snap_b);
    int64_t v;
    if (std::fabs(delta_a) <= snap_amount && std::fabs(delta_a) <= std::fabs(delta_b)) v = snap_a;
    else if (std::fabs(delta_b) <= snap_amount) v = snap_b;
    else {
        const double rounded = std::round(f);
        if (rounded <= -2147483648.0 || rounded >= 2147483647.0) throw LayoutErr{"ValueScalingFailed"};
        v = static_cast<int64_t>(rounded);
    }
    if (v < 0) throw LayoutErr{"ValueScalingFailed"};
    return v == 0 ? 1 : static_cast<int32_t>(v);
}

AR box_of(const AR& self, const AR& target, BoxKind kind) {                                   // :185-193
    if (target.aspect_wider_than(self) == (kind == kInner)) return create(target.w, proportional(self, target.w, true, &target));
    return create(proportional(self, target.h, false, &target), target.h);
}
AR intersection(const AR& a, const AR& b) { return create(std::min(a.w, b.w), std::min(a.h, b.h)); }   // :207-209
AR distort_with(const AR& self, const AR& other_old, const AR& other_new) {                    // :211-219, mult_fraction :245-247
    return create(static_cast<int32_t>(static_cast<int64_t>(self.w) * other_new.w / other_old.w),
                  static_cast<int32_t>(static_cast<int64_t>(self.h) * other_new.h / other_old.h));
}

struct Layout {                                        // sizing::Layout (:267-274)
    AR source, target, canvas, image;
    void scale_canvas(BoxKind kind) {                  // :304-311 (target = self.target)
        const AR nc = box_of(canvas, target, kind);
        image = distort_with(image, canvas, nc);
        canvas = nc;
    }
    void distort_canvas(const AR& t) { image = distort_with(image, canvas, t); canvas = t; }   // :318-325
    void pad_canvas(const AR& t) {                     // :332-337
        if (canvas.exceeds_any(t)) throw LayoutErr{"ImpossiblePad { target: " + dbg(t) + ", current: " + dbg(canvas) + " }"};
        canvas = t;
    }
    void virtual_canvas(const AR& t) {                 // :333-337
        const AR ni = intersection(image, t);
        source = box_of(ni, source, kInner);
        image = ni;
        canvas = t;
    }
    void crop(const AR& t) {                           // :339-346
        if (t.exceeds_any(canvas)) throw LayoutErr{"ImpossibleCrop { target: " + dbg(t) + ", current: " + dbg(canvas) + " }"};
        const AR ni = intersection(image, t);
        source = box_of(ni, source, kInner);
        image = ni;
        canvas = t;
    }
    int cmp_w() const { return canvas.w < target.w ? -1 : canvas.w > target.w ? 1 : 0; }      // canvas.cmp_size(&target) (:221-223, :419-421)
    int cmp_h() const { return canvas.h < target.h ? -1 : canvas.h > target.h ? 1 : 0; }
    bool either(int o) const { return cmp_w() == o || cmp_h() == o; }                          // Cond::Either / Neither (:538-540)
    bool neither(int o) const { return cmp_w() != o && cmp_h() != o; }
    bool larger_1d_smaller_1d() const { return (cmp_w() > 0 && cmp_h() < 0) || (cmp_w() < 0 && cmp_h() > 0); }   // :524-527
};

// `x as i32` of a float: NaN is 0, everything else saturates
int32_t as_i32(double v) { return v != v ? 0 : v >= 2147483647.0 ? INT32_MAX : v <= -2147483648.0 ? INT32_MIN : static_cast<int32_t>(v); }

// gravity1d (ir4/layout.rs:673-683)
int32_t gravity1d(float align_percentage, int32_t inner, int32_t outer) {
    const float ratio = std::min(std::max(align_percentage, 0.f), 100.f) / 100.f;             // (f32::clamp keeps a NaN, as these do)
    if ((outer < inner && inner < 1) || outer < 1) throw LayoutErr{"Outer box should never be smaller than inner box. All values must > 0"};
    const float v = std::round(static_cast<float>(outer - inner) * ratio);
    return std::max<int32_t>(0, std::min<int32_t>(as_i32(v), outer - inner));
}

// the step programs of build_constraints (:160-283), run as execute_all runs them (sizing.rs:436-463): a failed SkipUnless / a
// met SkipIf skips to the next BeginSequence; conditions compare the CURRENT canvas with the target
void run_constraints(Layout& lay, int fit, int scale) {
    const bool gate_down = lay.either(1), gate_up = lay.neither(1);                            // Either(Greater) / Neither(Greater)
    const bool gate = scale == kIr4Both || ((scale == kIr4Down || scale == kIr4Canvas) && gate_down) || (scale == kIr4Up && gate_up);
    if (fit == kIr4Max) {
        if (gate) lay.scale_canvas(kInner);
        if (scale == kIr4Canvas) lay.virtual_canvas(box_of(lay.canvas, lay.target, kInner));   // BoxOf {target: Target, ratio_source: CurrentCanvas, Inner}
    } else if (fit == kIr4Pad) {
        if (scale == kIr4Canvas) { if (gate) lay.scale_canvas(kInner); lay.pad_canvas(lay.target); }
        else if (gate) { lay.scale_canvas(kInner); lay.pad_canvas(lay.target); }
    } else if (fit == kIr4Stretch) {
        if (gate) lay.distort_canvas(lay.target);
        if (scale == kIr4Canvas) lay.pad_canvas(lay.target);
    } else if (fit == kIr4Crop) {
        if (scale == kIr4Both || (scale == kIr4Up && gate_up)) { lay.scale_canvas(kOuter); lay.crop(lay.target); }
        else if (scale == kIr4Down || scale == kIr4Canvas) {
            if (!lay.either(-1)) { lay.scale_canvas(kOuter); lay.crop(lay.target); }            // skip_if(Either(Less))
            if (lay.larger_1d_smaller_1d()) {                                                  // new_seq().skip_unless(Larger1DSmaller1D)
                if (scale == kIr4Down) lay.crop(intersection(lay.image, lay.target));          // .crop_intersection()
                else lay.virtual_canvas(lay.target);                                           // .virtual_canvas(Exact(Target))
            }
        }
    } else {
        lay.crop(box_of(lay.target, lay.canvas, kInner));                                       // CropAspect (sizing.rs:419)
    }
}

int32_t align1d(const Anchor1D& a, int32_t inner, int32_t outer) {                             // Ir4Layout::align1d (:649-660)
    if ((outer < inner && inner < 1) || outer < 1) throw LayoutErr{"Outer box should never be smaller than inner box. All values must > 0"};
    switch (a.kind) {
    case Anchor1D::kNear: return 0;
    case Anchor1D::kCenter: return (outer - inner) / 2;
    case Anchor1D::kFar: return outer - inner;
    default: return gravity1d(a.percent, inner, outer);
    }
}

// get_wh_from_all (:63-91): 0 stands for None
void wh_from_all(const Ir4LayoutParams& i, const AR& source, int32_t* ow, int32_t* oh) {
    int32_t w = std::max(i.w.some ? i.w.v : -1, -1), h = std::max(i.h.some ? i.h.v : -1, -1);
    int32_t mw = std::max(i.legacy_max_width.some ? i.legacy_max_width.v : -1, -1), mh = std::max(i.legacy_max_height.some ? i.legacy_max_height.v : -1, -1);
    if (mw > 0 && w > 0) { w = std::min(mw, w); mw = -1; }
    if (mh > 0 && h > 0) { h = std::min(mh, h); mh = -1; }
    if (w != -1 && mh != -1) mh = std::min(mh, proportional(source, w, true, nullptr));
    if (h != -1 && mw != -1) mw = std::min(mw, proportional(source, h, false, nullptr));
    w = std::max(w, mw); h = std::max(h, mh);
    *ow = w < 1 ? 0 : w; *oh = h < 1 ? 0 : h;
}

// get_ideal_target_size (:93-131)
AR ideal_target_size(const Ir4LayoutParams& i, const AR& source, double preshrink_ratio) {
    const int32_t unshrunk_w = as_i32(static_cast<double>(source.w) / preshrink_ratio), unshrunk_h = as_i32(static_cast<double>(source.h) / preshrink_ratio);
    int32_t w, h;
    wh_from_all(i, source, &w, &h);
    if (!w && !h) { w = unshrunk_w; h = unshrunk_h; }
    else if (!h) h = proportional(source, w, true, nullptr);
    else if (!w) w = proportional(source, h, false, nullptr);
    // float_min / float_max (:133-158) of comparable values: the parser lets only a finite zoom through
    double zoom = i.zoom.some ? static_cast<double>(i.zoom.v) : 1.0;
    if (!std::isfinite(zoom)) zoom = 80000.0;
    zoom = std::max(0.00008, std::min(zoom, 80000.0));
    auto side = [&](int32_t v) { return as_i32(std::max(1.0, std::min(std::round(static_cast<double>(v) * zoom), 2147483647.0))); };
    return create(side(w), side(h));
}

}  // namespace

int constraint_mode_from_name(const std::string& n) {
    static const char* const names[] = {"distort", "within", "fit", "larger_than", "within_crop", "fit_crop", "aspect_crop", "within_pad", "fit_pad"};
    for (int i = 0; i < 9; ++i)
        if (n == names[i]) return i;
    return -1;
}

bool process_constraint(int mode, int32_t source_w, int32_t source_h, int64_t w, int64_t h, bool has_gravity, float gx, float gy,
                        ConstraintLayout* out, std::string* error) {
    try {
        const AR initial = create(source_w, source_h);
        // get_wh_from_all (:62-91) without the legacy max values; get_ideal_target_size (:93-139) at zoom 1, pre-shrink ratio 1
        const bool some_w = w >= 1 && w <= 2147483647, some_h = h >= 1 && h <= 2147483647;
        AR target = initial;
        if (some_w && some_h) target = create(w, h);
        else if (some_w) target = create(w, proportional(initial, static_cast<int32_t>(w), true, nullptr));
        else if (some_h) target = create(proportional(initial, static_cast<int32_t>(h), false, nullptr), h);
        // build_constraints (:160-283): both sides ABSENT (not merely < 1) forces FitMode::Max
        int fit, scale = kIr4Down;
        switch (mode) {                                                                        // get_instructions (:290-332)
        case kDistort: fit = kIr4Stretch; scale = kIr4Both; break;
        case kWithin: fit = kIr4Max; scale = kIr4Down; break;
        case kFit: fit = kIr4Max; scale = kIr4Both; break;
        case kLargerThan: fit = kIr4Max; scale = kIr4Up; break;
        case kWithinCrop: fit = kIr4Crop; scale = kIr4Down; break;
        case kFitCrop: fit = kIr4Crop; scale = kIr4Both; break;
        case kAspectCrop: fit = kIr4AspectCrop; scale = kIr4Down; break;
        case kWithinPad: fit = kIr4Pad; scale = kIr4Down; break;
        case kFitPad: fit = kIr4Pad; scale = kIr4Both; break;
        default: throw LayoutErr{"NotImplemented"};
        }
        if (w < 0 && h < 0) fit = kIr4Max;
        Layout lay{initial, target, initial, initial};                                         // Layout::create (:452-454)
        run_constraints(lay, fit, scale);
        // results (:359-411)
        const float x = has_gravity ? gx : 50.f, y = has_gravity ? gy : 50.f;
        const AR new_crop = lay.source;
        const int32_t cx1 = gravity1d(x, new_crop.w, initial.w), cy1 = gravity1d(y, new_crop.h, initial.h);
        ConstraintLayout r;
        if (cx1 > 0 || cy1 > 0 || initial.w != new_crop.w || initial.h != new_crop.h) {
            r.has_crop = true;
            r.crop[0] = static_cast<uint32_t>(cx1); r.crop[1] = static_cast<uint32_t>(cy1);
            r.crop[2] = static_cast<uint32_t>(cx1 + new_crop.w); r.crop[3] = static_cast<uint32_t>(cy1 + new_crop.h);
        }
        r.scale_w = lay.image.w; r.scale_h = lay.image.h;
        r.canvas_w = lay.canvas.w; r.canvas_h = lay.canvas.h;
        const int32_t left = gravity1d(x, lay.image.w, lay.canvas.w), top = gravity1d(y, lay.image.h, lay.canvas.h);
        const int32_t right = lay.canvas.w - lay.image.w - left, bottom = lay.canvas.h - lay.image.h - top;
        if (left > 0 || top > 0 || right > 0 || bottom > 0) {
            if (left < 0 || top < 0 || right < 0 || bottom < 0) throw LayoutErr{"Negative padding showed up"};
            r.has_pad = true;
            r.pad[0] = static_cast<uint32_t>(left); r.pad[1] = static_cast<uint32_t>(top);
            r.pad[2] = static_cast<uint32_t>(right); r.pad[3] = static_cast<uint32_t>(bottom);
        }
        *out = r;
        return true;
    } catch (const LayoutErr& e) {
        if (error) *error = e.text;
        return false;
    }
}

bool ir4_align(const Anchor1D& x, const Anchor1D& y, int32_t inner_w, int32_t inner_h, int32_t outer_w, int32_t outer_h, int32_t* left, int32_t* top) {
    try {
        *left = align1d(x, inner_w, outer_w);
        *top = align1d(y, inner_h, outer_h);
        return true;
    } catch (const LayoutErr&) {
        return false;
    }
}

bool ir4_crop_and_layout(const Ir4LayoutParams& i, int32_t w, int32_t h, int32_t reference_w, int32_t reference_h, Ir4LayoutResult* out,
                         std::string* error) {
    try {
        // get_precrop / get_precrop_reference (:47-61): srotate by a quarter turn swaps the sides
        const bool swap = (((i.srotate.some ? i.srotate.v : 0) / 90 + 4) % 2) != 0;
        const int32_t pw = swap ? h : w, ph = swap ? w : h, ref_w = swap ? reference_h : reference_w, ref_h = swap ? reference_w : reference_h;
        // get_initial_copy_window_floats (:729-775) against the reference size
        double fl[4] = {0, 0, static_cast<double>(ref_w), static_cast<double>(ref_h)};
        if (i.has_crop) {
            const double xunits = i.cropxunits.some && i.cropxunits.v != 0.0 ? i.cropxunits.v : static_cast<double>(ref_w);
            const double yunits = i.cropyunits.some && i.cropyunits.v != 0.0 ? i.cropyunits.v : static_cast<double>(ref_h);
            double v4[4];
            for (int ix = 0; ix < 4; ++ix) {
                const double relative_to = ix % 2 == 0 ? xunits : yunits, max_dimension = static_cast<double>(ix % 2 == 0 ? ref_w : ref_h);
                double v = i.crop[ix] * max_dimension / relative_to;
                if ((ix < 2 && v < 0.0) || (ix > 1 && v <= 0.0)) v += max_dimension;           // negative offsets from the far edge
                if (v < 0.0) v = 0.0;
                if (v > max_dimension) v = max_dimension;
                v4[ix] = v;
            }
            if (!(std::round(v4[3]) <= std::round(v4[1]) || std::round(v4[2]) <= std::round(v4[0])))
                for (int ix = 0; ix < 4; ++ix) fl[ix] = v4[ix];
        }
        // get_initial_copy_window (:700-725): re-scaled to the decoded size, rounded, clamped; the whole frame when x2 <= x1
        if (ref_w != pw || ref_h != ph) {
            fl[0] = fl[0] * static_cast<double>(pw) / static_cast<double>(ref_w); fl[2] = fl[2] * static_cast<double>(pw) / static_cast<double>(ref_w);
            fl[1] = fl[1] * static_cast<double>(ph) / static_cast<double>(ref_h); fl[3] = fl[3] * static_cast<double>(ph) / static_cast<double>(ref_h);
        }
        int32_t win[4];
        for (int ix = 0; ix < 4; ++ix) win[ix] = std::max<int32_t>(0, std::min<int32_t>(as_i32(std::round(fl[ix])), ix % 2 == 0 ? pw : ph));
        if (win[3] <= win[1] || win[2] <= win[0]) { win[0] = 0; win[1] = 0; win[2] = pw; win[3] = ph; }
        const AR initial = create(static_cast<int64_t>(win[2]) - win[0], static_cast<int64_t>(win[3]) - win[1]);
        const AR target = ideal_target_size(i, initial, static_cast<double>(w) / static_cast<double>(reference_w));   // get_preshrink_ratio (:43-45)
        const int fit = !i.w.some && !i.h.some ? kIr4Max : i.mode == kIr4FitUnset ? kIr4Pad : i.mode;                    // build_constraints (:164-168)
        Layout lay{initial, target, initial, initial};
        run_constraints(lay, fit, i.scale == kIr4ScaleUnset ? kIr4Down : i.scale);
        const AR new_crop = lay.source;
        // c.gravity before anchor, centre otherwise (:441-449)
        Anchor1D ax, ay;
        if (i.has_c_gravity) { ax.kind = ay.kind = Anchor1D::kPercent; ax.percent = static_cast<float>(i.c_gravity[0]); ay.percent = static_cast<float>(i.c_gravity[1]); }
        else if (i.has_anchor) { ax = i.anchor_x; ay = i.anchor_y; }
        const int64_t x1 = static_cast<int64_t>(win[0]) + align1d(ax, new_crop.w, initial.w), y1 = static_cast<int64_t>(win[1]) + align1d(ay, new_crop.h, initial.h);
        Ir4LayoutResult r;
        if (x1 > 0 || y1 > 0 || pw != new_crop.w || ph != new_crop.h) {                                                 // :455-468
            r.has_crop = true;
            r.crop[0] = static_cast<uint32_t>(x1); r.crop[1] = static_cast<uint32_t>(y1);
            r.crop[2] = static_cast<uint32_t>(x1 + new_crop.w); r.crop[3] = static_cast<uint32_t>(y1 + new_crop.h);
        }
        r.source_w = new_crop.w; r.source_h = new_crop.h;
        r.image_w = lay.image.w; r.image_h = lay.image.h;
        r.canvas_w = lay.canvas.w; r.canvas_h = lay.canvas.h;
        *out = r;
        return true;
    } catch (const LayoutErr& e) {
        if (error) *error = e.text;
        return false;
    }
}

}  // namespace ifhip
