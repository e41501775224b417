// Constraint layout: what `constrain` and `watermark` ask imageflow_riapi for before they reach the hot path
// (flow/nodes/constrain.rs:49-52, flow/nodes/watermark.rs:134-139 -> imageflow_riapi::ir4::process_constraint).
// Host arithmetic only; restated from imageflow_riapi/src/sizing.rs and src/ir4/layout.rs (lines cited in layout.cpp).
// The same engine lays out a querystring (`command_string`): Ir4Layout::get_crop_and_layout over the parsed Instructions
// (querystring.hpp), with its own alignment rule (Ir4Layout::align).
#pragma once
#include <cstdint>
#include <string>

namespace ifhip {

enum ConstraintMode : int {            // imageflow_types ConstraintMode (lib.rs:984-1017), in its order
    kDistort = 0, kWithin, kFit, kLargerThan, kWithinCrop, kFitCrop, kAspectCrop, kWithinPad, kFitPad
};
// "distort" ... "fit_pad" -> the value above, -1 for anything else
int constraint_mode_from_name(const std::string& name);

struct ConstraintLayout {              // ir4/layout.rs ConstraintResults (:22-27)
    bool has_crop = false;
    uint32_t crop[4] = {0, 0, 0, 0};   // x1, y1, x2, y2 in the source
    int32_t scale_w = 0, scale_h = 0;  // scale_to
    bool has_pad = false;
    uint32_t pad[4] = {0, 0, 0, 0};    // left, top, right, bottom
    int32_t canvas_w = 0, canvas_h = 0;
};

// Ir4Layout::process_constraint (ir4/layout.rs:334-412).  w / h < 0: the constraint does not give that side.
// has_gravity false: ConstraintGravity::Center.  Returns false and fills *error (the Debug text of the LayoutError) when the
// reference returns Err.
bool process_constraint(int mode, int32_t source_w, int32_t source_h, int64_t w, int64_t h, bool has_gravity, float gravity_x,
                        float gravity_y, ConstraintLayout* out, std::string* error);

// ---- the querystring's layout -------------------------------------------------------------------------------------------
enum Ir4Fit : int { kIr4FitUnset = -1, kIr4Max, kIr4Pad, kIr4Crop, kIr4Stretch, kIr4AspectCrop };      // ir4/parsing.rs FitMode (:1219-1232)
enum Ir4Scale : int { kIr4ScaleUnset = -1, kIr4Down, kIr4Up, kIr4Both, kIr4Canvas };                  // ScaleMode (:1386-1397)
struct Anchor1D {                       // ir4/parsing.rs:1338-1344
    enum Kind : int { kNear, kCenter, kFar, kPercent } kind = kCenter;
    float percent = 0.f;
};
template <class T> struct Opt {         // Option<T> of a Copy type
    bool some = false;
    T v{};
    void set(const T& x) { some = true; v = x; }
};
struct Ir4LayoutParams {                // the fields of Instructions that Ir4Layout reads (ir4/parsing.rs:1236-1255)
    Opt<int32_t> w, h, legacy_max_width, legacy_max_height, srotate;
    int mode = kIr4FitUnset, scale = kIr4ScaleUnset;
    Opt<float> zoom;
    bool has_crop = false;
    double crop[4] = {0, 0, 0, 0};
    Opt<double> cropxunits, cropyunits;
    bool has_c_gravity = false;
    double c_gravity[2] = {0, 0};
    bool has_anchor = false;
    Anchor1D anchor_x, anchor_y;
};
struct Ir4LayoutResult {
    bool has_crop = false;
    uint32_t crop[4] = {0, 0, 0, 0};    // x1, y1, x2, y2 in the frame behind srotate / sflip
    int32_t source_w = 0, source_h = 0; // layout.get_source_crop(): the size of that crop
    int32_t image_w = 0, image_h = 0;   // BoxTarget::CurrentImage: what resample_2d scales to
    int32_t canvas_w = 0, canvas_h = 0; // BoxTarget::CurrentCanvas
};
// Ir4Layout::new(i, w, h, reference_width, reference_height).get_crop_and_layout() (ir4/layout.rs:414-470).  Returns false and
// fills *error where the reference returns Err -- or panics: a drop-in has no panic to offer.
bool ir4_crop_and_layout(const Ir4LayoutParams& i, int32_t w, int32_t h, int32_t reference_w, int32_t reference_h, Ir4LayoutResult* out,
                         std::string* error);
// Ir4Layout::align (ir4/layout.rs:649-671): where `inner` sits in `outer`.  Center is the integer division (outer - inner) / 2,
// not process_constraint's gravity1d(50).
bool ir4_align(const Anchor1D& x, const Anchor1D& y, int32_t inner_w, int32_t inner_h, int32_t outer_w, int32_t outer_h, int32_t* left,
               int32_t* top);

}  // namespace ifhip
