// encoder_select.cpp -- see encoder_select.hpp.  The reference's logic is restated with its lines cited; the arithmetic of the
// quality tables is in `float`, in the reference's order of operations and without FMA contraction: the results are
// truncated to u8, and one ulp changes a quality.
#include "encoder_select.hpp"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/imageflow_hip_encoder_select.h"
#include "common.hpp"

#pragma clang fp contract(off)

namespace ifsel {
namespace {

using ifshim::JVal;
using ifshim::kArgumentInvalid;
using ifshim::kInvalidJson;
using ifshim::raise;

// ---- the tables (auto.rs:587-621) --------------------------------------------------------------------------------------------
//                                        p      ssim2  moz    jpegli webp   avif   jxl   webp_m avif_s jxl_e png png_max png_s
constexpr QualityHints kAbsoluteLowest = {0.f,   0.f,   0.f,   0.f,   0.f,   0.f,   25.f,  5,     6,     6,    0,  4,      4};
constexpr QualityHints kQualityHints[8] = {
    {15.f,  10.f,  15.f,  15.f,  15.f,  23.f,  13.f,  6, 6, 5, 0,   10,  4},     // lowest
    {20.f,  30.f,  20.f,  20.f,  20.f,  34.f,  7.4f,  6, 6, 6, 0,   20,  4},     // low
    {34.f,  50.f,  34.f,  34.f,  34.f,  45.f,  4.3f,  6, 6, 5, 0,   35,  4},     // mediumlow
    {55.f,  60.f,  57.f,  52.f,  53.f,  44.f,  3.92f, 5, 6, 5, 0,   55,  4},     // medium
    {73.f,  70.f,  73.f,  73.f,  76.f,  55.f,  2.58f, 6, 6, 5, 50,  100, 4},     // good
    {91.f,  85.f,  91.f,  91.f,  93.f,  66.f,  1.0f,  5, 6, 5, 80,  100, 4},     // high
    {96.f,  90.f,  96.f,  96.f,  96.f,  100.f, 0.5f,  5, 6, 0, 90,  100, 4},     // highest
    {100.f, 100.f, 100.f, 100.f, 100.f, 100.f, 0.0f,  6, 5, 6, 100, 100, 4}};    // lossless

float clampf(float v, float lo, float hi) { return v < lo ? lo : v > hi ? hi : v; }                 // f32::clamp (a NaN stays)
uint8_t as_u8(float v) { return v != v ? 0 : v <= 0.f ? 0 : v >= 255.f ? 255 : static_cast<uint8_t>(v); }   // Rust's saturating `as u8`
// interpolate_value (auto.rs:696-702) WITHOUT its guard: the reference panics when b - a <= 0, which is every interpolated
// profile outside 55 < p < 73 (png 0 -> 0 below 55, avif 45 -> 44 in (34, 55), png_max 100 -> 100 above 73, avif 100 -> 100
// above 96); this build evaluates the same expression (DESIGN "Encoder selection").
float interpolate_value(float ratio, float a, float b) { return a + ratio * (b - a); }
QualityHints interpolate(float ratio, float percent, const QualityHints& lower, const QualityHints& higher) {   // auto.rs:743-764, 785-802
    QualityHints h = higher;                           // png_s, jxl_e, webp_m, avif_s: the higher row's
    h.p = percent;
    h.ssim2 = interpolate_value(ratio, lower.ssim2, higher.ssim2);
    h.moz = interpolate_value(ratio, lower.moz, higher.moz);
    h.jpegli = interpolate_value(ratio, lower.jpegli, higher.jpegli);
    h.webp = interpolate_value(ratio, lower.webp, higher.webp);
    h.avif = interpolate_value(ratio, lower.avif, higher.avif);
    h.jxl = interpolate_value(ratio, higher.jxl, lower.jxl);                                        // distance is inverse
    h.png = as_u8(clampf(interpolate_value(ratio, static_cast<float>(lower.png), static_cast<float>(higher.png)), 0.f, 100.f));
    h.png_max = as_u8(clampf(interpolate_value(ratio, static_cast<float>(lower.png_max), static_cast<float>(higher.png_max)), 0.f, 100.f));
    return h;
}

// ---- serde's readers (imageflow_types/src/lib.rs:270-775) ---------------------------------------------------------------
const JVal* field(const JVal& o, const char* key) {                                                 // an Option field: missing and null are None
    const JVal* v = o.get(key);
    return v && !v->is_null() ? v : nullptr;
}
const JVal& want_object(const JVal& v, const char* what) {
    if (v.t != JVal::Obj) raise(kInvalidJson, "InvalidJson: %s is an object", what);
    return v;
}
float to_f32(double n) { return n > FLT_MAX ? INFINITY : n < -FLT_MAX ? -INFINITY : static_cast<float>(n); }
void read_f32(const JVal& o, const char* key, const char* what, Opt<float>* out) {
    if (const JVal* v = field(o, key)) {
        if (v->t != JVal::Num) raise(kInvalidJson, "InvalidJson: %s.%s is a number", what, key);
        out->set(to_f32(v->n));
    }
}
void read_bool(const JVal& o, const char* key, const char* what, Opt<bool>* out) {
    if (const JVal* v = field(o, key)) {
        if (v->t != JVal::Bool) raise(kInvalidJson, "InvalidJson: %s.%s is a boolean", what, key);
        out->set(v->b);
    }
}
int read_name(const JVal& o, const char* key, const char* what, const char* const* names, int n, int none) {
    const JVal* v = field(o, key);
    if (!v) return none;
    if (v->t == JVal::Str) for (int k = 0; k < n; ++k) if (v->s == names[k]) return k;
    raise(kInvalidJson, "InvalidJson: %s.%s: unknown variant", what, key);
}
const char* const kBoolKeepNames[] = {"keep", "true", "false"};
const char* const kFormatNames[] = {"webp", "jpeg", "jpg", "png", "avif", "jxl", "gif", "keep"};
const char* const kProfileNames[] = {"lowest", "low", "mediumlow", "medium", "good", "high", "highest", "lossless"};
const char* const kJpegStyleNames[] = {"jpegli", "libjpegturbo", "mozjpeg", "default"};
const char* const kPngStyleNames[] = {"libpng", "lodepng", "pngquant", "default"};

QualityProfile read_profile(const JVal& o, const char* what, bool required) {
    QualityProfile qp;
    const JVal* v = field(o, "quality_profile");
    if (!v) {
        if (required) raise(kInvalidJson, "InvalidJson: %s: missing field `quality_profile`", what);
        return qp;
    }
    if (v->t == JVal::Str) {
        for (int k = 0; k < 8; ++k) if (v->s == kProfileNames[k]) qp.kind = k;
    } else if (v->t == JVal::Obj && v->o.size() == 1 && v->o[0].first == "percent" && v->o[0].second.t == JVal::Num) {
        qp.kind = kPercent;
        qp.percent = to_f32(v->o[0].second.n);
    }
    if (qp.kind == kQpNone) raise(kInvalidJson, "InvalidJson: %s.quality_profile is a profile's lowercase name or {\"percent\": number}", what);
    return qp;
}
AllowedFormats read_allow(const JVal& v) {
    want_object(v, "allow");
    AllowedFormats a;
    const struct { const char* key; int8_t* slot; } fields[] = {
        {"webp", &a.webp}, {"jxl", &a.jxl}, {"avif", &a.avif}, {"jpeg", &a.jpeg}, {"jpeg_progressive", &a.jpeg_progressive}, {"jpeg_xyb", &a.jpeg_xyb},
        {"png", &a.png}, {"gif", &a.gif}, {"all", &a.all}, {"web_safe", &a.web_safe}, {"modern_web_safe", &a.modern_web_safe}, {"color_profiles", &a.color_profiles}};
    for (const auto& f : fields) {
        Opt<bool> b;
        read_bool(v, f.key, "allow", &b);
        if (b.some) *f.slot = b.v ? 1 : 0;
    }
    return a;
}
EncoderHints read_hints(const JVal& v) {
    want_object(v, "encoder_hints");
    EncoderHints h;
    if (const JVal* j = field(v, "jpeg")) {
        want_object(*j, "encoder_hints.jpeg");
        h.has_jpeg = true;
        read_f32(*j, "quality", "encoder_hints.jpeg", &h.jpeg_quality);
        read_bool(*j, "progressive", "encoder_hints.jpeg", &h.jpeg_progressive);
        h.jpeg_mimic = read_name(*j, "mimic", "encoder_hints.jpeg", kJpegStyleNames, 4, kJpegStyleNone);
    }
    if (const JVal* p = field(v, "png")) {
        want_object(*p, "encoder_hints.png");
        h.has_png = true;
        read_f32(*p, "quality", "encoder_hints.png", &h.png_quality);
        read_f32(*p, "min_quality", "encoder_hints.png", &h.png_min_quality);
        if (const JVal* s = field(*p, "quantization_speed")) {
            if (s->t != JVal::Num || s->n != std::floor(s->n) || s->n < 0.0 || s->n > 255.0) raise(kInvalidJson, "InvalidJson: encoder_hints.png.quantization_speed is an integer 0..255");
            h.png_quantization_speed.set(static_cast<uint8_t>(s->n));
        }
        h.png_mimic = read_name(*p, "mimic", "encoder_hints.png", kPngStyleNames, 4, kPngStyleNone);
        read_bool(*p, "hint_max_deflate", "encoder_hints.png", &h.png_hint_max_deflate);
        h.png_lossless = read_name(*p, "lossless", "encoder_hints.png", kBoolKeepNames, 3, kBkNone);
    }
    if (const JVal* w = field(v, "webp")) {
        want_object(*w, "encoder_hints.webp");
        h.has_webp = true;
        read_f32(*w, "quality", "encoder_hints.webp", &h.webp_quality);
        h.webp_lossless = read_name(*w, "lossless", "encoder_hints.webp", kBoolKeepNames, 3, kBkNone);
    }
    if (const JVal* g = field(v, "gif")) { want_object(*g, "encoder_hints.gif"); h.has_gif = true; }
    return h;
}

// ---- AllowedFormats (lib.rs:443-560) ----------------------------------------------------------------------------------------
int8_t or_(int8_t a, int8_t b) { return a < 0 ? b : b < 0 ? a : static_cast<int8_t>(a || b); }
AllowedFormats web_safe() { AllowedFormats a; a.jpeg = a.png = a.gif = a.web_safe = 1; return a; }
AllowedFormats modern_web_safe() { AllowedFormats a = web_safe(); a.webp = a.modern_web_safe = a.color_profiles = a.jpeg_progressive = a.jpeg_xyb = 1; return a; }
AllowedFormats all_formats() { AllowedFormats a; a.webp = a.jxl = a.avif = a.jpeg = a.jpeg_progressive = a.jpeg_xyb = a.png = a.gif = a.all = a.web_safe = a.modern_web_safe = a.color_profiles = 1; return a; }
AllowedFormats merge(const AllowedFormats& s, const AllowedFormats& o) {
    AllowedFormats a;
    a.webp = or_(s.webp, o.webp); a.jxl = or_(s.jxl, o.jxl); a.avif = or_(s.avif, o.avif); a.jpeg = or_(s.jpeg, o.jpeg);
    a.jpeg_xyb = or_(s.jpeg_xyb, o.jpeg_xyb); a.jpeg_progressive = or_(s.jpeg_progressive, o.jpeg_progressive); a.png = or_(s.png, o.png);
    a.gif = or_(s.gif, o.gif); a.all = or_(s.all, o.all); a.web_safe = or_(s.web_safe, o.web_safe);
    a.modern_web_safe = or_(s.modern_web_safe, o.modern_web_safe); a.color_profiles = or_(s.color_profiles, o.color_profiles);
    return a;
}
AllowedFormats expand_sets(const AllowedFormats& a) {
    if (a.all == 1) return all_formats();
    if (a.web_safe == 1) return merge(a, web_safe());
    if (a.modern_web_safe == 1) return merge(a, modern_web_safe());
    return a;
}
bool any_formats_enabled(const AllowedFormats& a) { return a.webp == 1 || a.jxl == 1 || a.avif == 1 || a.jpeg == 1 || a.png == 1 || a.gif == 1; }

// ---- build_auto_encoder_details (auto.rs:1042-1111) -----------------------------------------------------------------------
struct Details {
    int format;
    bool needs_animation, needs_alpha;
    int needs_lossless;                                // Option<bool>: -1 None
    AllowedFormats allow;
    bool has_source, source_lossless;
};
Details details_of(const Preset& p, const Source& src, bool alpha_meaningful) {
    Details d;
    const bool matte_is_opaque = p.has_matte && (p.matte >> 24) == 0xFFu;                           // :1057
    d.has_source = src.kind != kSourceNone;
    d.source_lossless = d.has_source && src.lossless;
    d.needs_alpha = alpha_meaningful && !matte_is_opaque;                                           // :1072
    d.needs_animation = d.has_source && src.animated;                                               // :1079
    const int source_format = src.kind == kSourceJpeg ? kJpeg : src.kind == kSourcePng ? kPng : src.kind == kSourceGif ? kGif : src.kind == kSourceWebp ? kWebp : kFormatNone;
    d.format = p.is_auto ? kFormatNone : p.format == kKeep ? source_format : p.format;              // :1082-1085: keep without a source is auto
    d.needs_lossless = p.lossless == kBkKeep ? (d.has_source ? (d.source_lossless ? 1 : 0) : (d.needs_alpha ? 1 : 0))   // :1087-1094
                       : p.lossless == kBkTrue ? 1 : p.lossless == kBkFalse ? 0 : -1;
    if (p.quality_profile.kind == kLossless) d.needs_lossless = 1;                                  // :1095-1097
    d.allow = p.has_allow ? expand_sets(p.allow) : web_safe();                                      // :1113-1118
    return d;
}
// format_auto_select (auto.rs:1136-1242) with no jxl, avif, animated webp or jpegli: the branches that need one are gone, and
// with them the pixel count's only use (:1202)
int format_auto_select(const Preset& p, const Details& d) {
    const AllowedFormats& allowed = d.allow;
    if (!any_formats_enabled(allowed)) return kFormatNone;
    if (d.needs_animation) return kGif;                                                             // :1154-1159
    if (d.needs_lossless == 1 || d.needs_alpha) {                                                   // :1179-1191
        if (allowed.webp == 1) return kWebp;
        if (allowed.png == 1) return kPng;
    }
    const float approx_quality = approximate_quality_profile(p.quality_profile);                    // :1214-1221
    if ((approx_quality > 90.0f || allowed.jpeg_progressive != 1) && allowed.webp == 1) return kWebp;
    if (allowed.jpeg == 1) return kJpeg;
    if (allowed.png == 1) return kPng;
    if (allowed.gif == 1) return kGif;
    return kFormatNone;
}
int final_format_of(const Preset& p, const Details& d) {                                            // create_encoder_auto (:375-388)
    int f = d.format;
    if (f == kFormatNone) {
        f = format_auto_select(p, d);
        if (f == kFormatNone) raise(kArgumentInvalid, "InvalidArgument: No formats enabled; try 'allow': { 'web_safe':true}");
    }
    if (f == kJxl || f == kAvif) { f = format_auto_select(p, d); if (f == kFormatNone) f = kJpeg; }
    return f == kJpg ? kJpeg : f;
}

std::string num(double v) { char buf[40]; std::snprintf(buf, sizeof buf, "%.17g", v); return buf; }
std::string opt_int(int v) { return v < 0 ? "null" : std::to_string(v); }
std::string opt_bool(int v) { return v < 0 ? "null" : v ? "true" : "false"; }

}  // namespace

QualityHints get_quality_hints(const QualityProfile& qp) {
    if (qp.kind != kPercent) return kQualityHints[qp.kind];                                         // :766-768
    const float percent = clampf(qp.percent, 0.0f, 100.0f);
    const QualityHints* higher = &kQualityHints[7];
    for (int k = 7; k >= 0; --k) if (kQualityHints[k].p >= percent) higher = &kQualityHints[k];     // the first row at or above
    if (higher->p == percent) return *higher;
    const QualityHints* lower = &kAbsoluteLowest;
    for (int k = 0; k < 8; ++k) if (kQualityHints[k].p < percent) lower = &kQualityHints[k];        // the last row below
    const float ratio = (percent - lower->p) / (higher->p - lower->p);
    return interpolate(ratio, percent, *lower, *higher);
}
QualityHints get_quality_hints_by_ssim2(float ssim2) {
    const float percent = clampf(ssim2, 0.0f, 100.0f);
    const QualityHints* higher = &kQualityHints[7];
    for (int k = 7; k >= 0; --k) if (kQualityHints[k].ssim2 >= percent) higher = &kQualityHints[k];
    if (higher->ssim2 == percent) return *higher;
    const QualityHints* lower = &kAbsoluteLowest;
    for (int k = 0; k < 8; ++k) if (kQualityHints[k].ssim2 < percent) lower = &kQualityHints[k];
    const float ratio = (percent - lower->p) / (higher->p - lower->p);                              // sic (:784): from p, not from ssim2
    return interpolate(ratio, percent, *lower, *higher);
}
QualityHints get_quality_hints_with_dpr(const QualityProfile& qp, const Opt<float>& dpr) {
    const QualityHints hints = get_quality_hints(qp);
    if (!dpr.some || dpr.v == 3.0f) return hints;
    const float quality_factor = 3.0f / clampf(dpr.v, 0.1f, 12.0f);                                 // :717
    const float target_ssim2 = clampf(hints.ssim2 * quality_factor, 10.0f, 90.0f);                  // :721
    return get_quality_hints_by_ssim2(target_ssim2);
}
float approximate_quality_profile(const QualityProfile& qp) { return qp.kind == kQpNone ? 90.0f : get_quality_hints(qp).p; }

bool names_selection(const JVal* preset) { return preset && preset->t == JVal::Obj && (preset->get("auto") || preset->get("format")); }

Preset read_preset(const JVal& preset) {
    Preset p;
    const JVal* body = preset.get("auto");
    p.is_auto = body != nullptr;
    if (!body) body = preset.get("format");
    const char* what = p.is_auto ? "encode.preset.auto" : "encode.preset.format";
    if (!body || preset.o.size() != 1) raise(kInvalidJson, "InvalidJson: encode.preset is {\"auto\": {..}} or {\"format\": {..}}");
    want_object(*body, what);
    if (!p.is_auto) {
        p.format = read_name(*body, "format", what, kFormatNames, 8, kFormatNone);
        if (p.format == kFormatNone) raise(kInvalidJson, "InvalidJson: %s: missing field `format`", what);
    }
    p.quality_profile = read_profile(*body, what, p.is_auto);
    read_f32(*body, "quality_profile_dpr", what, &p.quality_profile_dpr);
    if (const JVal* m = field(*body, "matte")) {
        p.has_matte = true;
        p.matte = ifshim::parse_color(m, p.is_auto ? "encode.preset.auto.matte" : "encode.preset.format.matte");
        ifshim::to_json(*m, &p.matte_json);
    }
    p.lossless = read_name(*body, "lossless", what, kBoolKeepNames, 3, kBkNone);
    if (const JVal* a = field(*body, "allow")) { p.has_allow = true; p.allow = read_allow(*a); }
    if (!p.is_auto) if (const JVal* h = field(*body, "encoder_hints")) { p.has_hints = true; p.hints = read_hints(*h); }
    return p;
}

bool resolves_to_gif_without_frame(const Preset& p, const Source& src) {
    const Details d = details_of(p, src, false);
    if (d.format == kGif) return true;                                                              // `format: gif`, `keep` on a GIF source
    return d.format == kFormatNone && any_formats_enabled(d.allow) && d.needs_animation;            // auto-selection on an animated source (:1154-1159)
}

Resolved resolve(const Preset& p, const Source& src, bool alpha_meaningful, uint32_t w, uint32_t h) {
    (void)w; (void)h;                                                                               // final_pixel_count: read by the avif branch alone (:1202)
    const Details d = details_of(p, src, alpha_meaningful);
    Resolved r;
    r.format = final_format_of(p, d);
    r.has_matte = p.has_matte; r.matte = p.matte; r.matte_json = p.matte_json;
    const bool has_profile = p.quality_profile.kind != kQpNone;
    const QualityHints profile = has_profile ? get_quality_hints_with_dpr(p.quality_profile, p.quality_profile_dpr) : kAbsoluteLowest;
    const EncoderHints& eh = p.hints;                                                               // (all None without encoder_hints)
    if (r.format == kGif) { r.coder = kCoderGif; return r; }
    if (r.format == kJpeg) {                                                                        // create_jpeg_auto (:806-874)
        r.progressive = eh.jpeg_progressive.some ? eh.jpeg_progressive.v : true;
        if (d.allow.jpeg_progressive != 1) r.progressive = false;
        const float q = has_profile ? profile.moz : eh.jpeg_quality.some ? eh.jpeg_quality.v : 90.0f;
        r.quality = as_u8(clampf(q, 0.0f, 100.0f));
        if (eh.jpeg_mimic == kLibjpegTurbo) { r.coder = kCoderLibjpegTurbo; r.optimize_huffman_coding = r.progressive; }
        else r.coder = kCoderMozjpeg;                                                               // Default | Mozjpeg | Jpegli
        return r;
    }
    if (r.format == kWebp) {                                                                        // create_webp_auto (:876-912)
        const int manual_lossless = eh.webp_lossless == kBkKeep ? (d.has_source && d.source_lossless ? 1 : 0) : eh.webp_lossless == kBkTrue ? 1 : eh.webp_lossless == kBkFalse ? 0 : -1;
        const float manual_quality = clampf(eh.webp_quality.some ? eh.webp_quality.v : 80.0f, 0.0f, 100.0f);
        const int lossless = d.needs_lossless >= 0 ? d.needs_lossless : manual_lossless >= 0 ? manual_lossless : 0;
        if (lossless) { r.coder = kCoderWebpLossless; return r; }
        r.coder = kCoderWebpLossy;
        r.webp_quality = has_profile ? profile.webp : manual_quality;
        return r;
    }
    // create_png_auto (:914-1025)
    const bool libpng = eh.png_mimic == kLibpng;
    bool lossless;
    if (d.needs_lossless == 1) lossless = true;                                                     // :931-941
    else if (eh.png_lossless == kBkKeep) lossless = d.has_source && d.source_lossless;
    else if (eh.png_lossless == kBkTrue) lossless = true;
    else if (eh.png_lossless == kBkFalse) lossless = false;
    else if (d.needs_lossless == 0) lossless = false;
    else lossless = !eh.png_quality.some || libpng;
    r.maximum_deflate = eh.png_hint_max_deflate.some ? (eh.png_hint_max_deflate.v ? 1 : 0) : -1;
    if (has_profile) {                                                                              // :945-964
        if (profile.png == 100 || lossless) { r.coder = kCoderLodepng; return r; }
        r.coder = kCoderPngquant;
        r.speed = profile.png_s; r.quality = profile.png_max; r.minimum_quality = profile.png;
        return r;
    }
    if (libpng) {                                                                                   // :967-986
        r.coder = kCoderLibpng;
        r.png_32 = d.needs_alpha;
        r.zlib_9 = r.maximum_deflate == 1;
        return r;
    }
    // :995-1015 `PngEncoderStyle::Pngquant | PngEncoderStyle::Default if !lossless`; `mimic: lodepng` falls to the last arm (:1016-1022)
    if (!lossless && eh.png_mimic != kLodepng) {
        r.coder = kCoderPngquant;
        if (eh.png_quality.some) r.quality = as_u8(clampf(eh.png_quality.v, 0.0f, 100.0f));
        if (eh.png_min_quality.some) r.minimum_quality = as_u8(clampf(eh.png_min_quality.v, 0.0f, 100.0f));
        if (eh.png_quantization_speed.some) r.speed = eh.png_quantization_speed.v < 1 ? 1 : eh.png_quantization_speed.v > 10 ? 10 : eh.png_quantization_speed.v;
        return r;
    }
    r.coder = kCoderLodepng;
    return r;
}

const char* coder_name(int coder) {
    static const char* const names[] = {"mozjpeg", "libjpeg_turbo", "lodepng", "pngquant", "libpng", "webp_lossy", "webp_lossless", "gif"};
    return names[coder];
}

std::string resolved_json(const Resolved& r) {
    const std::string matte = r.has_matte ? r.matte_json : "null";
    std::string params;
    switch (r.coder) {
    case kCoderMozjpeg: params = "{\"quality\":" + opt_int(r.quality) + ",\"progressive\":" + opt_bool(r.progressive) + ",\"matte\":" + matte + "}"; break;
    case kCoderLibjpegTurbo:
        params = "{\"quality\":" + opt_int(r.quality) + ",\"progressive\":" + opt_bool(r.progressive) + ",\"optimize_huffman_coding\":" + opt_bool(r.optimize_huffman_coding) + ",\"matte\":" + matte + "}";
        break;
    case kCoderLodepng: params = "{\"maximum_deflate\":" + opt_bool(r.maximum_deflate) + "}"; break;
    case kCoderPngquant:
        params = "{\"quality\":" + opt_int(r.quality) + ",\"minimum_quality\":" + opt_int(r.minimum_quality) + ",\"speed\":" + opt_int(r.speed) + ",\"maximum_deflate\":" + opt_bool(r.maximum_deflate) + "}";
        break;
    case kCoderLibpng: params = std::string("{\"depth\":\"") + (r.png_32 ? "png_32" : "png_24") + "\",\"matte\":" + matte + ",\"zlib_compression\":" + (r.zlib_9 ? "9" : "null") + "}"; break;
    case kCoderWebpLossy: params = "{\"quality\":" + num(static_cast<double>(r.webp_quality)) + "}"; break;
    default: params = "{}"; break;
    }
    const char* format = r.format == kJpeg ? "jpeg" : r.format == kPng ? "png" : r.format == kWebp ? "webp" : "gif";
    return std::string("{\"format\":\"") + format + "\",\"coder\":\"" + coder_name(r.coder) + "\",\"params\":" + params + ",\"matte\":" + matte + "}";
}

std::string preset_json_of(const ifhip::Ir4Output& o) {
    using O = ifhip::Ir4Output;
    auto f32 = [](float v) { return std::isfinite(v) ? num(static_cast<double>(v)) : std::string("null"); };   // (serde_json writes a NaN as null)
    auto ob = [](const Opt<bool>& b) { return std::string(!b.some ? "null" : b.v ? "true" : "false"); };
    auto bk = [](int v) { return std::string(v == O::kBkKeep ? "\"keep\"" : v == O::kBkTrue ? "\"true\"" : v == O::kBkFalse ? "\"false\"" : "null"); };
    auto profile = [&](int kind, float percent) { return kind == O::kPercent ? "{\"percent\":" + f32(percent) + "}" : std::string("\"") + kProfileNames[kind] + "\""; };
    // read_allowed_formats (encoder.rs:5-29): web_safe, color_profiles as given (false when not), the three accept.* keys over it
    const std::string allow = "{\"webp\":" + ob(o.accept_webp) + ",\"jxl\":" + ob(o.accept_jxl) + ",\"avif\":" + ob(o.accept_avif) +
                              ",\"jpeg\":true,\"jpeg_progressive\":null,\"jpeg_xyb\":null,\"png\":true,\"gif\":true,\"all\":null,\"web_safe\":true,\"modern_web_safe\":null,\"color_profiles\":" +
                              (o.accept_color_profiles.some && o.accept_color_profiles.v ? "true" : "false") + "}";
    const int target = o.format != O::kFormatUnset ? o.format : o.qp != O::kQpUnset ? O::kAuto : O::kKeep;   // :33-37: qp makes the default auto
    const std::string dpr = o.qp_dpr.some ? f32(o.qp_dpr.v) : "null";
    if (target == O::kAuto) {                                                                       // :42-55
        const std::string qp = o.qp != O::kQpUnset ? profile(o.qp, o.qp_percent) : o.quality.some ? profile(O::kPercent, static_cast<float>(o.quality.v)) : "\"high\"";
        return "{\"auto\":{\"quality_profile\":" + qp + ",\"quality_profile_dpr\":" + dpr + ",\"matte\":null,\"lossless\":" + bk(o.lossless) + ",\"allow\":" + allow + "}}";
    }
    static const char* const formats[] = {"keep", "jpeg", "png", "gif", "webp", "avif", "jxl"};
    auto quality_or = [&](const Opt<int32_t>& first) {                                              // `v as f32`
        return first.some ? f32(static_cast<float>(first.v)) : o.quality.some ? f32(static_cast<float>(o.quality.v)) : std::string("null");
    };
    auto u8 = [](const Opt<uint8_t>& v) { return v.some ? std::to_string(static_cast<int>(v.v)) : std::string("null"); };
    // read_encoder_hints (:70-98)
    const std::string jpeg = "{\"quality\":" + quality_or(o.jpeg_quality) + ",\"progressive\":" + ob(o.jpeg_progressive) + ",\"mimic\":" +
                             (o.jpeg_li.some && o.jpeg_li.v ? "\"jpegli\"" : o.jpeg_turbo.some && o.jpeg_turbo.v ? "\"libjpegturbo\"" : "null") + "}";
    const std::string png = "{\"quality\":" + u8(o.png_quality) + ",\"min_quality\":" + u8(o.png_min_quality) + ",\"quantization_speed\":" + u8(o.png_quantization_speed) +
                            ",\"mimic\":" + (o.png_libpng.some && o.png_libpng.v ? "\"libpng\"" : "null") + ",\"hint_max_deflate\":" + ob(o.png_max_deflate) + ",\"lossless\":" + bk(o.png_lossless) + "}";
    const std::string webp = "{\"quality\":" + (o.webp_quality.some ? f32(o.webp_quality.v) : quality_or(Opt<int32_t>())) + ",\"lossless\":" + bk(o.webp_lossless) + "}";
    return std::string("{\"format\":{\"format\":\"") + formats[target] + "\",\"quality_profile\":" + (o.qp != O::kQpUnset ? profile(o.qp, o.qp_percent) : "null") +
           ",\"quality_profile_dpr\":" + dpr + ",\"matte\":null,\"lossless\":" + bk(o.lossless) + ",\"allow\":" + allow +
           ",\"encoder_hints\":{\"webp\":" + webp + ",\"jpeg\":" + jpeg + ",\"png\":" + png + ",\"gif\":{}}}}";
}

}  // namespace ifsel

namespace {
int copy_out(const std::string& json, char* out, size_t cap, size_t* needed) {
    *needed = json.size() + 1;
    if (cap >= json.size() + 1) std::memcpy(out, json.c_str(), json.size() + 1);
    return IFHIP_SELECT_OK;
}
}  // namespace

extern "C" int ifhip_shim_querystring_encoder_preset(const char* value, char* out, size_t cap, size_t* needed) {
    if (!value || !needed || (!out && cap)) return ifhip::fail(IFHIP_SELECT_INVALID, "InvalidArgument: ifhip_shim_querystring_encoder_preset needs value and needed");
    ifhip::Ir4Instructions i;
    std::string err;
    const int rc = ifhip::parse_querystring(value, &i, &err, true);
    if (rc != ifhip::kQsOk) return ifhip::fail(rc == ifhip::kQsRefused ? IFHIP_SELECT_REFUSED : IFHIP_SELECT_INVALID, "%s", err.c_str());
    return copy_out(ifsel::preset_json_of(i.out), out, cap, needed);
}

extern "C" int ifhip_shim_resolve_encoder_preset(const char* preset_json, size_t len, int source_kind, int source_lossless, uint32_t source_frames,
                                                 int alpha_meaningful, uint32_t w, uint32_t h, char* out, size_t cap, size_t* needed) {
    if (!preset_json || !needed || (!out && cap)) return ifhip::fail(IFHIP_SELECT_INVALID, "InvalidArgument: ifhip_shim_resolve_encoder_preset needs preset_json and needed");
    if (source_kind < IFHIP_SELECT_SOURCE_NONE || source_kind > IFHIP_SELECT_SOURCE_WEBP) return ifhip::fail(IFHIP_SELECT_INVALID, "InvalidArgument: source_kind is none (0), jpeg (1), png (2), gif (3) or webp (4)");
    try {
        const ifshim::JVal preset = ifshim::parse_json(reinterpret_cast<const uint8_t*>(preset_json), len);
        if (!ifsel::names_selection(&preset)) ifshim::raise(ifshim::kInvalidJson, "InvalidJson: encode.preset is {\"auto\": {..}} or {\"format\": {..}}");
        ifsel::Source src;
        src.kind = source_kind;
        src.lossless = (source_kind == IFHIP_SELECT_SOURCE_PNG || source_kind == IFHIP_SELECT_SOURCE_WEBP) && source_lossless != 0;
        src.animated = source_kind == IFHIP_SELECT_SOURCE_GIF && source_frames > 1u;
        return copy_out(ifsel::resolved_json(ifsel::resolve(ifsel::read_preset(preset), src, alpha_meaningful != 0, w, h)), out, cap, needed);
    } catch (const ifshim::FlowErr& e) {
        return ifhip::fail(e.cat == ifshim::kInvalidJson ? IFHIP_SELECT_INVALID_JSON : IFHIP_SELECT_INVALID, "%s", e.msg.c_str());
    }
}
