// encoder_select.hpp -- which coder an `encode` node's presets `auto` and `format` come to, as the reference decides it:
// the readers of EncoderPreset::Auto / ::Format (imageflow_types/src/lib.rs:270-775), the quality tables
// (imageflow_core/src/codecs/auto.rs:568-803), the resolution against the source file and the final frame
// (build_auto_encoder_details, format_auto_select, create_encoder_auto and create_{jpeg,webp,png}_auto, auto.rs:368-566,
// 805-1242) and the preset a querystring's output keys make (calculate_encoder_preset, imageflow_riapi/src/ir4/encoder.rs:5-98).
// Modelled on the reference built with `c-codecs` and without `zen-codecs`: FEATURES_IMPLEMENTED (auto.rs:1127-1134) is
// {jxl: false, avif: false, webp_animation: false, jpegli: false}.  Host text and arithmetic only: no device, no context.
#pragma once
#include <cstdint>
#include <string>

#include "querystring.hpp"
#include "shim_json.hpp"

namespace ifsel {

enum Format : int { kFormatNone = -1, kWebp, kJpeg, kJpg, kPng, kAvif, kJxl, kGif, kKeep };       // OutputImageFormat (lib.rs:274-283)
enum BoolKeep : int { kBkNone = -1, kBkKeep, kBkTrue, kBkFalse };                                   // lib.rs:607-611
enum Profile : int { kQpNone = -1, kLowest, kLow, kMediumLow, kMedium, kGood, kHigh, kHighest, kLossless, kPercent };   // lib.rs:644-654
enum JpegStyle : int { kJpegStyleNone = -1, kJpegli, kLibjpegTurbo, kMozjpeg, kJpegDefault };       // lib.rs:384-390
enum PngStyle : int { kPngStyleNone = -1, kLibpng, kLodepng, kPngquant, kPngDefault };              // lib.rs:410-415
enum Coder : int { kCoderMozjpeg, kCoderLibjpegTurbo, kCoderLodepng, kCoderPngquant, kCoderLibpng, kCoderWebpLossy, kCoderWebpLossless, kCoderGif };
enum SourceKind : int { kSourceNone = 0, kSourceJpeg = 1, kSourcePng = 2, kSourceGif = 3, kSourceWebp = 4 };   // IFHIP_SELECT_SOURCE_*

template <class T> using Opt = ifhip::Opt<T>;

struct QualityProfile { int kind = kQpNone; float percent = 0.f; };
// Option<bool> per field: -1 None, 0 Some(false), 1 Some(true) (lib.rs:421-441)
struct AllowedFormats { int8_t webp = -1, jxl = -1, avif = -1, jpeg = -1, jpeg_progressive = -1, jpeg_xyb = -1, png = -1, gif = -1, all = -1, web_safe = -1, modern_web_safe = -1, color_profiles = -1; };
struct EncoderHints {                                                                               // lib.rs:326-404
    bool has_jpeg = false, has_png = false, has_webp = false, has_gif = false;
    Opt<float> jpeg_quality, png_quality, png_min_quality, webp_quality;
    Opt<bool> jpeg_progressive, png_hint_max_deflate;
    Opt<uint8_t> png_quantization_speed;
    int jpeg_mimic = kJpegStyleNone, png_mimic = kPngStyleNone, png_lossless = kBkNone, webp_lossless = kBkNone;
};
struct Preset {                                                                                     // EncoderPreset::Auto | ::Format (lib.rs:710-744)
    bool is_auto = false;
    int format = kFormatNone;                          // Format only
    QualityProfile quality_profile;                    // kind kQpNone: None (Format only)
    Opt<float> quality_profile_dpr;
    bool has_matte = false;
    uint32_t matte = 0;                                // Color32 0xAARRGGBB
    std::string matte_json;                            // the colour as it was given
    int lossless = kBkNone;
    bool has_allow = false, has_hints = false;
    AllowedFormats allow;
    EncoderHints hints;
};
// the job's source (Job::find_source): what get_unscaled_unrotated_image_info tells build_auto_encoder_details (auto.rs:1059-1079)
struct Source { int kind = kSourceNone; bool lossless = false, animated = false; };
struct Resolved {
    int format = kFormatNone;                          // kJpeg, kPng, kWebp or kGif
    int coder = kCoderMozjpeg;
    int quality = -1, minimum_quality = -1, speed = -1;   // u8 options of mozjpeg / libjpeg_turbo / pngquant; -1: None
    float webp_quality = 0.f;
    bool progressive = false, optimize_huffman_coding = false, png_32 = false;
    int maximum_deflate = -1;                          // Option<bool> of lodepng / pngquant
    bool zlib_9 = false;                               // libpng: zlib_compression Some(9)
    bool has_matte = false;
    uint32_t matte = 0;
    std::string matte_json;
};

struct QualityHints { float p, ssim2, moz, jpegli, webp, avif, jxl; uint8_t webp_m, avif_s, jxl_e, png, png_max, png_s; };   // auto.rs:570-586
QualityHints get_quality_hints(const QualityProfile& qp);                                           // auto.rs:725-770
QualityHints get_quality_hints_by_ssim2(float ssim2);                                               // auto.rs:772-803
QualityHints get_quality_hints_with_dpr(const QualityProfile& qp, const Opt<float>& dpr);           // auto.rs:703-724
float approximate_quality_profile(const QualityProfile& qp);                                        // auto.rs:623-628

// True for an `encode` preset this file resolves: {"auto": ..} or {"format": ..}
bool names_selection(const ifshim::JVal* preset);
// throws ifshim::FlowErr kInvalidJson for a missing required field or a wrong type
Preset read_preset(const ifshim::JVal& preset);
// throws ifshim::FlowErr kArgumentInvalid "No formats enabled; ..."
Resolved resolve(const Preset& p, const Source& src, bool alpha_meaningful, uint32_t w, uint32_t h);
// The outcomes that are known from the preset and the source alone (no frame): does it resolve to GIF?
bool resolves_to_gif_without_frame(const Preset& p, const Source& src);
const char* coder_name(int coder);
// {"format": .., "coder": .., "params": {..}, "matte": ..}; params is the object of the named preset of that coder
std::string resolved_json(const Resolved& r);
// calculate_encoder_preset + read_allowed_formats + read_encoder_hints (ir4/encoder.rs:5-98) as JSON, serde's field order
std::string preset_json_of(const ifhip::Ir4Output& o);

}  // namespace ifsel
