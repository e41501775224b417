// The RIAPI querystring of `command_string` {kind: "ir4"}: imageflow_riapi's Instructions (src/ir4/parsing.rs), parsed from
// the text, and their expansion into the nodes and decoder commands the reference builds (Ir4Layout::add_steps, ir4/layout.rs
// :473-647; Ir4Expand::get_decode_commands, ir4/mod.rs:155-210).  Host text and arithmetic only -- no device, no context:
// the interpreter (Job::command_string, shim_nodes.cpp) runs what comes out, and ifhip_shim_expand_command_string hands the same expansion to tests.
#pragma once
#include <cstdint>
#include <string>

#include "layout.hpp"

namespace ifhip {

enum QsStatus : int { kQsOk = 0, kQsLayoutError = 1, kQsRefused = 2, kQsInvalid = 3 };

// The encoder half of Instructions as the reference reads it (ir4/parsing.rs:589-626), filled only where the parser is told
// that the caller selects its encoder as the reference does (parse_querystring's `encoder_selection`).
struct Ir4Output {
    enum Format : int { kFormatUnset = -1, kKeep, kJpeg, kPng, kGif, kWebp, kAvif, kJxl, kAuto };   // OutputFormat (:1346-1355)
    enum BoolKeep : int { kBkUnset = -1, kBkKeep, kBkTrue, kBkFalse };
    enum Qp : int { kQpUnset = -1, kLowest, kLow, kMediumLow, kMedium, kGood, kHigh, kHighest, kLossless, kPercent };
    bool parsed = false;
    int format = kFormatUnset;                         // `format`, else `thumbnail`
    Opt<int32_t> quality, jpeg_quality;
    Opt<bool> jpeg_progressive, jpeg_turbo, jpeg_li, png_libpng, png_max_deflate, accept_webp, accept_avif, accept_jxl, accept_color_profiles;
    Opt<float> webp_quality, qp_dpr;
    Opt<uint8_t> png_quality, png_min_quality, png_quantization_speed;
    int lossless = kBkUnset, webp_lossless = kBkUnset, png_lossless = kBkUnset;
    int qp = kQpUnset;
    float qp_percent = 0.f;
};

struct Ir4Instructions : Ir4LayoutParams {             // ir4/parsing.rs:1236-1337, the keys this library honours
    Ir4Output out;
    Opt<int32_t> rotate;
    bool has_flip = false, flip_h = false, flip_v = false, has_sflip = false, sflip_h = false, sflip_v = false;
    Opt<uint32_t> bgcolor;                             // Color32: 0xAARRGGBB
    Opt<float> s_alpha, s_brightness, s_contrast, s_saturation, f_sharpen, min_precise_scaling_ratio;
    Opt<bool> s_sepia, watermark_red_dot, ignoreicc, autorotate;
    std::string s_grayscale;                           // the ColorFilterSrgb name ("grayscale_ntsc" ...), empty: unset
    std::string f_sharpen_when;                        // s::SharpenWhen's JSON name, empty: unset
    std::string down_filter, up_filter;                // s::Filter's JSON name, empty: unset
    enum Colorspace : int { kUnset = -1, kSrgb, kLinear, kGamma };
    int down_colorspace = kUnset, up_colorspace = kUnset;
    bool has_round_corners = false;                    // s.roundcorners: 1 or 4 values
    double round_corners[4] = {0, 0, 0, 0};
    bool balance_white = false;                        // a.balancewhite = true | area
    Opt<int32_t> trim_threshold;                       // trim.threshold: the caller trims before it lays out
    float trim_padding = 0.f;
    // the encoder half, as the interpreter has always read it: `quality` / `jpeg.quality` (-1: unset), `format=jpg|jpeg`
    int quality = -1, jpeg_quality = -1;
    bool jpeg_out = false, format_jpeg = false;
};

// The text of a querystring -> Instructions (Instructions::delete_from_map, ir4/parsing.rs:481-635).  kQsRefused: a key this
// library does not honour (the reference would warn and go on; a drop-in that cannot warn refuses); kQsInvalid: a filter name
// or a size no value of the reference's could mean.  *error: "ActionNotSupported: ..." / "InvalidNodeParams: ...".
// encoder_selection: the output keys (`format` / `thumbnail` in all their spellings, `qp`, `qp.dpr` / `qp.dppx`, `lossless`,
// `accept.*`, `quality`, `jpeg.*`, `webp.*`, `png.*`) are read with the reference's parsers (:589-626, 848-925, 1346-1385) into
// out->out instead of refused; false: the string is read as it always was.
int parse_querystring(const std::string& text, Ir4Instructions* out, std::string* error, bool encoder_selection = false);

// Instructions + the frame they meet -> {"decoder_commands": [...], "steps": [...], "canvas": [w, h]}: the nodes in the JSON form
// v1/execute takes, without decode and encode.  watermarks: the JSON text of command_string.watermarks (an array), or null.
int expand_querystring(const Ir4Instructions& i, int32_t source_w, int32_t source_h, int32_t reference_w, int32_t reference_h,
                       const char* watermarks_json, std::string* json, std::string* error);

}  // namespace ifhip
