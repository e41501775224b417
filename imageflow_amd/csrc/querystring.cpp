// The RIAPI querystring layer (see querystring.hpp): Instructions::delete_from_map (imageflow_riapi/src/ir4/parsing.rs:481-635
// and the Parser helpers :692-1103), the colour helpers (imageflow_helpers/src/colors.rs:36-75), Ir4Layout::add_steps
// (ir4/layout.rs:473-647) and Ir4Expand::get_decode_commands (ir4/mod.rs:155-210).  Reads untrusted text: every index is
// checked, every float-to-integer cast saturates, and tools/sanitize/querystring_fuzz.cpp runs it under ASan + UBSan.
#include "querystring.hpp"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/imageflow_abi_subset.h"
#include "common.hpp"

namespace ifhip {
namespace {

struct QsErr { int status; std::string text; };

std::string trim_ws(const std::string& v) {              // str::trim of ASCII text
    const size_t b = v.find_first_not_of(" \t\r\n\f\v"), e = v.find_last_not_of(" \t\r\n\f\v");
    return b == std::string::npos ? std::string() : v.substr(b, e - b + 1);
}
std::string lower(std::string s) {
    for (char& ch : s) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
    return s;
}
bool ieq(const std::string& a, const char* b) { return lower(a) == lower(b); }             // eq_ignore_ascii_case
int hex_digit(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

// application/x-www-form-urlencoded, as Url::query_pairs decodes it: '+' is a blank, %XX a byte, a '%' that no two hex
// digits follow stays
std::string form_decode(const std::string& s) {
    std::string o;
    o.reserve(s.size());
    for (size_t i = 0; i < s.size(); ++i) {
        if (s[i] == '+') o.push_back(' ');
        else if (s[i] == '%' && i + 2 < s.size() && hex_digit(s[i + 1]) >= 0 && hex_digit(s[i + 2]) >= 0) {
            o.push_back(static_cast<char>(hex_digit(s[i + 1]) * 16 + hex_digit(s[i + 2])));
            i += 2;
        } else o.push_back(s[i]);
    }
    return o;
}

// `str::parse::<f64>` (core dec2flt): an optional sign, then `inf`, `infinity` or `nan` in any case, or digits with an
// optional fraction (at least one digit in all) and an optional exponent; no blanks, no hex
bool rust_float_grammar(const std::string& s) {
    const size_t i = (!s.empty() && (s[0] == '+' || s[0] == '-')) ? 1 : 0;
    const std::string rest = lower(s.substr(i));
    if (rest == "inf" || rest == "infinity" || rest == "nan") return true;
    size_t j = 0, digits = 0;
    while (j < rest.size() && std::isdigit(static_cast<unsigned char>(rest[j]))) { ++j; ++digits; }
    if (j < rest.size() && rest[j] == '.') { ++j; while (j < rest.size() && std::isdigit(static_cast<unsigned char>(rest[j]))) { ++j; ++digits; } }
    if (!digits) return false;
    if (j < rest.size() && rest[j] == 'e') {
        ++j;
        if (j < rest.size() && (rest[j] == '+' || rest[j] == '-')) ++j;
        const size_t e0 = j;
        while (j < rest.size() && std::isdigit(static_cast<unsigned char>(rest[j]))) ++j;
        if (j == e0) return false;
    }
    return j == rest.size();
}
bool parse_f64(const std::string& s, double* out) {      // any value the grammar allows, NaN and infinities included
    if (!rust_float_grammar(s)) return false;
    *out = std::strtod(s.c_str(), nullptr);               // correctly rounded, as Rust's
    return true;
}
bool parse_f32(const std::string& s, float* out) {
    if (!rust_float_grammar(s)) return false;
    *out = std::strtof(s.c_str(), nullptr);
    return true;
}
bool parse_i32(const std::string& s, int32_t* out) {     // `str::parse::<i32>`: sign, digits, no overflow
    size_t i = (!s.empty() && (s[0] == '+' || s[0] == '-')) ? 1 : 0;
    if (i == s.size()) return false;
    int64_t v = 0;
    for (; i < s.size(); ++i) {
        if (!std::isdigit(static_cast<unsigned char>(s[i]))) return false;
        v = v * 10 + (s[i] - '0');
        if (v > 2147483648ll) return false;
    }
    if (s[0] == '-') v = -v;
    if (v > INT32_MAX) return false;
    *out = static_cast<int32_t>(v);
    return true;
}
bool parse_f64_list(const std::string& s, size_t want, std::vector<double>* out, bool lenient) {
    out->clear();
    size_t b = 0;
    while (true) {
        const size_t c = std::min(s.find(',', b), s.size());
        if (out->size() <= want) {                        // (more parts than wanted fail on the count: no need to keep 10 000 of them)
            double d = 0;
            if (!parse_f64(trim_ws(s.substr(b, c - b)), &d)) { if (!lenient) return false; d = 0; }
            out->push_back(d);
        }
        if (c == s.size()) break;
        b = c + 1;
    }
    return out->size() == want;
}

// colors.rs:36-75 -> Color32 0xAARRGGBB
const std::pair<const char*, uint32_t> kCssColors[] = {   // the CSS3 names (colors.rs:199-353); "transparent" is 0
    {"aliceblue", 0xFFF0F8FFu}, {"antiquewhite", 0xFFFAEBD7u}, {"aqua", 0xFF00FFFFu}, {"aquamarine", 0xFF7FFFD4u}, {"azure", 0xFFF0FFFFu},
    {"beige", 0xFFF5F5DCu}, {"bisque", 0xFFFFE4C4u}, {"black", 0xFF000000u}, {"blanchedalmond", 0xFFFFEBCDu}, {"blue", 0xFF0000FFu},
    {"blueviolet", 0xFF8A2BE2u}, {"brown", 0xFFA52A2Au}, {"burlywood", 0xFFDEB887u}, {"cadetblue", 0xFF5F9EA0u}, {"chartreuse", 0xFF7FFF00u},
    {"chocolate", 0xFFD2691Eu}, {"coral", 0xFFFF7F50u}, {"cornflowerblue", 0xFF6495EDu}, {"cornsilk", 0xFFFFF8DCu}, {"crimson", 0xFFDC143Cu},
    {"cyan", 0xFF00FFFFu}, {"darkblue", 0xFF00008Bu}, {"darkcyan", 0xFF008B8Bu}, {"darkgoldenrod", 0xFFB8860Bu}, {"darkgray", 0xFFA9A9A9u},
    {"darkgreen", 0xFF006400u}, {"darkgrey", 0xFFA9A9A9u}, {"darkkhaki", 0xFFBDB76Bu}, {"darkmagenta", 0xFF8B008Bu}, {"darkolivegreen", 0xFF556B2Fu},
    {"darkorange", 0xFFFF8C00u}, {"darkorchid", 0xFF9932CCu}, {"darkred", 0xFF8B0000u}, {"darksalmon", 0xFFE9967Au}, {"darkseagreen", 0xFF8FBC8Fu},
    {"darkslateblue", 0xFF483D8Bu}, {"darkslategray", 0xFF2F4F4Fu}, {"darkslategrey", 0xFF2F4F4Fu}, {"darkturquoise", 0xFF00CED1u},
    {"darkviolet", 0xFF9400D3u}, {"deeppink", 0xFFFF1493u}, {"deepskyblue", 0xFF00BFFFu}, {"dimgray", 0xFF696969u}, {"dimgrey", 0xFF696969u},
    {"dodgerblue", 0xFF1E90FFu}, {"firebrick", 0xFFB22222u}, {"floralwhite", 0xFFFFFAF0u}, {"forestgreen", 0xFF228B22u}, {"fuchsia", 0xFFFF00FFu},
    {"gainsboro", 0xFFDCDCDCu}, {"ghostwhite", 0xFFF8F8FFu}, {"gold", 0xFFFFD700u}, {"goldenrod", 0xFFDAA520u}, {"gray", 0xFF808080u},
    {"green", 0xFF008000u}, {"greenyellow", 0xFFADFF2Fu}, {"grey", 0xFF808080u}, {"honeydew", 0xFFF0FFF0u}, {"hotpink", 0xFFFF69B4u},
    {"indianred", 0xFFCD5C5Cu}, {"indigo", 0xFF4B0082u}, {"ivory", 0xFFFFFFF0u}, {"khaki", 0xFFF0E68Cu}, {"lavender", 0xFFE6E6FAu},
    {"lavenderblush", 0xFFFFF0F5u}, {"lawngreen", 0xFF7CFC00u}, {"lemonchiffon", 0xFFFFFACDu}, {"lightblue", 0xFFADD8E6u},
    {"lightcoral", 0xFFF08080u}, {"lightcyan", 0xFFE0FFFFu}, {"lightgoldenrodyellow", 0xFFFAFAD2u}, {"lightgray", 0xFFD3D3D3u},
    {"lightgreen", 0xFF90EE90u}, {"lightgrey", 0xFFD3D3D3u}, {"lightpink", 0xFFFFB6C1u}, {"lightsalmon", 0xFFFFA07Au},
    {"lightseagreen", 0xFF20B2AAu}, {"lightskyblue", 0xFF87CEFAu}, {"lightslategray", 0xFF778899u}, {"lightslategrey", 0xFF778899u},
    {"lightsteelblue", 0xFFB0C4DEu}, {"lightyellow", 0xFFFFFFE0u}, {"lime", 0xFF00FF00u}, {"limegreen", 0xFF32CD32u}, {"linen", 0xFFFAF0E6u},
    {"magenta", 0xFFFF00FFu}, {"maroon", 0xFF800000u}, {"mediumaquamarine", 0xFF66CDAAu}, {"mediumblue", 0xFF0000CDu}, {"mediumorchid", 0xFFBA55D3u},
    {"mediumpurple", 0xFF9370DBu}, {"mediumseagreen", 0xFF3CB371u}, {"mediumslateblue", 0xFF7B68EEu}, {"mediumspringgreen", 0xFF00FA9Au},
    {"mediumturquoise", 0xFF48D1CCu}, {"mediumvioletred", 0xFFC71585u}, {"midnightblue", 0xFF191970u}, {"mintcream", 0xFFF5FFFAu},
    {"mistyrose", 0xFFFFE4E1u}, {"moccasin", 0xFFFFE4B5u}, {"navajowhite", 0xFFFFDEADu}, {"navy", 0xFF000080u}, {"oldlace", 0xFFFDF5E6u},
    {"olive", 0xFF808000u}, {"olivedrab", 0xFF6B8E23u}, {"orange", 0xFFFFA500u}, {"orangered", 0xFFFF4500u}, {"orchid", 0xFFDA70D6u},
    {"palegoldenrod", 0xFFEEE8AAu}, {"palegreen", 0xFF98FB98u}, {"paleturquoise", 0xFFAFEEEEu}, {"palevioletred", 0xFFDB7093u},
    {"papayawhip", 0xFFFFEFD5u}, {"peachpuff", 0xFFFFDAB9u}, {"peru", 0xFFCD853Fu}, {"pink", 0xFFFFC0CBu}, {"plum", 0xFFDDA0DDu},
    {"powderblue", 0xFFB0E0E6u}, {"purple", 0xFF800080u}, {"rebeccapurple", 0xFF663399u}, {"red", 0xFFFF0000u}, {"rosybrown", 0xFFBC8F8Fu},
    {"royalblue", 0xFF4169E1u}, {"saddlebrown", 0xFF8B4513u}, {"salmon", 0xFFFA8072u}, {"sandybrown", 0xFFF4A460u}, {"seagreen", 0xFF2E8B57u},
    {"seashell", 0xFFFFF5EEu}, {"sienna", 0xFFA0522Du}, {"silver", 0xFFC0C0C0u}, {"skyblue", 0xFF87CEEBu}, {"slateblue", 0xFF6A5ACDu},
    {"slategray", 0xFF708090u}, {"slategrey", 0xFF708090u}, {"snow", 0xFFFFFAFAu}, {"springgreen", 0xFF00FF7Fu}, {"steelblue", 0xFF4682B4u},
    {"tan", 0xFFD2B48Cu}, {"teal", 0xFF008080u}, {"thistle", 0xFFD8BFD8u}, {"tomato", 0xFFFF6347u}, {"turquoise", 0xFF40E0D0u},
    {"violet", 0xFFEE82EEu}, {"wheat", 0xFFF5DEB3u}, {"white", 0xFFFFFFFFu}, {"whitesmoke", 0xFFF5F5F5u}, {"yellow", 0xFFFFFF00u},
    {"yellowgreen", 0xFF9ACD32u},
    {"transparent", 0x00000000u}};
bool parse_color(const std::string& value, uint32_t* out) {
    for (unsigned char ch : value) if (ch >= 0x80) return false;                           // "CSS colors must be in ASCII only"
    if (value.empty()) return false;
    const std::string v = value[0] == '#' ? value.substr(1) : value;
    bool hex = !v.empty() && v.size() <= 8;                                                // u32::from_str_radix(v, 16)
    for (char ch : v) hex = hex && hex_digit(ch) >= 0;
    if (!hex) {
        // (from_str_radix also takes a leading '+' and any number of leading zeros: "+fff" panics in the reference's slicing and
        // "000000fff" is FormatIncorrect -- neither names a colour)
        bool radix_ok = !v.empty();
        size_t k = !v.empty() && v[0] == '+' ? 1 : 0;
        if (k == v.size()) radix_ok = false;
        uint64_t acc = 0;
        for (; radix_ok && k < v.size(); ++k) {
            if (hex_digit(v[k]) < 0) radix_ok = false;
            else { acc = acc * 16 + static_cast<uint64_t>(hex_digit(v[k])); if (acc > 0xFFFFFFFFull) radix_ok = false; }
        }
        if (radix_ok) return false;
        const std::string name = lower(value);
        for (const auto& kv : kCssColors) if (name == kv.first) { *out = kv.second; return true; }
        return false;
    }
    auto part = [&](size_t at, size_t n) -> uint32_t {
        const uint32_t hi = static_cast<uint32_t>(hex_digit(v[at]));
        return n == 1 ? (hi << 4) | hi : (hi << 4) | static_cast<uint32_t>(hex_digit(v[at + 1]));
    };
    switch (v.size()) {
    case 3: *out = 0xFF000000u | (part(0, 1) << 16) | (part(1, 1) << 8) | part(2, 1); return true;
    case 4: *out = (part(3, 1) << 24) | (part(0, 1) << 16) | (part(1, 1) << 8) | part(2, 1); return true;
    case 6: *out = 0xFF000000u | (part(0, 2) << 16) | (part(2, 2) << 8) | part(4, 2); return true;
    case 8: *out = (part(6, 2) << 24) | (part(0, 2) << 16) | (part(2, 2) << 8) | part(4, 2); return true;
    default: return false;
    }
}

bool parse_bool(const std::string& s, bool* out) {       // parsing.rs:841-847
    const std::string v = lower(s);
    if (v == "true" || v == "1" || v == "yes" || v == "on") { *out = true; return true; }
    if (v == "false" || v == "0" || v == "no" || v == "off") { *out = false; return true; }
    return false;
}

// FilterStrings (parsing.rs:159-193) spells every filter with and without underscores, any case -> s::Filter's JSON name.  A
// name the reference would drop with a warning is refused: a drop-in that cannot warn must not pick another filter silently.
std::string filter_name(const std::string& v) {
    static const char* names[] = {"robidoux_fast", "robidoux", "robidoux_sharp", "ginseng", "ginseng_sharp", "lanczos", "lanczos_sharp", "lanczos_2",
                                  "lanczos_2_sharp", "cubic", "cubic_sharp", "catmull_rom", "mitchell", "cubic_b_spline", "hermite", "jinc", "triangle",
                                  "linear", "box", "fastest", "n_cubic", "n_cubic_sharp"};
    auto squash = [](const std::string& t) {
        std::string o;
        for (char ch : t) if (ch != '_') o.push_back(static_cast<char>(std::tolower(static_cast<unsigned char>(ch))));
        return o;
    };
    const std::string want = squash(v);
    for (const char* n : names) if (squash(n) == want) return n;
    char buf[160];
    std::snprintf(buf, sizeof buf, "InvalidNodeParams: querystring filter '%.60s' is not one of imageflow's filters", v.c_str());
    throw QsErr{kQsInvalid, buf};
}

// `width` / `height` / `maxwidth` / `maxheight`: an i32 as the reference reads it; any other text as this library always has
// (the leading number strtod finds, truncated; below 1: not given; beyond an i32: an error)
Opt<int32_t> parse_side(const std::string& raw) {
    Opt<int32_t> r;
    const std::string t = trim_ws(raw);
    if (t.empty()) return r;
    int32_t v = 0;
    if (parse_i32(t, &v)) { r.set(v); return r; }
    const double d = std::atof(raw.c_str());
    if (!(d >= 0 && d <= 2147483647.0)) throw QsErr{kQsInvalid, "InvalidNodeParams: querystring width/height out of range"};
    if (d >= 1) r.set(static_cast<int32_t>(d));
    return r;
}

const char* const kKeys[] = {"width", "w", "height", "h", "maxwidth", "maxheight", "zoom", "dpr", "dppx", "mode", "stretch", "crop", "scale",
                             "cropxunits", "cropyunits", "c", "c.gravity", "anchor", "srotate", "rotate", "sflip", "sourceflip", "flip", "bgcolor",
                             "s.alpha", "s.brightness", "s.contrast", "s.saturation", "s.sepia", "s.grayscale", "f.sharpen", "f.sharpen_when",
                             "up.filter", "down.filter", "up.colorspace", "down.colorspace", "watermark_red_dot", "ignoreicc",
                             "decoder.min_precise_scaling_ratio", "autorotate", "quality", "jpeg.quality", "format", "s.roundcorners",
                             "a.balancewhite", "trim.threshold", "trim.percentpadding"};
// the output keys read only under `encoder_selection` (parsing.rs:589-626); `quality`, `jpeg.quality` and `format` are in kKeys
const char* const kOutputKeys[] = {"thumbnail", "qp", "qp.dpr", "qp.dppx", "lossless", "accept.webp", "accept.avif", "accept.jxl", "accept.color_profiles",
                                   "jpeg.progressive", "jpeg.turbo", "jpeg.li", "webp.quality", "webp.lossless", "png.quality", "png.min_quality",
                                   "png.quantization_speed", "png.libpng", "png.max_deflate", "png.lossless"};
bool parse_u8(const std::string& s, uint8_t* out) {      // `str::parse::<u8>`: an optional '+', digits, at most 255
    size_t i = (!s.empty() && s[0] == '+') ? 1 : 0;
    if (i == s.size()) return false;
    int v = 0;
    for (; i < s.size(); ++i) {
        if (!std::isdigit(static_cast<unsigned char>(s[i]))) return false;
        v = v * 10 + (s[i] - '0');
        if (v > 255) return false;
    }
    *out = static_cast<uint8_t>(v);
    return true;
}

void parse(const std::string& q, Ir4Instructions* out, bool encoder_selection) {
    Ir4Instructions i;
    // Url::from_str would end the query at a '#': what follows is the fragment, and every key in it would be dropped in silence
    if (q.find('#') != std::string::npos) throw QsErr{kQsRefused, "ActionNotSupported: querystring holds a raw '#' (a fragment starts there); write %23"};
    std::map<std::string, std::string> m;               // trimmed values; a repeated key: the last one
    size_t at = 0;
    while (at < q.size()) {
        const size_t amp = std::min(q.find('&', at), q.size());
        const std::string kv = q.substr(at, amp - at);
        at = amp + 1;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) continue;
        const std::string k = lower(form_decode(kv.substr(0, eq)));
        std::string v = form_decode(kv.substr(eq + 1));
        bool known = false;
        for (const char* name : kKeys) known = known || k == name;
        bool output_key = encoder_selection && (k == "quality" || k == "jpeg.quality" || k == "format");
        if (encoder_selection) for (const char* name : kOutputKeys) output_key = output_key || k == name;
        if (output_key) { m[k] = trim_ws(v); continue; }                                   // read below, as the reference reads them
        if (!known) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "ActionNotSupported: querystring key '%.100s'", k.c_str());
            throw QsErr{kQsRefused, buf};
        }
        // ---- the keys the interpreter has always read, as it has always read them
        if (k == "down.filter") i.down_filter = filter_name(v);
        else if (k == "up.filter") i.up_filter = filter_name(v);
        else if (k == "quality" || k == "jpeg.quality") {
            char* end = nullptr;
            const long qv = std::strtol(v.c_str(), &end, 10);
            // a value that is no integer is ignored with a warning by the reference (parse_i32): the encoder's default quality
            // then applies -- the key still says "a JPEG comes out"
            if (end == v.c_str() || *end) i.jpeg_out = true;
            else (k == "quality" ? i.quality : i.jpeg_quality) = static_cast<int>(std::max(0l, std::min(100l, qv)));
        } else if (k == "format") {
            v = lower(v);
            if (v != "jpg" && v != "jpeg") {
                char buf[220];
                std::snprintf(buf, sizeof buf, "ActionNotSupported: querystring format=%.40s (this shim writes JPEG; PNG / GIF / WebP coders are out of scope)", v.c_str());
                throw QsErr{kQsRefused, buf};
            }
            i.jpeg_out = true;
            i.format_jpeg = true;
        } else if (k == "s.roundcorners") {
            // parse_round_corners (:811-840): each comma-separated part trimmed and parsed as an f64; a part that does not parse,
            // or a count other than 1 or 4, leaves the key unset
            const std::string s = trim_ws(v);
            std::vector<double> vals;
            if (!s.empty()) {
                if (parse_f64_list(s, 4, &vals, false)) { i.has_round_corners = true; for (int j = 0; j < 4; ++j) i.round_corners[j] = vals[static_cast<size_t>(j)]; }
                else if (parse_f64_list(s, 1, &vals, false)) { i.has_round_corners = true; for (int j = 0; j < 4; ++j) i.round_corners[j] = vals[0]; }
            }
        } else if (k == "a.balancewhite") {
            // parse_white_balance (:1022-1033): only True and Area add the node (layout.rs:587-589); Simple and Gimp are kept with
            // a warning and add nothing
            const std::string s = lower(trim_ws(v));
            if (s == "true" || s == "area") i.balance_white = true;
        } else if (k == "trim.threshold") {
            int32_t t = 0;
            if (parse_i32(trim_ws(v), &t)) i.trim_threshold.set(t);
        } else if (k == "trim.percentpadding") {
            float f = 0.f;
            if (parse_f32(trim_ws(v), &f) && std::isfinite(f)) i.trim_padding = f;
        } else m[k] = trim_ws(v);
    }
    auto val = [&](const char* key) -> const std::string* {                                // warning_parse (:719-748): blank is absent
        auto it = m.find(key);
        return it == m.end() || it->second.empty() ? nullptr : &it->second;
    };
    auto f32_of = [&](const char* key, Opt<float>* o) {                                    // parse_f32 (:869-874): finite
        float f = 0.f;
        if (const std::string* v = val(key)) if (parse_f32(*v, &f) && std::isfinite(f)) o->set(f);
    };
    auto bool_of = [&](const char* key, Opt<bool>* o) {
        bool b = false;
        if (const std::string* v = val(key)) if (parse_bool(*v, &b)) o->set(b);
    };
    // size and multipliers (:489-494): `width` before `w`, `zoom` before `dpr` before `dppx` -- each only where the one before
    // it gave nothing
    for (const char* k : {"width", "w"}) if (!i.w.some) if (const std::string* v = val(k)) i.w = parse_side(*v);
    for (const char* k : {"height", "h"}) if (!i.h.some) if (const std::string* v = val(k)) i.h = parse_side(*v);
    if (const std::string* v = val("maxwidth")) i.legacy_max_width = parse_side(*v);
    if (const std::string* v = val("maxheight")) i.legacy_max_height = parse_side(*v);
    for (const char* k : {"zoom", "dpr", "dppx"})
        if (!i.zoom.some) if (const std::string* v = val(k)) {                             // parse_dpr (:875-880)
            std::string t = *v;
            while (!t.empty() && t.back() == 'x') t.pop_back();
            float f = 0.f;
            if (parse_f32(t, &f) && std::isfinite(f)) i.zoom.set(f);
        }
    // flip-rotate (:497-500)
    auto flip_of = [&](const std::string* v, bool* has, bool* fh, bool* fv) {
        if (!v) return;
        const std::string s = lower(*v);
        if (s == "none") { *has = true; *fh = false; *fv = false; }
        else if (s == "h" || s == "x") { *has = true; *fh = true; *fv = false; }
        else if (s == "v" || s == "y") { *has = true; *fh = false; *fv = true; }
        else if (s == "both" || s == "xy") { *has = true; *fh = true; *fv = true; }
    };
    flip_of(val("flip"), &i.has_flip, &i.flip_h, &i.flip_v);
    flip_of(val("sflip"), &i.has_sflip, &i.sflip_h, &i.sflip_v);
    if (!i.has_sflip) flip_of(val("sourceflip"), &i.has_sflip, &i.sflip_h, &i.sflip_v);
    auto rotate_of = [&](const char* key, Opt<int32_t>* o) {                               // parse_rotate (:962-974)
        float value = 0.f;
        const std::string* v = val(key);
        if (!v || !parse_f32(*v, &value)) return;
        const float turns = std::fmod(std::round(value / 90.f), 4.f);
        const int32_t t = turns != turns ? 0 : static_cast<int32_t>(turns);                // |turns| < 4
        o->set(((t + 4) % 4) * 90);
    };
    rotate_of("srotate", &i.srotate);
    rotate_of("rotate", &i.rotate);
    bool_of("autorotate", &i.autorotate);
    // fit mode and scale (:504-526)
    if (const std::string* v = val("mode")) {
        if (ieq(*v, "max")) i.mode = kIr4Max;
        else if (ieq(*v, "pad")) i.mode = kIr4Pad;
        else if (ieq(*v, "crop")) i.mode = kIr4Crop;
        else if (ieq(*v, "stretch") || ieq(*v, "carve")) i.mode = kIr4Stretch;
        else if (ieq(*v, "aspectcrop")) i.mode = kIr4AspectCrop;                            // (`none` and anything else: unset)
    }
    if (i.mode == kIr4FitUnset) if (const std::string* v = val("stretch")) if (ieq(*v, "fill")) i.mode = kIr4Stretch;
    const std::string* crop_text = val("crop");
    if (crop_text && ieq(*crop_text, "auto")) { if (i.mode == kIr4FitUnset) i.mode = kIr4Crop; crop_text = nullptr; }
    if (const std::string* v = val("scale")) {
        if (ieq(*v, "down") || ieq(*v, "downscaleonly")) i.scale = kIr4Down;
        else if (ieq(*v, "up") || ieq(*v, "upscaleonly")) i.scale = kIr4Up;
        else if (ieq(*v, "both")) i.scale = kIr4Both;
        else if (ieq(*v, "canvas") || ieq(*v, "upscalecanvas")) i.scale = kIr4Canvas;
    }
    bool_of("ignoreicc", &i.ignoreicc);
    auto colorspace_of = [&](const char* key, int* o) {
        if (const std::string* v = val(key)) *o = ieq(*v, "srgb") ? Ir4Instructions::kSrgb : ieq(*v, "linear") ? Ir4Instructions::kLinear : ieq(*v, "gamma") ? Ir4Instructions::kGamma : Ir4Instructions::kUnset;
    };
    colorspace_of("down.colorspace", &i.down_colorspace);
    colorspace_of("up.colorspace", &i.up_colorspace);
    // crop (:539-553): `c` is a strict crop in percent and shuts out `crop` and its units; `crop` strict, then lenient
    std::vector<double> vals;
    const std::string* c = val("c");
    if (c && parse_f64_list(*c, 4, &vals, false)) {
        i.has_crop = true; i.cropxunits.set(100.0); i.cropyunits.set(100.0);
    } else {
        if (crop_text) {
            if (parse_f64_list(*crop_text, 4, &vals, false)) i.has_crop = true;
            else {                                                                         // parse_crop (:793-809)
                std::string s;
                for (char ch : *crop_text) if (ch != '(' && ch != ')') s.push_back(ch);
                i.has_crop = parse_f64_list(trim_ws(s), 4, &vals, true);
            }
        }
        double d = 0;
        if (const std::string* v = val("cropxunits")) if (parse_f64(*v, &d) && std::isfinite(d)) i.cropxunits.set(d);
        if (const std::string* v = val("cropyunits")) if (parse_f64(*v, &d) && std::isfinite(d)) i.cropyunits.set(d);
    }
    if (i.has_crop) for (int j = 0; j < 4; ++j) i.crop[j] = vals[static_cast<size_t>(j)];
    if (const std::string* v = val("c.gravity")) if (parse_f64_list(*v, 2, &vals, false)) { i.has_c_gravity = true; i.c_gravity[0] = vals[0]; i.c_gravity[1] = vals[1]; }
    if (const std::string* v = val("anchor")) {                                            // parse_anchor (:1079-1102)
        static const struct { const char* name; Anchor1D::Kind x, y; } kNames[] = {
            {"topleft", Anchor1D::kNear, Anchor1D::kNear}, {"topcenter", Anchor1D::kCenter, Anchor1D::kNear}, {"topright", Anchor1D::kFar, Anchor1D::kNear},
            {"middleleft", Anchor1D::kNear, Anchor1D::kCenter}, {"middlecenter", Anchor1D::kCenter, Anchor1D::kCenter}, {"middleright", Anchor1D::kFar, Anchor1D::kCenter},
            {"bottomleft", Anchor1D::kNear, Anchor1D::kFar}, {"bottomcenter", Anchor1D::kCenter, Anchor1D::kFar}, {"bottomright", Anchor1D::kFar, Anchor1D::kFar}};
        const std::string s = lower(*v);
        for (const auto& n : kNames) if (s == n.name) { i.has_anchor = true; i.anchor_x.kind = n.x; i.anchor_y.kind = n.y; }
        if (!i.has_anchor && parse_f64_list(s, 2, &vals, false)) {
            i.has_anchor = true;
            i.anchor_x.kind = i.anchor_y.kind = Anchor1D::kPercent;
            i.anchor_x.percent = static_cast<float>(vals[0]); i.anchor_y.percent = static_cast<float>(vals[1]);
        }
    }
    // effects (:556-562)
    if (const std::string* v = val("s.grayscale")) {
        if (ieq(*v, "true") || ieq(*v, "y") || ieq(*v, "ntsc")) i.s_grayscale = "grayscale_ntsc";
        else if (ieq(*v, "ry")) i.s_grayscale = "grayscale_ry";
        else if (ieq(*v, "flat")) i.s_grayscale = "grayscale_flat";
        else if (ieq(*v, "bt709")) i.s_grayscale = "grayscale_bt709";
    }
    f32_of("s.contrast", &i.s_contrast);
    f32_of("s.alpha", &i.s_alpha);
    f32_of("s.saturation", &i.s_saturation);
    f32_of("s.brightness", &i.s_brightness);
    bool_of("s.sepia", &i.s_sepia);
    // resizing filter and sharpening (:578-582)
    f32_of("f.sharpen", &i.f_sharpen);
    if (const std::string* v = val("f.sharpen_when")) {
        if (ieq(*v, "downscaling")) i.f_sharpen_when = "downscaling";
        else if (ieq(*v, "sizediffers")) i.f_sharpen_when = "size_differs";
        else if (ieq(*v, "always")) i.f_sharpen_when = "always";
    }
    f32_of("decoder.min_precise_scaling_ratio", &i.min_precise_scaling_ratio);
    if (const std::string* v = val("bgcolor")) { uint32_t col = 0; if (parse_color(*v, &col)) i.bgcolor.set(col); }
    bool_of("watermark_red_dot", &i.watermark_red_dot);
    if (encoder_selection) {
        // Format-specific tuning and format selection (:589-626)
        Ir4Output& o = i.out;
        o.parsed = true;
        auto i32_of = [&](const char* key, Opt<int32_t>* t) { int32_t n = 0; if (const std::string* v = val(key)) if (parse_i32(*v, &n)) t->set(n); };
        auto u8_of = [&](const char* key, Opt<uint8_t>* t) { uint8_t n = 0; if (const std::string* v = val(key)) if (parse_u8(*v, &n)) t->set(n); };
        auto bool_keep_of = [&](const char* key, int* t) {                                  // parse_bool_keep (:848-856)
            bool b = false;
            if (const std::string* v = val(key)) {
                if (parse_bool(*v, &b)) *t = b ? Ir4Output::kBkTrue : Ir4Output::kBkFalse;
                else if (ieq(*v, "keep") || ieq(*v, "preserve")) *t = Ir4Output::kBkKeep;
            }
        };
        i32_of("jpeg.quality", &o.jpeg_quality);
        bool_of("jpeg.progressive", &o.jpeg_progressive);
        bool_of("jpeg.turbo", &o.jpeg_turbo);
        bool_of("jpeg.li", &o.jpeg_li);
        f32_of("webp.quality", &o.webp_quality);
        bool_keep_of("webp.lossless", &o.webp_lossless);
        bool_keep_of("png.lossless", &o.png_lossless);
        u8_of("png.min_quality", &o.png_min_quality);
        u8_of("png.quality", &o.png_quality);
        u8_of("png.quantization_speed", &o.png_quantization_speed);
        bool_of("png.libpng", &o.png_libpng);
        bool_of("png.max_deflate", &o.png_max_deflate);
        bool_of("accept.jxl", &o.accept_jxl);
        bool_of("accept.webp", &o.accept_webp);
        bool_of("accept.avif", &o.accept_avif);
        bool_of("accept.color_profiles", &o.accept_color_profiles);
        for (const char* key : {"format", "thumbnail"}) {                                  // OutputFormatStrings (:50-66, 1134-1154): 15 spellings, any case
            if (o.format != Ir4Output::kFormatUnset) break;
            const std::string* v = val(key);
            if (!v) continue;
            static const struct { const char* name; int format; } kNames[] = {
                {"jpg", Ir4Output::kJpeg}, {"jpe", Ir4Output::kJpeg}, {"jif", Ir4Output::kJpeg}, {"jfif", Ir4Output::kJpeg}, {"jfi", Ir4Output::kJpeg},
                {"exif", Ir4Output::kJpeg}, {"jpeg", Ir4Output::kJpeg}, {"png", Ir4Output::kPng}, {"gif", Ir4Output::kGif}, {"webp", Ir4Output::kWebp},
                {"avif", Ir4Output::kAvif}, {"jxl", Ir4Output::kJxl}, {"jpegxl", Ir4Output::kJxl}, {"auto", Ir4Output::kAuto}, {"keep", Ir4Output::kKeep}};
            for (const auto& n : kNames) if (ieq(*v, n.name)) { o.format = n.format; break; }
        }
        bool_keep_of("lossless", &o.lossless);
        i32_of("quality", &o.quality);
        if (const std::string* v = val("qp")) {                                            // parse_quality_profile (:910-925), QualityProfile::parse
            static const struct { const char* name; int qp; } kNames[] = {
                {"lowest", Ir4Output::kLowest}, {"low", Ir4Output::kLow}, {"medium-low", Ir4Output::kMediumLow}, {"mediumlow", Ir4Output::kMediumLow},
                {"medium", Ir4Output::kMedium}, {"good", Ir4Output::kGood}, {"medium-high", Ir4Output::kGood}, {"mediumhigh", Ir4Output::kGood},
                {"high", Ir4Output::kHigh}, {"highest", Ir4Output::kHighest}, {"lossless", Ir4Output::kLossless}};
            float f = 0.f;
            if (ieq(*v, "quality")) { if (o.quality.some) { o.qp = Ir4Output::kPercent; o.qp_percent = static_cast<float>(o.quality.v); } }
            else {
                for (const auto& n : kNames) if (o.qp == Ir4Output::kQpUnset && ieq(*v, n.name)) o.qp = n.qp;
                if (o.qp == Ir4Output::kQpUnset && parse_f32(*v, &f)) { o.qp = Ir4Output::kPercent; o.qp_percent = std::fmin(100.f, std::fmax(0.f, f)); }   // (a NaN is 0)
            }
        }
        for (const char* key : {"qp.dpr", "qp.dppx"}) {                                    // parse_qp_dpr (:881-896): no finiteness check
            if (o.qp_dpr.some) break;
            const std::string* v = val(key);
            if (!v) continue;
            if (ieq(*v, "dpr") || ieq(*v, "dppx") || ieq(*v, "zoom")) { if (i.zoom.some) o.qp_dpr.set(i.zoom.v); continue; }
            std::string t = *v;
            while (!t.empty() && t.back() == 'x') t.pop_back();
            float f = 0.f;
            if (parse_f32(t, &f)) o.qp_dpr.set(f);
        }
        i.format_jpeg = i.jpeg_out = o.format == Ir4Output::kJpeg;                         // the white background of format=jpg (layout.rs:492-503)
    }
    // the reference parses `autorotate` and never reads it: its decoder always applies the EXIF orientation, as this one does
    if (i.autorotate.some && !i.autorotate.v)
        throw QsErr{kQsRefused, "ActionNotSupported: querystring autorotate=false (the decoder always applies the EXIF orientation, as the reference's does)"};
    *out = i;
}

// ---- JSON out ------------------------------------------------------------------------------------------------------------
std::string num(double v) {                              // 17 digits: the text reads back as the very same double
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}
std::string f32_json(float v) { return std::isfinite(v) ? num(static_cast<double>(v)) : "null"; }   // (serde_json writes a NaN as null)
// bgcolor, else white for format=jpg, else transparent (layout.rs:492-503).  The resample's own background is white also for a
// `quality` that is no number (white_default = jpeg_out): such a string has always been flattened by the resampler here.
std::string color_json(const Ir4Instructions& i, bool white_default) {
    if (i.bgcolor.some) {
        const uint32_t c = i.bgcolor.v;
        char buf[64];
        std::snprintf(buf, sizeof buf, "{\"srgb\":{\"hex\":\"%08X\"}}", static_cast<unsigned>((c << 8) | (c >> 24)));   // to_rrggbbaa_string
        return buf;
    }
    return white_default ? "{\"srgb\":{\"hex\":\"FFFFFFFF\"}}" : "\"transparent\"";
}

// command_string.watermarks: the elements of the array as they stand, and whether each one's fit_box is of the canvas
struct Scan {
    const char *p, *end;
    int depth = 0;
    void ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) ++p; }
    bool str(std::string* raw) {                         // at '"': through the closing quote; *raw: the text between, escapes as written
        if (p >= end || *p != '"') return false;
        ++p;
        const char* b = p;
        while (p < end && *p != '"') { if (*p == '\\') ++p; if (p < end) ++p; }
        if (p >= end) return false;
        if (raw) raw->assign(b, static_cast<size_t>(p - b));
        ++p;
        return true;
    }
    bool value() {
        ws();
        if (p >= end) return false;
        if (*p == '"') return str(nullptr);
        if (*p == '{' || *p == '[') {
            const char close = *p == '{' ? '}' : ']';
            const bool obj = *p == '{';
            if (++depth > 64) return false;
            ++p; ws();
            if (p < end && *p == close) { ++p; --depth; return true; }
            while (true) {
                if (obj) { ws(); if (!str(nullptr)) return false; ws(); if (p >= end || *p != ':') return false; ++p; }
                if (!value()) return false;
                ws();
                if (p < end && *p == ',') { ++p; continue; }
                if (p < end && *p == close) { ++p; --depth; return true; }
                return false;
            }
        }
        const char* b = p;
        while (p < end && *p != ',' && *p != ']' && *p != '}' && *p != ' ' && *p != '\n' && *p != '\r' && *p != '\t') ++p;
        return p > b;
    }
};
bool fit_box_of_canvas(const std::string& mark) {        // WatermarkConstraintBox::CanvasMargins | CanvasPercentage (layout.rs:626-636)
    Scan s{mark.data(), mark.data() + mark.size()};
    s.ws();
    if (s.p >= s.end || *s.p != '{') return false;
    ++s.p;
    while (true) {
        s.ws();
        std::string key;
        if (!s.str(&key)) return false;
        s.ws();
        if (s.p >= s.end || *s.p != ':') return false;
        ++s.p; s.ws();
        if (key == "fit_box") {
            if (s.p >= s.end || *s.p != '{') return false;
            ++s.p; s.ws();
            std::string kind;
            return s.str(&kind) && (kind == "canvas_margins" || kind == "canvas_percentage");
        }
        if (!s.value()) return false;
        s.ws();
        if (s.p < s.end && *s.p == ',') { ++s.p; continue; }
        return false;
    }
}
void split_watermarks(const char* text, std::vector<std::string>* image_marks, std::vector<std::string>* canvas_marks) {
    if (!text) return;
    Scan s{text, text + std::strlen(text)};
    s.ws();
    if (s.end - s.p == 4 && !std::memcmp(s.p, "null", 4)) return;
    auto bad = [] { throw QsErr{kQsInvalid, "InvalidJson: command_string.watermarks must be an array of watermark objects"}; };
    if (s.p >= s.end || *s.p != '[') bad();
    ++s.p; s.ws();
    if (s.p < s.end && *s.p == ']') { ++s.p; s.ws(); if (s.p != s.end) bad(); return; }
    while (true) {
        s.ws();
        const char* b = s.p;
        if (s.p >= s.end || *s.p != '{' || !s.value()) bad();
        const std::string mark(b, static_cast<size_t>(s.p - b));
        (fit_box_of_canvas(mark) ? canvas_marks : image_marks)->push_back(mark);
        s.ws();
        if (s.p < s.end && *s.p == ',') { ++s.p; continue; }
        if (s.p < s.end && *s.p == ']') { ++s.p; break; }
        bad();
    }
    s.ws();
    if (s.p != s.end) bad();
}

void add_rotate(std::vector<std::string>* steps, const Opt<int32_t>& r) {                  // FramewiseBuilder::add_rotate (:796-805)
    if (!r.some) return;
    switch (((r.v / 90) + 4) % 4) {
    case 1: steps->push_back("\"rotate_90\""); break;
    case 2: steps->push_back("\"rotate_180\""); break;
    case 3: steps->push_back("\"rotate_270\""); break;
    default: break;
    }
}

void expand(const Ir4Instructions& i, int32_t sw, int32_t sh, int32_t rw, int32_t rh, const char* watermarks_json, std::string* json) {
    if (sw < 1 || sh < 1 || rw < 1 || rh < 1) throw QsErr{kQsLayoutError, "InvalidDimensions"};
    Ir4LayoutResult lay;
    std::string err;
    if (!ir4_crop_and_layout(i, sw, sh, rw, rh, &lay, &err)) throw QsErr{kQsLayoutError, err};
    std::vector<std::string> image_marks, canvas_marks;
    split_watermarks(watermarks_json, &image_marks, &canvas_marks);
    // ---- Ir4Expand::get_decode_commands (ir4/mod.rs:155-210); `to.w` divides both sides there (:161-162)
    std::vector<std::string> commands;
    {
        const double downscale_ratio = std::min(static_cast<double>(lay.source_w) / static_cast<double>(lay.image_w), static_cast<double>(lay.source_h) / static_cast<double>(lay.image_w));
        const double preshrink = (i.min_precise_scaling_ratio.some ? static_cast<double>(i.min_precise_scaling_ratio.v) : 2.1) / downscale_ratio;
        const bool gamma_correct = i.down_colorspace != Ir4Instructions::kSrgb;
        if (i.ignoreicc.some && i.ignoreicc.v) commands.push_back("\"discard_color_profile\"");
        if (preshrink < 1.0) {
            auto as_i64 = [](double v) -> long long { return v != v ? 0 : v >= 9.2e18 ? INT64_MAX : v <= -9.2e18 ? INT64_MIN : static_cast<long long>(v); };
            const long long hw = as_i64(std::floor(static_cast<double>(sw) * preshrink)), hh = as_i64(std::floor(static_cast<double>(sh) * preshrink));
            const char* g = gamma_correct ? "true" : "false";
            commands.push_back("{\"jpeg_downscale_hints\":{\"width\":" + std::to_string(hw) + ",\"height\":" + std::to_string(hh) + ",\"scale_luma_spatially\":" + g +
                               ",\"gamma_correct_for_srgb_during_spatial_luma_scaling\":" + g + "}}");
            if (!gamma_correct) commands.push_back("{\"webp_decoder_hints\":{\"width\":" + std::to_string(static_cast<int32_t>(hw)) + ",\"height\":" + std::to_string(static_cast<int32_t>(hh)) + "}}");
        }
    }
    // ---- Ir4Layout::add_steps (ir4/layout.rs:473-647)
    std::vector<std::string> steps;
    add_rotate(&steps, i.srotate);
    if (i.has_sflip) { if (i.sflip_h) steps.push_back("\"flip_h\""); if (i.sflip_v) steps.push_back("\"flip_v\""); }
    if (lay.has_crop)
        steps.push_back("{\"crop\":{\"x1\":" + std::to_string(lay.crop[0]) + ",\"y1\":" + std::to_string(lay.crop[1]) + ",\"x2\":" + std::to_string(lay.crop[2]) + ",\"y2\":" + std::to_string(lay.crop[3]) + "}}");
    const std::string bg = color_json(i, i.format_jpeg);
    {
        const bool downscaling = lay.image_w < lay.source_w || lay.image_h < lay.source_h;
        const int space = downscaling ? i.down_colorspace : i.up_colorspace;
        std::string h = "{";
        if (i.f_sharpen.some) h += "\"sharpen_percent\":" + f32_json(i.f_sharpen.v) + ",";
        if (!i.down_filter.empty()) h += "\"down_filter\":\"" + i.down_filter + "\",";
        if (!i.up_filter.empty()) h += "\"up_filter\":\"" + i.up_filter + "\",";
        if (space == Ir4Instructions::kLinear) h += "\"scaling_colorspace\":\"linear\",";
        else if (space == Ir4Instructions::kSrgb) h += "\"scaling_colorspace\":\"srgb\",";
        h += "\"background_color\":" + color_json(i, i.jpeg_out) + ",\"resample_when\":\"size_differs_or_sharpening_requested\"";
        if (!i.f_sharpen_when.empty()) h += ",\"sharpen_when\":\"" + i.f_sharpen_when + "\"";
        steps.push_back("{\"resample_2d\":{\"w\":" + std::to_string(lay.image_w) + ",\"h\":" + std::to_string(lay.image_h) + ",\"hints\":" + h + "}}}");
    }
    if (i.has_round_corners) {
        const double* q = i.round_corners;
        std::string radius;
        if (q[0] == q[1] && q[0] == q[2] && q[0] == q[3]) radius = "{\"percentage\":" + f32_json(static_cast<float>(q[0])) + "}";      // iter_all_eq (NaN: never)
        else radius = "{\"percentage_custom\":{\"top_left\":" + f32_json(static_cast<float>(q[0])) + ",\"top_right\":" + f32_json(static_cast<float>(q[1])) +
                      ",\"bottom_right\":" + f32_json(static_cast<float>(q[2])) + ",\"bottom_left\":" + f32_json(static_cast<float>(q[3])) + "}}";
        steps.push_back("{\"round_image_corners\":{\"radius\":" + radius + ",\"background_color\":" + bg + "}}");
    }
    if (i.s_alpha.some) steps.push_back("{\"color_filter_srgb\":{\"alpha\":" + f32_json(i.s_alpha.v) + "}}");
    if (i.s_brightness.some) steps.push_back("{\"color_filter_srgb\":{\"brightness\":" + f32_json(i.s_brightness.v) + "}}");
    if (i.s_contrast.some) steps.push_back("{\"color_filter_srgb\":{\"contrast\":" + f32_json(i.s_contrast.v) + "}}");
    if (i.s_saturation.some) steps.push_back("{\"color_filter_srgb\":{\"saturation\":" + f32_json(i.s_saturation.v) + "}}");
    if (i.s_sepia.some && i.s_sepia.v) steps.push_back("{\"color_filter_srgb\":\"sepia\"}");
    if (!i.s_grayscale.empty()) steps.push_back("{\"color_filter_srgb\":\"" + i.s_grayscale + "\"}");
    if (i.balance_white) steps.push_back("{\"white_balance_histogram_area_threshold_srgb\":{\"threshold\":null}}");
    for (const std::string& w : image_marks) steps.push_back("{\"watermark\":" + w + "}");
    Anchor1D ax, ay;                                                                        // pad_anchor: anchor alone, c.gravity places only the crop
    if (i.has_anchor) { ax = i.anchor_x; ay = i.anchor_y; }
    int32_t left = 0, top = 0;
    if (!ir4_align(ax, ay, lay.image_w, lay.image_h, lay.canvas_w, lay.canvas_h, &left, &top)) throw QsErr{kQsLayoutError, "Outer box should never be smaller than inner box. All values must > 0"};
    const int64_t right = static_cast<int64_t>(lay.canvas_w) - lay.image_w - left, bottom = static_cast<int64_t>(lay.canvas_h) - lay.image_h - top;
    if (left > 0 || top > 0 || right > 0 || bottom > 0) {
        if (left < 0 || top < 0 || right < 0 || bottom < 0) throw QsErr{kQsLayoutError, "Negative padding showed up"};
        steps.push_back("{\"expand_canvas\":{\"left\":" + std::to_string(left) + ",\"top\":" + std::to_string(top) + ",\"right\":" + std::to_string(right) + ",\"bottom\":" + std::to_string(bottom) + ",\"color\":" + bg + "}}");
    }
    for (const std::string& w : canvas_marks) steps.push_back("{\"watermark\":" + w + "}");
    add_rotate(&steps, i.rotate);
    if (i.has_flip) { if (i.flip_h) steps.push_back("\"flip_h\""); if (i.flip_v) steps.push_back("\"flip_v\""); }
    if (i.watermark_red_dot.some && i.watermark_red_dot.v) steps.push_back("\"watermark_red_dot\"");   // after rotate / flip, unlike ImageResizer (:641-644)
    std::string o = "{\"decoder_commands\":[";
    for (size_t k = 0; k < commands.size(); ++k) o += (k ? "," : "") + commands[k];
    o += "],\"steps\":[";
    for (size_t k = 0; k < steps.size(); ++k) o += (k ? "," : "") + steps[k];
    o += "],\"canvas\":[" + std::to_string(lay.canvas_w) + "," + std::to_string(lay.canvas_h) + "]}";
    *json = o;
}

}  // namespace

int parse_querystring(const std::string& text, Ir4Instructions* out, std::string* error, bool encoder_selection) {
    try {
        parse(text, out, encoder_selection);
        return kQsOk;
    } catch (const QsErr& e) {
        if (error) *error = e.text;
        return e.status;
    }
}

int expand_querystring(const Ir4Instructions& i, int32_t source_w, int32_t source_h, int32_t reference_w, int32_t reference_h,
                       const char* watermarks_json, std::string* json, std::string* error) {
    try {
        expand(i, source_w, source_h, reference_w, reference_h, watermarks_json, json);
        return kQsOk;
    } catch (const QsErr& e) {
        if (error) *error = e.status == kQsLayoutError ? "InvalidNodeParams: querystring layout error: " + e.text : e.text;
        return e.status;
    }
}

}  // namespace ifhip

extern "C" int ifhip_shim_expand_command_string(const char* value, int32_t source_w, int32_t source_h, int32_t reference_w, int32_t reference_h,
                                                const char* watermarks_json, char* out, size_t cap, size_t* needed) {
    if (!value || !needed || (!out && cap)) return ifhip::fail(ifhip::kQsInvalid, "InvalidArgument: ifhip_shim_expand_command_string needs value and needed");
    ifhip::Ir4Instructions i;
    std::string json, err;
    int rc = ifhip::parse_querystring(value, &i, &err);
    if (rc == ifhip::kQsOk) rc = ifhip::expand_querystring(i, source_w, source_h, reference_w, reference_h, watermarks_json, &json, &err);
    if (rc != ifhip::kQsOk) return ifhip::fail(rc, "%s", err.c_str());
    *needed = json.size() + 1;
    if (cap >= json.size() + 1) std::memcpy(out, json.c_str(), json.size() + 1);
    return ifhip::kQsOk;
}
