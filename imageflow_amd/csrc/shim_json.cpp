// shim_json.cpp -- the JSON reader of the ABI shim and the parameter readers behind it (shim_json.hpp).
#include "shim_json.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/imageflow_hip.h"   // (plain C99: the IFHIP_ENCODE_CODER_* constants)

namespace ifshim {

// ---- JSON ------------------------------------------------------------------------------------------------------
struct JParser {
    const char *p, *end;
    int depth = 0;
    void ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) ++p; }
    [[noreturn]] void bad(const char* what) { raise(kInvalidJson, "InvalidJson: %s at byte %ld", what, static_cast<long>(end - p)); }
    void lit(const char* w) { const size_t n = std::strlen(w); if (static_cast<size_t>(end - p) < n || std::memcmp(p, w, n)) bad("bad literal"); p += n; }
    std::string str() {
        std::string out;
        ++p;
        while (true) {
            if (p >= end) bad("unterminated string");
            const unsigned char c = static_cast<unsigned char>(*p++);
            if (c == '"') return out;
            if (c < 0x20) bad("control character in string");
            if (c != '\\') { out.push_back(static_cast<char>(c)); continue; }
            if (p >= end) bad("unterminated escape");
            const char e = *p++;
            switch (e) {
            case '"': case '\\': case '/': out.push_back(e); break;
            case 'b': out.push_back('\b'); break;
            case 'f': out.push_back('\f'); break;
            case 'n': out.push_back('\n'); break;
            case 'r': out.push_back('\r'); break;
            case 't': out.push_back('\t'); break;
            case 'u': {
                if (end - p < 4) bad("short \\u escape");
                unsigned v = 0;
                for (int i = 0; i < 4; ++i) {
                    const char h = *p++;
                    v = v * 16 + (h >= '0' && h <= '9' ? h - '0' : h >= 'a' && h <= 'f' ? h - 'a' + 10 : h >= 'A' && h <= 'F' ? h - 'A' + 10 : (bad("bad hex digit"), 0));
                }
                if (v < 0x80) out.push_back(static_cast<char>(v));
                else if (v < 0x800) { out.push_back(static_cast<char>(0xC0 | (v >> 6))); out.push_back(static_cast<char>(0x80 | (v & 63))); }
                else { out.push_back(static_cast<char>(0xE0 | (v >> 12))); out.push_back(static_cast<char>(0x80 | ((v >> 6) & 63))); out.push_back(static_cast<char>(0x80 | (v & 63))); }
                break;
            }
            default: bad("bad escape");
            }
        }
    }
    JVal value() {
        if (++depth > 64) bad("nesting too deep");
        ws();
        if (p >= end) bad("unexpected end");
        JVal v;
        const char c = *p;
        if (c == '{') {
            v.t = JVal::Obj; ++p; ws();
            if (p < end && *p == '}') { ++p; --depth; return v; }
            while (true) {
                ws();
                if (p >= end || *p != '"') bad("expected a key");
                std::string k = str();
                ws();
                if (p >= end || *p != ':') bad("expected ':'");
                ++p;
                v.o.emplace_back(std::move(k), value());
                ws();
                if (p < end && *p == ',') { ++p; continue; }
                if (p < end && *p == '}') { ++p; break; }
                bad("expected ',' or '}'");
            }
        } else if (c == '[') {
            v.t = JVal::Arr; ++p; ws();
            if (p < end && *p == ']') { ++p; --depth; return v; }
            while (true) {
                v.a.push_back(value());
                ws();
                if (p < end && *p == ',') { ++p; continue; }
                if (p < end && *p == ']') { ++p; break; }
                bad("expected ',' or ']'");
            }
        } else if (c == '"') { v.t = JVal::Str; v.s = str(); }
        else if (c == 't') { lit("true"); v.t = JVal::Bool; v.b = true; }
        else if (c == 'f') { lit("false"); v.t = JVal::Bool; }
        else if (c == 'n') { lit("null"); }
        else {
            // RFC 8259 number grammar only: strtod alone would also take "inf", "nan", hex floats and leading '+'
            const char* q = p;
            if (q < end && *q == '-') ++q;
            if (q >= end || *q < '0' || *q > '9') bad("unexpected character");
            if (*q == '0') ++q; else while (q < end && *q >= '0' && *q <= '9') ++q;
            if (q < end && *q == '.') { ++q; if (q >= end || *q < '0' || *q > '9') bad("bad number"); while (q < end && *q >= '0' && *q <= '9') ++q; }
            if (q < end && (*q == 'e' || *q == 'E')) {
                ++q;
                if (q < end && (*q == '+' || *q == '-')) ++q;
                if (q >= end || *q < '0' || *q > '9') bad("bad number");
                while (q < end && *q >= '0' && *q <= '9') ++q;
            }
            if (q - p > 64) bad("number too long");
            const std::string tmp(p, static_cast<size_t>(q - p));
            v.n = std::strtod(tmp.c_str(), nullptr);
            if (!std::isfinite(v.n)) bad("number out of range");
            p = q;
            v.t = JVal::Num;
        }
        --depth;
        return v;
    }
};
JVal parse_json(const uint8_t* buf, size_t n) {
    JParser P{reinterpret_cast<const char*>(buf), reinterpret_cast<const char*>(buf) + n};
    JVal v = P.value();
    P.ws();
    if (P.p != P.end) P.bad("trailing characters");
    return v;
}
// Which coder `encode` hands a preset to (IFHIP_ENCODE_CODER_*): the object forms by their key, in the order `encode` asks;
// EncoderPreset::WebPLossless is a unit variant, so its JSON is the string "webplossless".  Everything else -- "gif",
// "webplossy" in any form, lodepng, no preset -- is the raw BGRA container.
int encode_coder(const JVal* preset) {
    if (!preset) return IFHIP_ENCODE_CODER_RAW;
    if (preset->get("libjpeg_turbo")) return IFHIP_ENCODE_CODER_JPEG;
    if (preset->get("libpng")) return IFHIP_ENCODE_CODER_PNG;
    if (preset->get("pngquant")) return IFHIP_ENCODE_CODER_PNGQUANT;
    if (preset->get("mozjpeg")) return IFHIP_ENCODE_CODER_MOZJPEG;
    if (preset->t == JVal::Str && preset->s == "webplossless") return IFHIP_ENCODE_CODER_WEBP_LOSSLESS;
    return IFHIP_ENCODE_CODER_RAW;
}
int64_t want_int(const JVal& o, const char* key, const char* node) {
    const JVal* v = o.get(key);
    if (!v || v->t != JVal::Num || v->n != std::floor(v->n) || std::fabs(v->n) > 9007199254740992.0)
        raise(kInvalidJson, "InvalidJson: %s.%s must be an integer", node, key);
    return static_cast<int64_t>(v->n);
}
uint32_t want_u32(const JVal& o, const char* key, const char* node) {
    const int64_t v = want_int(o, key, node);
    if (v < 0 || v > 0x7fffffff) raise(kInvalidJson, "InvalidJson: %s.%s out of range", node, key);
    return static_cast<uint32_t>(v);
}

// imageflow_types::Color (lib.rs:807-824) + imageflow_helpers/src/colors.rs:36-61 -> Color32 0xAARRGGBB
uint32_t parse_color(const JVal* v, const char* node) {
    if (!v || v->is_null()) return 0u;
    if (v->t == JVal::Str) {
        if (v->s == "transparent") return 0u;
        if (v->s == "black") return 0xFF000000u;
        raise(kInvalidJson, "InvalidJson: %s: unknown colour '%s'", node, v->s.c_str());
    }
    const JVal* srgb = v->get("srgb");
    const JVal* hex = srgb ? srgb->get("hex") : nullptr;
    if (!hex || hex->t != JVal::Str) raise(kInvalidJson, "InvalidJson: %s: colour must be \"transparent\", \"black\" or {\"srgb\":{\"hex\":..}}", node);
    std::string s = hex->s;
    if (!s.empty() && s[0] == '#') s.erase(0, 1);
    if (s.size() == 3 || s.size() == 4) { std::string d; for (char c : s) { d.push_back(c); d.push_back(c); } s = d; }
    if (s.size() == 6) s += "FF";
    if (s.size() != 8) raise(kArgumentInvalid, "InvalidNodeParams: %s: bad colour '%s'", node, hex->s.c_str());
    uint32_t ch[4];
    for (int i = 0; i < 4; ++i) {
        char* e = nullptr;
        const std::string part = s.substr(static_cast<size_t>(2 * i), 2);
        ch[i] = static_cast<uint32_t>(std::strtoul(part.c_str(), &e, 16));
        if (e != part.c_str() + 2) raise(kArgumentInvalid, "InvalidNodeParams: %s: bad colour '%s'", node, hex->s.c_str());
    }
    return (ch[3] << 24) | (ch[0] << 16) | (ch[1] << 8) | ch[2];
}
// s::Color::Transparent, the enum value (a missing colour reads as it): the only colour create_canvas.rs:79-82 turns into a
// ReplaceSelf canvas -- an srgb colour whose alpha is 0 still makes a BlendWithMatte canvas
bool keyword_transparent(const JVal* v) { return !v || v->is_null() || (v->t == JVal::Str && v->s == "transparent"); }
int parse_filter(const JVal* v, int dflt) {                      // imageflow_types/src/lib.rs:144-205
    if (!v || v->is_null()) return dflt;
    static const std::pair<const char*, int> names[] = {
        {"robidoux_fast", 1}, {"robidoux", 2}, {"robidoux_sharp", 3}, {"ginseng", 4}, {"ginseng_sharp", 5}, {"lanczos", 6},
        {"lanczos_sharp", 7}, {"lanczos_2", 8}, {"lanczos_2_sharp", 9}, {"cubic", 11}, {"cubic_sharp", 12}, {"catmull_rom", 13},
        {"mitchell", 14}, {"cubic_b_spline", 15}, {"hermite", 16}, {"jinc", 17}, {"triangle", 22}, {"linear", 23}, {"box", 24},
        {"fastest", 27}, {"n_cubic", 29}, {"n_cubic_sharp", 30}};
    if (v->t == JVal::Str)
        for (const auto& kv : names) if (v->s == kv.first) return kv.second;
    raise(kInvalidJson, "InvalidJson: unknown filter");
}


// JVal -> text: command_string.watermarks goes to the querystring expansion as text, and every number reads back as itself
void to_json(const JVal& v, std::string* o) {
    switch (v.t) {
    case JVal::Null: *o += "null"; break;
    case JVal::Bool: *o += v.b ? "true" : "false"; break;
    case JVal::Num: { char buf[40]; std::snprintf(buf, sizeof buf, "%.17g", v.n); *o += buf; break; }
    case JVal::Str:
        o->push_back('"');
        for (unsigned char ch : v.s) {
            if (ch == '"' || ch == '\\') { o->push_back('\\'); o->push_back(static_cast<char>(ch)); }
            else if (ch < 0x20) { char buf[8]; std::snprintf(buf, sizeof buf, "\\u%04x", ch); *o += buf; }
            else o->push_back(static_cast<char>(ch));
        }
        o->push_back('"');
        break;
    case JVal::Arr:
        o->push_back('[');
        for (size_t i = 0; i < v.a.size(); ++i) { if (i) o->push_back(','); to_json(v.a[i], o); }
        o->push_back(']');
        break;
    case JVal::Obj:
        o->push_back('{');
        for (size_t i = 0; i < v.o.size(); ++i) { if (i) o->push_back(','); to_json(JVal{JVal::Str, false, 0, v.o[i].first, {}, {}}, o); o->push_back(':'); to_json(v.o[i].second, o); }
        o->push_back('}');
        break;
    }
}

std::string json_escape(const std::string& s) {
    std::string o;
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') { o.push_back('\\'); o.push_back(static_cast<char>(c)); }
        else if (c == '\n') o += "\\n";
        else if (c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o.push_back(static_cast<char>(c));
    }
    return o;
}

}  // namespace ifshim
