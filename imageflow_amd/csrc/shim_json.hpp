// shim_json.hpp -- the ABI shim's JSON reader and the parameter readers behind it (shim_json.cpp): what takes bytes straight from
// an untrusted caller.  Standard library, shim_errors.hpp and the IFHIP_ENCODE_CODER_* constants only -- no GPU runtime -- so
// that tests/shim_json_check.cpp runs it in a program of its own under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "shim_errors.hpp"

namespace ifshim {

struct JVal {
    enum T { Null, Bool, Num, Str, Arr, Obj } t = Null;
    bool b = false;
    double n = 0;
    std::string s;
    std::vector<JVal> a;
    std::vector<std::pair<std::string, JVal>> o;
    const JVal* get(const char* k) const {
        if (t != Obj) return nullptr;
        for (const auto& kv : o) if (kv.first == k) return &kv.second;
        return nullptr;
    }
    bool is_null() const { return t == Null; }
};
// RFC 8259, with three limits of its own: nesting at most 64 deep, a number of at most 64 characters, a finite double
JVal parse_json(const uint8_t* buf, size_t n);
// JVal -> text: command_string.watermarks goes to the querystring expansion as text, and every number reads back as itself
void to_json(const JVal& v, std::string* o);
std::string json_escape(const std::string& s);                   // the inside of a JSON string, for the responses

// ---- what nodes read their parameters with ----------------------------------------------------------------------------------
int encode_coder(const JVal* preset);                            // IFHIP_ENCODE_CODER_*
int64_t want_int(const JVal& o, const char* key, const char* node);
uint32_t want_u32(const JVal& o, const char* key, const char* node);
uint32_t parse_color(const JVal* v, const char* node);           // -> Color32 0xAARRGGBB
bool keyword_transparent(const JVal* v);
int parse_filter(const JVal* v, int dflt);

}  // namespace ifshim
