// Encoder selection under the sanitizers: querystrings with damaged output keys through ifhip_shim_querystring_encoder_preset
// (the reference's parsers of format, qp, qp.dpr, lossless, accept.*, jpeg.*, webp.*, png.*), what they make and damaged
// `auto` / `format` presets through ifhip_shim_resolve_encoder_preset (serde's readers, the quality tables with every
// float-to-u8 cast, the resolution).  Host code only: links csrc/encoder_select.cpp, querystring.cpp, layout.cpp,
// shim_json.cpp and stubs.cpp.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "imageflow_hip_encoder_select.h"
#include "imageflow_hip.h"

namespace ifhip { const char* last_error(); }                                             // stubs.cpp; api.cpp's accessor is not linked here
extern "C" const char* ifhip_last_error_message(void) { return ifhip::last_error(); }

static long g_presets = 0, g_resolved = 0, g_refused = 0, g_invalid = 0;
static void resolve(const std::string& json) {
    std::vector<char> out(static_cast<size_t>(rand() % 3 == 0 ? rand() % 64 : 4096));
    size_t needed = 0;
    const int rc = ifhip_shim_resolve_encoder_preset(json.data(), json.size(), rand() % 5, rand() % 2, static_cast<uint32_t>(rand() % 4), rand() % 2,
                                                     1u + static_cast<uint32_t>(rand() % 4000), 1u + static_cast<uint32_t>(rand() % 4000), out.data(), out.size(), &needed);
    if (rc == 0) { ++g_resolved; if (needed <= out.size() && std::strlen(out.data()) + 1 != needed) { printf("length mismatch for %s\n", json.c_str()); exit(1); } }
    else { ++g_invalid; if (!ifhip_last_error_message()[0]) { printf("no message for %s\n", json.c_str()); exit(1); } }
}
static void damage(std::string* m) {
    const int muts = rand() % 5;
    for (int k = 0; k < muts; ++k) {
        const size_t at = static_cast<size_t>(rand()) % m->size();
        switch (rand() % 5) {
        case 0: (*m)[at] = static_cast<char>(rand()); break;
        case 1: (*m)[at] = "0123456789,.-+eEx%&=:{}[]\"nul"[rand() % 29]; break;
        case 2: m->insert(at, std::to_string(rand() % 2 ? rand() : -rand()) + std::string(static_cast<size_t>(rand() % 40), '9')); break;
        case 3: m->erase(at, static_cast<size_t>(rand() % 8)); break;
        default: m->insert(at, rand() % 2 ? "1e39" : "-0.5"); break;
        }
        if (m->empty()) *m = "q";
    }
}
int main() {
    srand(11);
    const std::string strings[] = {
        "format=png&png.quality=80&png.min_quality=20&png.quantization_speed=3&png.libpng=0&png.max_deflate=1&png.lossless=keep",
        "qp=good&qp.dpr=1.5x&accept.webp=1&accept.avif=true&accept.jxl=no&accept.color_profiles=on&lossless=preserve",
        "thumbnail=jfif&quality=70&jpeg.quality=55&jpeg.progressive=true&jpeg.turbo=1&jpeg.li=0&w=40",
        "format=webp&webp.quality=66.5&webp.lossless=false&qp=37.5&qp.dppx=zoom&zoom=2x",
        "format=auto&quality=80&qp=quality&qp.dpr=12"};
    const std::string presets[] = {
        "{\"auto\":{\"quality_profile\":{\"percent\":64.5},\"quality_profile_dpr\":2,\"matte\":{\"srgb\":{\"hex\":\"#abcf\"}},\"lossless\":\"keep\",\"allow\":{\"web_safe\":true,\"webp\":true}}}",
        "{\"format\":{\"format\":\"png\",\"quality_profile\":\"good\",\"quality_profile_dpr\":0.5,\"matte\":\"black\",\"lossless\":\"false\",\"allow\":{\"all\":true},"
        "\"encoder_hints\":{\"png\":{\"quality\":80,\"min_quality\":20,\"quantization_speed\":3,\"mimic\":\"pngquant\",\"hint_max_deflate\":true,\"lossless\":\"keep\"},"
        "\"jpeg\":{\"quality\":90,\"progressive\":true,\"mimic\":\"libjpegturbo\"},\"webp\":{\"quality\":75.5,\"lossless\":\"true\"},\"gif\":{}}}}",
        "{\"format\":{\"format\":\"keep\",\"quality_profile\":{\"percent\":12},\"quality_profile_dpr\":20,\"allow\":{\"modern_web_safe\":true}}}"};
    for (int it = 0; it < 40000; ++it) {
        std::string m = strings[rand() % 5];
        damage(&m);
        if (rand() % 6 == 0) m.resize(1 + static_cast<size_t>(rand()) % m.size());
        std::vector<char> out(8192);
        size_t needed = 0;
        const int rc = ifhip_shim_querystring_encoder_preset(m.c_str(), out.data(), out.size(), &needed);
        if (rc == 0) { ++g_presets; resolve(out.data()); }                               // what the querystring layer makes always reads
        else { ++g_refused; if (!ifhip_last_error_message()[0]) { printf("no message for %s\n", m.c_str()); exit(1); } }
        std::string p = presets[rand() % 3];
        damage(&p);
        if (rand() % 8 == 0) p.resize(1 + static_cast<size_t>(rand()) % p.size());
        resolve(p);
    }
    for (const char* s : {"qp.dpr=nan&qp=good", "qp.dpr=inf&qp=good", "qp.dpr=-inf&qp=1e39", "qp=-nan", "qp.dpr=1e-50x&qp=low", "quality=-2147483648&qp=quality",
                          "png.quality=+255", "png.quality=0256", "webp.quality=1e39", "format=", "qp.dpr=xxxx", "qp.dpr=x"}) {
        std::vector<char> out(8192);
        size_t needed = 0;
        if (ifhip_shim_querystring_encoder_preset(s, out.data(), out.size(), &needed) == 0) { ++g_presets; resolve(out.data()); }
    }
    for (const char* p : {"{\"auto\":{\"quality_profile\":{\"percent\":1e308},\"quality_profile_dpr\":1e308}}", "{\"auto\":{\"quality_profile\":{\"percent\":-1e308},\"quality_profile_dpr\":-1e308}}",
                          "{\"format\":{\"format\":\"webp\",\"encoder_hints\":{\"webp\":{\"quality\":1e300}}}}", "{\"format\":{\"format\":\"jpeg\",\"encoder_hints\":{\"jpeg\":{\"quality\":-1e300}}}}",
                          "{\"auto\":{\"quality_profile\":{\"percent\":1e-320},\"quality_profile_dpr\":1e-320}}"})
        resolve(p);
    printf("encoder selection: %ld presets from querystrings, %ld resolved, %ld querystrings refused, %ld presets refused\n", g_presets, g_resolved, g_refused, g_invalid);
    return g_presets > 1000 && g_resolved > 1000 && g_invalid > 1000 ? 0 : 1;
}
