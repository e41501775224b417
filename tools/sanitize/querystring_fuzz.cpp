// Querystrings with random damage through ifhip_shim_expand_command_string, under the sanitizers: the form decoding, the
// Instructions parser, the colour reader, the layout arithmetic (every float-to-integer cast) and the watermark splitter.
// Host code only: links csrc/querystring.cpp, csrc/layout.cpp and stubs.cpp.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "imageflow_abi_subset.h"
#include "imageflow_hip.h"

namespace ifhip { const char* last_error(); }                                             // stubs.cpp; api.cpp's accessor is not linked here
extern "C" const char* ifhip_last_error_message(void) { return ifhip::last_error(); }

static long g_ok = 0, g_layout = 0, g_refused = 0, g_invalid = 0;
static void feed(const std::string& qs, int w, int h, int rw, int rh, const char* marks) {
    std::vector<char> out(static_cast<size_t>(rand() % 3 == 0 ? rand() % 64 : 4096));
    size_t needed = 0;
    const int rc = ifhip_shim_expand_command_string(qs.c_str(), w, h, rw, rh, marks, out.data(), out.size(), &needed);
    if (rc == 0) { ++g_ok; if (needed <= out.size() && std::strlen(out.data()) + 1 != needed) { printf("length mismatch for %s\n", qs.c_str()); exit(1); } }
    else { (rc == 1 ? g_layout : rc == 2 ? g_refused : g_invalid)++; if (!ifhip_last_error_message()[0]) { printf("no message for %s\n", qs.c_str()); exit(1); } }
}
int main() {
    srand(7);
    const std::string seeds[] = {
        "w=170&h=220&mode=crop&scale=both&crop=449,0,-472,0&anchor=bottomright&c.gravity=20,80",
        "width=80&height=80&bgcolor=%23aaeeff80&srotate=90&sflip=xy&rotate=270&flip=y&zoom=1.5x&watermark_red_dot=true",
        "c=10,10,90,90&s.alpha=.5&s.brightness=.1&s.contrast=-.2&s.saturation=.3&s.sepia=true&s.grayscale=bt709&f.sharpen=15&f.sharpen_when=always",
        "maxwidth=40&maxheight=30&up.filter=ginseng&down.filter=lanczos_2_sharp&up.colorspace=srgb&down.colorspace=gamma&decoder.min_precise_scaling_ratio=3&ignoreicc=1",
        "crop=(1,2,3,4)&cropxunits=100&cropyunits=0&anchor=25.5,99&mode=aspectcrop&stretch=fill&dpr=2&dppx=3&s.roundcorners=1,2,3,4&a.balancewhite=area&trim.threshold=80",
        "h=-100&maxwidth=2&mode=crop&bgcolor=LightSlateGray&scale=canvas&autorotate=true&quality=90&format=jpg&jpeg.quality=5&trim.percentpadding=.5"};
    const char* marks[] = {nullptr, "null", "[]", "[{\"io_id\":2,\"fit_box\":{\"canvas_margins\":{\"left\":1,\"top\":1,\"right\":1,\"bottom\":1}}},{\"io_id\":3,\"fit_box\":null,\"hints\":{\"a\":[1,\"x\\\"]\"]}}]",
                           "[{\"io_id\":2,\"fit_box\":{\"image_percentage\"", "[{]", "{", "[1,2]", "[{\"fit_box\":{\"canvas_percentage\":{}}},", "[{\"\\"};
    auto side = [] { const int r = rand() % 20; return r == 0 ? 0 : r == 1 ? -5 : r == 2 ? 2147483647 : 1 + rand() % 3000; };
    for (int it = 0; it < 60000; ++it) {
        std::string m = seeds[rand() % 6];
        const int muts = rand() % 6;
        for (int k = 0; k < muts; ++k) {
            const size_t at = static_cast<size_t>(rand()) % m.size();
            switch (rand() % 5) {
            case 0: m[at] = static_cast<char>(rand()); break;                            // any byte, 0 and the non-ASCII ones included
            case 1: m[at] = "0123456789,.-+eEx%&=#()"[rand() % 23]; break;
            case 2: m.insert(at, std::to_string(rand() % 2 ? rand() : -rand()) + std::string(static_cast<size_t>(rand() % 40), '9')); break;   // overlong numbers
            case 3: m.erase(at, static_cast<size_t>(rand() % 8)); break;
            default: m.insert(at, "%"); break;
            }
            if (m.empty()) m = "w";
        }
        if (rand() % 6 == 0) m.resize(1 + static_cast<size_t>(rand()) % m.size());          // truncated, maybe inside a %XX
        if (rand() % 40 == 0) m += "%";                                                   // '%' at the end of the string
        const int w = side(), h = side();
        const bool reduced = rand() % 3 == 0;
        feed(m, w, h, reduced ? side() : w, reduced ? side() : h, marks[rand() % 10]);
    }
    // the cases named in the issue that random damage meets too rarely
    feed("crop=" + std::string(10000, ','), 100, 50, 100, 50, nullptr);
    feed("c=1" + std::string(10000, ',') + "2&anchor=" + std::string(5000, ',') + "&s.roundcorners=" + std::string(9999, ','), 100, 50, 100, 50, nullptr);
    feed("w=" + std::string(5000, '9') + "&zoom=" + std::string(400, '9') + "e" + std::string(300, '9') + "&rotate=1" + std::string(600, '0'), 100, 50, 100, 50, nullptr);
    feed("s.alpha=0." + std::string(3000, '1') + "&cropxunits=1e-400&crop=1e308,1e308,-1e308,-1e308&c.gravity=nan,inf", 100, 50, 800, 400, nullptr);
    for (const char* tail : {"w=5&bgcolor=%", "w=5&bgcolor=%2", "w=5&bgcolor=%23", "%", "%=%", "w=%zz&h=%4", "bgcolor=\xC3\xA9\xC3\xA9\xC3\xA9", "bgcolor=\xE2\x82\xAC" "fff",
                             "bgcolor=%C3%A9ff", "bgcolor=#", "bgcolor=%23%23", "bgcolor=+ff", "bgcolor=+fffff", "bgcolor=\xFF", "=&=&&&=", "&", ""})
        feed(tail, 100, 50, 100, 50, nullptr);
    std::string deep = "[";
    for (int k = 0; k < 200; ++k) deep += "{\"a\":[";
    feed("w=5", 100, 50, 100, 50, deep.c_str());
    printf("querystrings: %ld expanded, %ld layout errors, %ld refused, %ld invalid\n", g_ok, g_layout, g_refused, g_invalid);
    return g_ok > 1000 && g_refused > 1000 ? 0 : 1;
}
