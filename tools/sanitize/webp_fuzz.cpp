// The host side of the WebP decoder on mutated files: the RIFF walk (csrc/webp_read.cpp), the prepare of the stream and the
// main image's token loop as the device runs it (csrc/webp_decode_core.hpp), under ASan + UBSan.  Files: argv.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "webp_decode_core.hpp"
#include "webp_read.hpp"

using namespace ifhip;

static std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> d;
    if (FILE* f = std::fopen(path, "rb")) { uint8_t buf[4096]; size_t n; while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n); std::fclose(f); }
    return d;
}

int main(int argc, char** argv) {
    srand(5);
    size_t runs = 0, parsed = 0, prepared = 0, decoded = 0;
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> file = read_file(argv[a]);
        if (file.size() < 32) continue;
        for (int it = 0; it < 2000; ++it) {
            std::vector<uint8_t> m = file;
            const int muts = it ? 1 + rand() % 5 : 0;
            for (int k = 0; k < muts; ++k) {
                const size_t at = (rand() % 3) ? rand() % (m.size() < 120 ? m.size() : 120) : rand() % m.size();     // mostly the head: container, header, codes
                if (rand() % 2) m[at] = (uint8_t)rand(); else m[at] ^= (uint8_t)(1u << (rand() % 8));
            }
            if (rand() % 8 == 0) m.resize(12 + rand() % (m.size() - 12));
            ++runs;
            WebpParsed P;
            if (parse_webp_for_decode(m.data(), m.size(), &P) != 0) continue;
            ++parsed;
            if (static_cast<uint64_t>(P.w) * P.h > (1u << 21)) continue;       // (a mutated size: the image alone would be gigabytes)
            WebpJob J;
            webp_prepare_job(P, &J);
            if (J.status) continue;
            ++prepared;
            WebpHeadReader R(reinterpret_cast<const uint8_t*>(J.prepared->payload.data()), static_cast<uint32_t>(P.payload_len));
            std::vector<uint32_t> out;
            if (R.main_image(*J.prepared, &out, nullptr) == 0) ++decoded;
        }
    }
    std::printf("webp_fuzz: %zu mutated files, %zu passed the container walk, %zu the prepare, %zu the token loop; no sanitizer report\n", runs, parsed, prepared, decoded);
    return 0;
}
