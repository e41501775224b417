// The GIF decoder on mutated files, on the CPU: the container walk (csrc/gif_read.cpp) and the batch as the device runs it --
// the scan, lengths, places, resolve and compose of csrc/gif_decode_core.hpp over a block of exactly the size the device entry
// allocates -- under ASan + UBSan.  A stand-alone program: files in argv, built and run by tools/sanitize/run.sh.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gif_decode_core.hpp"
#include "gif_read.hpp"

using namespace ifhip;

static std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> d;
    if (FILE* f = std::fopen(path, "rb")) { uint8_t buf[4096]; size_t n; while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n); std::fclose(f); }
    return d;
}

int main(int argc, char** argv) {
    srand(7);
    size_t runs = 0, parsed = 0, walked = 0, decoded = 0;
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> file = read_file(argv[a]);
        if (file.size() < 20) continue;
        const int iterations = file.size() > 20000 ? 60 : 600;
        for (int it = 0; it < iterations; ++it) {
            std::vector<uint8_t> m = file;
            const int muts = it ? 1 + rand() % 5 : 0;
            for (int k = 0; k < muts; ++k) {
                const size_t at = (rand() % 3) ? rand() % (m.size() < 120 ? m.size() : 120) : rand() % m.size();     // mostly the head: screen, tables, descriptors
                if (rand() % 2) m[at] = (uint8_t)rand(); else m[at] ^= (uint8_t)(1u << (rand() % 8));
            }
            if (rand() % 8 == 0) m.resize(6 + rand() % (m.size() - 6));
            ++runs;
            GifParsed P;
            const uint32_t target = static_cast<uint32_t>(rand() % 4);
            if (parse_gif(m.data(), m.size(), target, &P) != 0 || !P.w || !P.h) continue;
            ++parsed;
            if (static_cast<uint64_t>(P.w) * P.h > (1u << 20)) continue;       // (a mutated screen: the frame alone would be gigabytes)
            if (!P.status) ++walked;
            std::vector<uint8_t> frame(static_cast<size_t>(P.w) * P.h * 4u);
            const GifParsed* files[1] = {&P};
            uint8_t* frames[1] = {frame.data()};
            const uint32_t strides[1] = {4u * P.w};
            GifLayout L;
            gif_layout_batch(files, 1, frames, strides, &L);
            std::vector<uint8_t> block(L.total ? L.total : 1, 0xA5);
            uint32_t status = 0;
            gif_decode_batch_cpu(L, 1, block.data(), &status, 1u + static_cast<uint32_t>(rand() % 5));
            if (!status) ++decoded;
        }
    }
    std::printf("gif_fuzz: %zu mutated files, %zu with a header, %zu passed the container walk, %zu decoded; no sanitizer report\n", runs, parsed, walked, decoded);
    return 0;
}
