// gif_decode_emulate.cpp -- csrc/gif_read.cpp and csrc/gif_decode_core.hpp on the CPU: the container walk as the library runs
// it, the batch's block laid out by gif_layout_batch with exactly the sizes the device entry allocates, and the five launches
// as loops (the wave's ballot over 64 lanes, the workgroup's 256 threads between barriers) -- an access outside the block's
// bounds is a finding of the sanitizer build.  Built by tests/test_gif_decode_core.py with g++ (and with ASan + UBSan).
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/gif_read.cpp"
#include "../imageflow_amd/csrc/gif_decode_core.hpp"

namespace ifhip {
int fail(int status, const char*, ...) { return status; }
}  // namespace ifhip

using namespace ifhip;

extern "C" {

// One file, frame `target` -> BGRA rows of 4 * w bytes (at most `cap` bytes); returns the status word, kGifDecContainer where
// the header does not parse.  *w, *h: the logical screen; *frames: the frames the walk saw.
uint32_t gif_dec_emu_decode(const uint8_t* file, size_t len, uint32_t target, uint8_t* bgra, uint64_t cap, uint32_t* w, uint32_t* h, uint32_t* frames, uint32_t grid_x) {
    GifParsed P;
    *w = *h = *frames = 0;
    if (parse_gif(file, len, target, &P) != 0 || !P.w || !P.h) return kGifDecContainer;
    *w = P.w; *h = P.h; *frames = static_cast<uint32_t>(P.frames.size());
    if (static_cast<uint64_t>(P.w) * P.h * 4u > cap) return kGifDecContainer;
    const GifParsed* files[1] = {&P};
    uint8_t* out[1] = {bgra};
    const uint32_t strides[1] = {4u * P.w};
    GifLayout L;
    gif_layout_batch(files, 1, out, strides, &L);
    uint8_t* block = static_cast<uint8_t*>(std::malloc(L.total ? L.total : 1));
    std::memset(block + L.blob.size(), 0xA5, L.total - L.blob.size());      // the scratch is not cleared on the device either
    uint32_t status = 0;
    gif_decode_batch_cpu(L, 1, block, &status, grid_x ? grid_x : 1u);
    std::free(block);
    return status;
}

}  // extern "C"

#ifdef GIF_DEC_EMU_MAIN
// The sanitizer build: files from a file (u32 len, u32 target, bytes), a line "status w h sum" per case.
#include <cstdio>
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[2];
    while (std::fread(head, 4, 2, f) == 2) {
        std::vector<uint8_t> src(head[0] ? head[0] : 1);
        if (head[0] && std::fread(src.data(), 1, head[0], f) != head[0]) return 3;
        std::vector<uint8_t> out(4u << 20);
        uint32_t w = 0, h = 0, frames = 0;
        const uint32_t st = gif_dec_emu_decode(src.data(), head[0], head[1], out.data(), out.size(), &w, &h, &frames, 3);
        uint32_t sum = 0;
        if (!st) for (size_t i = 0; i < static_cast<size_t>(w) * h; ++i) { uint32_t v; std::memcpy(&v, out.data() + 4u * i, 4); sum = sum * 0x01000193u ^ v; }
        std::printf("%u %u %u %u\n", st, st ? 0u : w, st ? 0u : h, sum);
    }
    std::fclose(f);
    return 0;
}
#endif
