// webp_decode_emulate.cpp -- csrc/webp_decode_core.hpp on the CPU: the host prepare as the library runs it, the main image's
// token loop with the executor's wave-wide parts as loops over 64 lanes, and the inverse transforms in the kernels' order --
// the predictor in a second writing of webp_transform_kernel's skewed schedule (lane r two pixels behind lane r - 1, the
// three upper neighbours handed down between lanes): this checks the schedule's arithmetic, the kernel's own loop is the GPU tests'.
// Built by tests/test_webp_decode_core.py with g++ (and with ASan + UBSan): every buffer here has exactly the size the device entry gives its kernels, so an access outside the bounds is a finding.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/webp_decode_core.hpp"

using namespace ifhip;

namespace {

void inverse_predictor(const uint32_t* src, uint32_t* dst, uint32_t w, uint32_t h, uint32_t bits, const uint32_t* tiles) {
    const uint32_t tiles_x = webp_subsample(w, bits), mask = (1u << bits) - 1u;
    for (uint32_t y0 = 0; y0 < h; y0 += kWebpLanes) {
        uint32_t prod[kWebpLanes] = {}, up[kWebpLanes], tr[kWebpLanes] = {}, tt[kWebpLanes] = {}, tl[kWebpLanes] = {}, left[kWebpLanes] = {}, first[kWebpLanes] = {}, mode[kWebpLanes] = {};
        if (y0) tr[0] = dst[static_cast<size_t>(y0 - 1u) * w];
        for (uint32_t t = 0; t < w + 2u * (kWebpLanes - 1u); ++t) {
            for (uint32_t r = 0; r < kWebpLanes; ++r) up[r] = r ? prod[r - 1u] : 0u;             // the lane shift, before anybody's step
            for (uint32_t r = 0; r < kWebpLanes; ++r) {
                const uint32_t x = t - 2u * r, y = y0 + r;
                const bool on = y < h && t >= 2u * r && x < w;
                uint32_t in = up[r];
                if (r == 0u) in = on && y && x + 1u < w ? dst[static_cast<size_t>(y - 1u) * w + x + 1u] : 0u;
                tl[r] = tt[r]; tt[r] = tr[r]; tr[r] = in;
                if (!on) continue;
                if ((x & mask) == 0u) mode[r] = webp_tile_mode(tiles[static_cast<size_t>(y >> bits) * tiles_x + (x >> bits)]);
                const uint32_t v = webp_add(src[static_cast<size_t>(y) * w + x], webp_predict_at(mode[r], x, y, left[r], tt[r], tl[r], x + 1u < w ? tr[r] : first[r]));
                dst[static_cast<size_t>(y) * w + x] = v;
                left[r] = v; prod[r] = v;
                if (x == 0u) first[r] = v;
            }
        }
    }
}

}  // namespace

extern "C" {

// A VP8L payload (the chunk's bytes) -> ARGB dwords, w * h of them at most `cap`; the status of webp_decode_core.hpp.
// The payload is copied into a buffer of exactly len rounded up to 16 bytes, as the device block holds it.
uint32_t webp_dec_emu_decode(const uint8_t* payload, uint32_t len, uint32_t* argb, uint64_t cap, uint32_t* w, uint32_t* h, uint32_t* alpha) {
    const size_t in_bytes = (static_cast<size_t>(len) + 15u) & ~static_cast<size_t>(15);
    uint8_t* in = static_cast<uint8_t*>(std::aligned_alloc(16, in_bytes ? in_bytes : 16));
    std::memset(in, 0, in_bytes ? in_bytes : 16);
    if (len) std::memcpy(in, payload, len);
    uint32_t status;
    {
        WebpHeadReader R(in, len);
        WebpPrepared P;
        status = R.prepare(&P);
        std::vector<uint32_t> a, b;
        if (!status) { *w = P.w; *h = P.h; *alpha = P.alpha; status = R.main_image(P, &a, nullptr); }
        if (!status) {
            uint32_t cur_w = P.xsize;
            for (uint32_t k = P.n_transforms; k-- > 0u;) {
                const WebpTransform& T = P.t[k];
                b.assign(static_cast<size_t>(T.xsize) * P.h, 0u);
                if (T.kind == 0u) inverse_predictor(a.data(), b.data(), T.xsize, P.h, T.bits, T.data.data());
                else
                    for (uint32_t y = 0; y < P.h; ++y)
                        for (uint32_t x = 0; x < T.xsize; ++x) {
                            const size_t i = static_cast<size_t>(y) * T.xsize + x;
                            if (T.kind == 1u) b[i] = webp_cross_color(a[i], T.data[static_cast<size_t>(y >> T.bits) * webp_subsample(T.xsize, T.bits) + (x >> T.bits)]);
                            else if (T.kind == 2u) b[i] = webp_add_green(a[i]);
                            else b[i] = webp_index_pixel(a.data() + static_cast<size_t>(y) * cur_w, x, T.bits, T.data.data(), static_cast<uint32_t>(T.data.size()));
                        }
                a.swap(b);
                cur_w = T.xsize;
            }
            if (static_cast<uint64_t>(P.w) * P.h <= cap) std::memcpy(argb, a.data(), a.size() * 4u);
        }
    }
    std::free(in);
    return status;
}

}  // extern "C"

#ifdef WEBP_DEC_EMU_MAIN
// The sanitizer build: payloads from a file (u32 len, bytes), a line "status w h crc32-like sum" per case.
#include <cstdio>
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t len;
    while (std::fread(&len, 4, 1, f) == 1) {
        std::vector<uint8_t> src(len ? len : 1);
        if (len && std::fread(src.data(), 1, len, f) != len) return 3;
        std::vector<uint32_t> out(1u << 20);
        uint32_t w = 0, h = 0, alpha = 0;
        const uint32_t st = webp_dec_emu_decode(src.data(), len, out.data(), out.size(), &w, &h, &alpha);
        uint32_t sum = 0;
        if (!st) for (size_t i = 0; i < static_cast<size_t>(w) * h; ++i) sum = sum * 0x01000193u ^ out[i];
        std::printf("%u %u %u %u\n", st, st ? 0u : w, st ? 0u : h, sum);
    }
    std::fclose(f);
    return 0;
}
#endif
