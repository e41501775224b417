// vp8_decode_emulate.cpp -- the lossy WebP decoder without a device: the host stage as the library runs it
// (csrc/vp8_read.cpp) and the functions of csrc/vp8_decode_core.hpp in the kernels' schedules -- the residuals block by
// block, prediction and loop filter as wavefronts of skew 2 over the macroblocks (macroblock (x, y) in step x + 2y, every
// lane's rows before every lane's columns), the alpha plane un-filtered, the frame converted pixel by pixel.  The VP8L-coded
// alpha plane goes through tests/webp_decode_emulate.cpp behind the five header bytes the ALPH chunk leaves out.
// Built by tests/test_vp8_decode_core.py with g++ (and with ASan + UBSan): every buffer here has exactly the size the device
// entry gives its kernels, so an access outside the bounds is a finding.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/vp8_read.cpp"
#include "webp_decode_emulate.cpp"

using namespace ifhip;

extern "C" {

// The `VP8 ` chunk's bytes and the `ALPH` chunk's (null: none) -> BGRA dwords, w * h of them at most `cap`; the status word.
uint32_t vp8_emu_decode(const uint8_t* vp8, uint32_t vp8_len, const uint8_t* alph, uint32_t alph_len, uint32_t* bgra, uint64_t cap, uint32_t* w, uint32_t* h) {
    std::vector<uint8_t> in(vp8, vp8 + vp8_len), al(alph ? alph : vp8, alph ? alph + alph_len : vp8);   // exact sizes
    Vp8Frame F;
    if (vp8_read_frame(in.data(), in.size(), &F)) return F.status;
    if (alph && vp8_read_alpha(al.data(), al.size(), &F)) return F.status;
    *w = F.w; *h = F.h;
    const size_t n_mb = static_cast<size_t>(F.mbw) * F.mbh;
    for (size_t m = 0; m < n_mb; ++m)
        for (uint32_t b = 0; b < 24u; ++b) vp8_residual_mb_block(F.levels.data() + m * kVp8MbLevels, F.mbs[m], F.quant[F.mbs[m].segment], b);
    std::vector<uint8_t> Y(n_mb * 256u), U(n_mb * 64u), V(n_mb * 64u);
    const Vp8Planes P = {Y.data(), U.data(), V.data(), F.mbw * 16u, F.mbw * 8u, F.mbw, F.mbh};
    const uint32_t steps = F.mbw + 2u * (F.mbh - 1u);
    for (uint32_t s = 0; s < steps; ++s)
        for (uint32_t y = 0; y < F.mbh && 2u * y <= s; ++y) {
            const uint32_t x = s - 2u * y;
            if (x >= F.mbw) continue;
            const size_t m = static_cast<size_t>(y) * F.mbw + x;
            for (uint32_t lane = 0; lane < 64u; ++lane) vp8_predict_mb(P, F.mbs[m], F.levels.data() + m * kVp8MbLevels, x, y, lane, 64u);
        }
    if (F.filter != kVp8FilterNone)
        for (uint32_t s = 0; s < steps; ++s)
            for (int vertical = 0; vertical < 2; ++vertical)
                for (uint32_t y = 0; y < F.mbh && 2u * y <= s; ++y) {
                    const uint32_t x = s - 2u * y;
                    if (x >= F.mbw) continue;
                    for (uint32_t lane = 0; lane < 32u; ++lane) vp8_filter_mb_line(P, F.mbs[static_cast<size_t>(y) * F.mbw + x], F.filter, x, y, lane, vertical != 0);
                }
    std::vector<uint8_t> A;
    if (F.alpha_kind != kVp8AlphaNone) {
        A.resize(static_cast<size_t>(F.w) * F.h);
        std::vector<uint32_t> argb;
        if (F.alpha_kind == kVp8AlphaVp8l) {
            const uint32_t head = (F.w - 1u) | (F.h - 1u) << 14;
            std::vector<uint8_t> full = {0x2F, static_cast<uint8_t>(head), static_cast<uint8_t>(head >> 8), static_cast<uint8_t>(head >> 16), static_cast<uint8_t>(head >> 24)};
            full.insert(full.end(), F.alpha_data, F.alpha_data + F.alpha_len);
            argb.resize(A.size());
            uint32_t ww = 0, hh = 0, aa = 0;
            if (webp_dec_emu_decode(full.data(), static_cast<uint32_t>(full.size()), argb.data(), argb.size(), &ww, &hh, &aa)) return kVp8DecAlphaStream;
        }
        for (uint32_t y = 0; y < F.h; ++y)
            for (uint32_t x = 0; x < F.w; ++x) {
                const size_t i = static_cast<size_t>(y) * F.w + x;
                const uint32_t coded = F.alpha_kind == kVp8AlphaVp8l ? (argb[i] >> 8) & 255u : F.alpha_data[i];
                A[i] = static_cast<uint8_t>(coded + vp8_alpha_predict(F.alpha_filter, x, y, x ? A[i - 1u] : 0u, y ? A[i - F.w] : 0u, x && y ? A[i - F.w - 1u] : 0u));
            }
    }
    if (static_cast<uint64_t>(F.w) * F.h > cap) return kVp8DecOk;
    for (uint32_t y = 0; y < F.h; ++y)
        for (uint32_t x = 0; x < F.w; ++x) bgra[static_cast<size_t>(y) * F.w + x] = vp8_bgra_pixel(P, A.empty() ? nullptr : A.data(), F.w, F.h, x, y);
    return kVp8DecOk;
}

}  // extern "C"

#ifdef VP8_DEC_EMU_MAIN
// The sanitizer build: cases from a file (u32 vp8_len, u32 alph_len or 0xFFFFFFFF for none, bytes), a line "status w h sum" per case.
#include <cstdio>
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t len[2];
    while (std::fread(len, 4, 2, f) == 2) {
        const bool has = len[1] != 0xFFFFFFFFu;
        std::vector<uint8_t> a(len[0] ? len[0] : 1), b(has && len[1] ? len[1] : 1);
        if (len[0] && std::fread(a.data(), 1, len[0], f) != len[0]) return 3;
        if (has && len[1] && std::fread(b.data(), 1, len[1], f) != len[1]) return 3;
        std::vector<uint32_t> out(1u << 20);
        uint32_t w = 0, h = 0;
        const uint32_t st = vp8_emu_decode(a.data(), len[0], has ? b.data() : nullptr, has ? len[1] : 0u, out.data(), out.size(), &w, &h);
        uint32_t sum = 0;
        if (!st) for (size_t i = 0; i < static_cast<size_t>(w) * h; ++i) sum = sum * 0x01000193u ^ out[i];
        std::printf("%u %u %u %u\n", st, st ? 0u : w, st ? 0u : h, sum);
    }
    std::fclose(f);
    return 0;
}
#endif
