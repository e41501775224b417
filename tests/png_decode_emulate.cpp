// png_decode_emulate.cpp -- csrc/png_decode_core.hpp on the CPU, lane by lane: the inflate with the executor's wave-wide parts as
// loops over 64 lanes, and the un-filter in the kernel's skewed schedule (lane r one pixel behind lane r - 1, the three
// neighbours handed over between lanes).  Built by tests/test_png_decode_core.py with g++ (and with ASan + UBSan): every
// buffer here has exactly the size the device entry gives its kernels, so an access outside the bounds is a finding.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../imageflow_amd/csrc/png_decode_core.hpp"

using namespace ifhip;

namespace {
struct HostExec {
    template <typename F> void lanes(F f) { for (uint32_t lane = 0; lane < kInfLanes; ++lane) f(lane); }
    template <typename F> void one(F f) { f(); }
    void sync() {}
};
uint8_t* aligned_bytes(size_t n) {            // exactly n bytes (a multiple of 16), 16-byte aligned
    return static_cast<uint8_t*>(std::aligned_alloc(16, n ? n : 16));
}

// one (sub-)image in place: `base` points at its first filter byte
uint32_t unfilter_image(uint8_t* base, uint32_t w, uint32_t h, uint32_t ct, uint32_t depth) {
    const uint32_t bpp = png_filter_bpp(ct, depth), rb = static_cast<uint32_t>(png_row_bytes(w, ct, depth)), pitch = rb + 1u, units = rb / bpp;
    uint32_t status = kPngDecOk;
    for (uint32_t y0 = 0; y0 < h; y0 += kInfLanes) {
        uint64_t a[kInfLanes] = {}, c[kInfLanes] = {}, prod[kInfLanes] = {}, up[kInfLanes];
        uint32_t f[kInfLanes];
        for (uint32_t r = 0; r < kInfLanes; ++r) {
            f[r] = y0 + r < h ? base[static_cast<size_t>(y0 + r) * pitch] : 0u;
            if (f[r] > 4u) { status = kPngDecFilter; f[r] = 0; }
        }
        for (uint32_t t = 0; t < units + kInfLanes - 1u; ++t) {
            for (uint32_t r = 0; r < kInfLanes; ++r) up[r] = r ? prod[r - 1u] : 0u;          // the lane shift, before anybody's step
            for (uint32_t r = 0; r < kInfLanes; ++r) {
                const uint32_t x = t - r, y = y0 + r;
                if (t < r || x >= units || y >= h) continue;
                uint8_t* p = base + static_cast<size_t>(y) * pitch + 1u + static_cast<size_t>(x) * bpp;
                const uint64_t b = r ? up[r] : y ? png_load_pixel(p - pitch, bpp) : 0u;
                const uint64_t v = png_unfilter_pixel(f[r], png_load_pixel(p, bpp), a[r], b, c[r], bpp);
                png_store_pixel(p, v, bpp);
                a[r] = v; c[r] = b; prod[r] = v;
            }
        }
    }
    return status;
}
}  // namespace

extern "C" {

// the stream in a buffer of exactly len rounded up to 16 bytes, the output in one of exactly cap rounded up to 16
uint32_t png_dec_emu_inflate(const uint8_t* src, uint32_t len, uint8_t* dst, uint32_t cap, uint32_t* produced) {
    const size_t in_bytes = (static_cast<size_t>(len) + 15u) & ~static_cast<size_t>(15), out_bytes = (static_cast<size_t>(cap) + 15u) & ~static_cast<size_t>(15);
    uint8_t* in = aligned_bytes(in_bytes);
    uint8_t* out = aligned_bytes(out_bytes);
    std::memset(in, 0, in_bytes ? in_bytes : 16);
    if (len) std::memcpy(in, src, len);
    PngInflateLds* S = new PngInflateLds;
    std::memset(S, 0xA5, sizeof *S);
    HostExec x;
    const PngInflateResult r = png_inflate(x, *S, in, len, out, cap);
    if (r.produced) std::memcpy(dst, out, r.produced);
    if (produced) *produced = r.produced;
    delete S;
    std::free(in); std::free(out);
    return r.status;
}

uint64_t png_dec_emu_inflated_size(uint32_t w, uint32_t h, uint32_t ct, uint32_t depth, uint32_t interlace) { return png_inflated_size(w, h, ct, depth, interlace); }
uint32_t png_dec_emu_filter_bpp(uint32_t ct, uint32_t depth) { return png_filter_bpp(ct, depth); }

// the inflated bytes of a whole file, in place
uint32_t png_dec_emu_unfilter(uint8_t* data, uint32_t w, uint32_t h, uint32_t ct, uint32_t depth, uint32_t interlace) {
    if (!interlace) return unfilter_image(data, w, h, ct, depth);
    uint32_t status = kPngDecOk;
    size_t off = 0;
    for (uint32_t p = 0; p < 7u; ++p) {
        const uint32_t pw = png_pass_width(w, p), ph = png_pass_height(h, p);
        if (!pw || !ph) continue;
        const uint32_t s = unfilter_image(data + off, pw, ph, ct, depth);
        if (s) status = s;
        off += png_image_bytes(pw, ph, ct, depth);
    }
    return status;
}

// un-filtered bytes -> BGRA rows of `stride`; palette: 256 BGRA dwords
void png_dec_emu_expand(const uint8_t* data, uint32_t w, uint32_t h, uint32_t ct, uint32_t depth, uint32_t interlace, const uint32_t* palette,
                        uint32_t has_trns, const uint32_t* key, uint8_t* out, uint32_t stride) {
    PngExpand e = {ct, depth, has_trns, {key[0], key[1], key[2]}};
    size_t pass_off[7];
    size_t off = 0;
    for (uint32_t p = 0; p < 7u; ++p) { pass_off[p] = off; off += png_image_bytes(png_pass_width(w, p), png_pass_height(h, p), ct, depth); }
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const uint8_t* row;
            uint32_t px = x;
            if (interlace) {
                const uint32_t p = png_pass_of(x, y), pw = png_pass_width(w, p);
                px = (x - png_pass_x0(p)) / png_pass_dx(p);
                row = data + pass_off[p] + static_cast<size_t>((y - png_pass_y0(p)) / png_pass_dy(p)) * (1u + png_row_bytes(pw, ct, depth)) + 1u;
            } else {
                row = data + static_cast<size_t>(y) * (1u + png_row_bytes(w, ct, depth)) + 1u;
            }
            const uint32_t v = png_expand_pixel(e, palette, row, px);
            std::memcpy(out + static_cast<size_t>(y) * stride + 4u * x, &v, 4);
        }
}

}  // extern "C"

#ifdef PNG_DEC_EMU_MAIN
// The sanitizer build: cases from a file (u32 kind; 0: len, cap, bytes -- 1: w, h, colour type, depth, interlace, n, bytes),
// a line "status produced crc32" per case.
#include <cstdio>
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t kind;
    while (std::fread(&kind, 4, 1, f) == 1) {
        if (kind == 0u) {
            uint32_t hdr[2];
            if (std::fread(hdr, 4, 2, f) != 2) return 3;
            std::vector<uint8_t> src(hdr[0] ? hdr[0] : 1), dst(hdr[1] ? hdr[1] : 1);
            if (hdr[0] && std::fread(src.data(), 1, hdr[0], f) != hdr[0]) return 3;
            uint32_t produced = 0;
            const uint32_t st = png_dec_emu_inflate(src.data(), hdr[0], dst.data(), hdr[1], &produced);
            std::printf("%u %u %u\n", st, produced, png_crc32(dst.data(), produced));
        } else {
            uint32_t hdr[6];
            if (std::fread(hdr, 4, 6, f) != 6) return 3;
            std::vector<uint8_t> data(hdr[5] ? hdr[5] : 1);
            if (hdr[5] && std::fread(data.data(), 1, hdr[5], f) != hdr[5]) return 3;
            const uint32_t st = png_dec_emu_unfilter(data.data(), hdr[0], hdr[1], hdr[2], hdr[3], hdr[4]);
            std::printf("%u %u %u\n", st, hdr[5], png_crc32(data.data(), hdr[5]));
        }
    }
    std::fclose(f);
    return 0;
}
#endif
