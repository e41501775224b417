// png_read.cpp -- the host side of the PNG decoder: signature, chunk walk with CRCs, IHDR / PLTE / tRNS rules, the colour
// policy, and the gathering of the IDAT payloads into the one zlib stream that goes to the device (csrc/png_decode.hip).
// What png_read_info does for the reference (c_components/lib/codec_png_wrapper.c:131-212; libpng_decoder.rs:36-104,
// 297-299,340-383).  Pixel data is never inflated here; a compressed iCCP profile is, with the same core as the kernels.
#include "png_read.hpp"

#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "common.hpp"
#include "png_decode_core.hpp"

namespace ifhip {
namespace {

struct HostExec {
    template <typename F> void lanes(F f) { for (uint32_t lane = 0; lane < kInfLanes; ++lane) f(lane); }
    template <typename F> void one(F f) { f(); }
    void sync() {}
};

uint32_t be32(const uint8_t* p) { return static_cast<uint32_t>(p[0]) << 24 | static_cast<uint32_t>(p[1]) << 16 | static_cast<uint32_t>(p[2]) << 8 | p[3]; }
uint32_t be16(const uint8_t* p) { return static_cast<uint32_t>(p[0]) << 8 | p[1]; }
constexpr uint32_t fourcc(char a, char b, char c, char d) {
    return static_cast<uint32_t>(static_cast<uint8_t>(a)) << 24 | static_cast<uint32_t>(static_cast<uint8_t>(b)) << 16 | static_cast<uint32_t>(static_cast<uint8_t>(c)) << 8 | static_cast<uint8_t>(d);
}
uint32_t crc_of(const uint8_t* p, size_t n) {
    static uint32_t table[256];
    static const bool ready = [] { for (uint32_t i = 0; i < 256u; ++i) table[i] = png_crc_step(0u, i); return true; }();
    (void)ready;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}
int malformed(const char* what) { return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: LibPNG error: %s", what); }

// iCCP: name (1..79 bytes), 0, compression method 0, a zlib stream.  The profile's size is in its own first four bytes.
// -> 1: the profile describes sRGB, 2: any other (also one that does not inflate)
int classify_iccp(const uint8_t* q, size_t n, std::vector<uint8_t>* profile) {
    size_t k = 0;
    while (k < n && k < 80u && q[k]) ++k;
    if (k == 0u || k >= n || q[k] != 0 || k + 2u > n || q[k + 1u] != 0) return 2;
    const uint8_t* z = q + k + 2u;
    const size_t zn = n - k - 2u;
    const size_t padded = (zn + 15u) & ~static_cast<size_t>(15);
    std::vector<PngQuad> in(padded / 16u + 1u, PngQuad{0u, 0u, 0u, 0u});
    std::memcpy(in.data(), z, zn);
    std::unique_ptr<PngInflateLds> S(new PngInflateLds);
    HostExec x;
    // the first 128 bytes (they hold the profile's size: the stream is cut there), then the whole profile; capped at 16 MiB
    std::vector<PngQuad> head(8);
    PngInflateResult r = png_inflate(x, *S, reinterpret_cast<const uint8_t*>(in.data()), static_cast<uint32_t>(zn), reinterpret_cast<uint8_t*>(head.data()), 128u);
    if (r.status != kPngDecOk) return 2;
    const uint32_t size = be32(reinterpret_cast<const uint8_t*>(head.data()));
    if (size < 132u || size > (16u << 20)) return 2;
    std::vector<PngQuad> out((size + 15u) / 16u);
    r = png_inflate(x, *S, reinterpret_cast<const uint8_t*>(in.data()), static_cast<uint32_t>(zn), reinterpret_cast<uint8_t*>(out.data()), size);
    if (r.status != kPngDecOk) return 2;
    profile->assign(reinterpret_cast<const uint8_t*>(out.data()), reinterpret_cast<const uint8_t*>(out.data()) + size);
    return icc_describes_srgb(profile->data(), size) ? 1 : 2;
}

}  // namespace

int parse_png(const uint8_t* d, size_t len, PngParsed* out, bool gather) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
    if (!d || len < 8u || std::memcmp(d, sig, 8) != 0) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: not a PNG (no signature)");
    PngParsed& P = *out;
    P.idat.clear();
    P.icc.clear();
    for (uint32_t i = 0; i < 256u; ++i) P.palette[i] = 0xFF000000u;
    size_t pos = 8, idat_total = 0;
    bool have_ihdr = false, have_plte = false, have_idat = false, have_iend = false, have_srgb = false, have_gama = false, have_chrm = false, have_iccp = false;
    uint32_t n_palette = 0, gama = 0, chrm[8] = {0};
    int iccp_kind = 0;
    const uint8_t* trns = nullptr;
    size_t trns_len = 0;
    while (!have_iend) {
        if (pos + 12u > len) return malformed(have_idat ? "Read Error (no IEND)" : "Read Error (the file ends inside a chunk)");
        const uint32_t n = be32(d + pos), type = be32(d + pos + 4);
        if (n > 0x7FFFFFFFu || static_cast<uint64_t>(pos) + 12u + n > len) return malformed("Read Error (a chunk is longer than the file)");
        const uint8_t* q = d + pos + 8;
        const bool checked = type == fourcc('I', 'H', 'D', 'R') || type == fourcc('P', 'L', 'T', 'E') || type == fourcc('t', 'R', 'N', 'S') || type == fourcc('I', 'D', 'A', 'T') ||
                             type == fourcc('I', 'E', 'N', 'D') || type == fourcc('s', 'R', 'G', 'B') || type == fourcc('g', 'A', 'M', 'A') || type == fourcc('c', 'H', 'R', 'M') ||
                             type == fourcc('i', 'C', 'C', 'P');
        if (checked && crc_of(d + pos + 4, 4u + n) != be32(q + n)) return malformed("CRC error");
        if (!have_ihdr && type != fourcc('I', 'H', 'D', 'R')) return malformed("Missing IHDR before the first chunk");
        if (type == fourcc('I', 'H', 'D', 'R')) {
            if (have_ihdr || n != 13u) return malformed("Invalid IHDR chunk");
            have_ihdr = true;
            P.w = be32(q); P.h = be32(q + 4); P.depth = q[8]; P.color_type = q[9]; P.interlace = q[12];
            if (P.w == 0u || P.h == 0u || P.w > 0x7FFFFFFFu || P.h > 0x7FFFFFFFu) return malformed("Invalid IHDR data (image size)");
            if (!png_legal_type(P.color_type, P.depth)) return malformed("Invalid IHDR data (colour type and bit depth)");
            if (q[10] != 0 || q[11] != 0 || P.interlace > 1u) return malformed("Invalid IHDR data (compression, filter or interlace method)");
            P.alpha_used = (P.color_type & 4u) != 0u || P.color_type == 3u;      // codec_png_wrapper.c:176-186
            P.uses_palette = (P.color_type & 1u) != 0u;                         // :270
        } else if (type == fourcc('P', 'L', 'T', 'E')) {
            if (have_plte || have_idat) return malformed("PLTE out of place");
            if (n % 3u != 0u || n > 768u) return malformed("Invalid palette chunk");
            if (P.color_type == 3u && n / 3u > (1u << P.depth)) return malformed("Invalid palette chunk (more entries than the bit depth can index)");
            have_plte = true;
            n_palette = n / 3u;
            if (P.color_type == 3u)
                for (uint32_t i = 0; i < n_palette; ++i) P.palette[i] = 0xFF000000u | static_cast<uint32_t>(q[3u * i]) << 16 | static_cast<uint32_t>(q[3u * i + 1u]) << 8 | q[3u * i + 2u];
        } else if (type == fourcc('t', 'R', 'N', 'S')) {
            if (have_idat) return malformed("tRNS after IDAT");
            if (P.color_type == 3u ? have_plte : true) { trns = q; trns_len = n; }           // (before PLTE: libpng ignores it)
        } else if (type == fourcc('I', 'D', 'A', 'T')) {
            if (P.color_type == 3u && !have_plte) return malformed("Missing PLTE before IDAT");
            have_idat = true;
            idat_total += n;
            if (idat_total > 0x7FFF0000u) return malformed("IDAT data above 2^31 bytes");
            if (gather && n) P.idat.push_back({q, n});
        } else if (type == fourcc('I', 'E', 'N', 'D')) {
            have_iend = true;
        } else if (type == fourcc('s', 'R', 'G', 'B')) {
            have_srgb = true;
        } else if (type == fourcc('g', 'A', 'M', 'A')) {
            if (n == 4u) { have_gama = true; gama = be32(q); }
        } else if (type == fourcc('c', 'H', 'R', 'M')) {
            if (n == 32u) { have_chrm = true; for (int k = 0; k < 8; ++k) chrm[k] = be32(q + 4 * k); }
        } else if (type == fourcc('i', 'C', 'C', 'P')) {
            if (!have_iccp) { have_iccp = true; iccp_kind = classify_iccp(q, n, &P.icc); }
        } else if (!(type & 0x20000000u)) {                                          // bit 5 of the first letter clear: critical
            return malformed("unhandled critical chunk");
        }
        pos += 12u + static_cast<size_t>(n);
    }
    if (!have_idat) return malformed("Missing IDAT");
    if (trns) {
        if (P.color_type == 3u) {
            if (trns_len <= n_palette && trns_len <= 256u)
                for (size_t i = 0; i < trns_len; ++i) P.palette[i] = (P.palette[i] & 0x00FFFFFFu) | static_cast<uint32_t>(trns[i]) << 24;
        } else if ((P.color_type == 0u && trns_len == 2u) || (P.color_type == 2u && trns_len == 6u)) {
            const uint32_t mask = P.depth == 16u ? 0xFFFFu : (1u << P.depth) - 1u;   // png_do_expand compares the key's low bits
            P.has_trns = 1u;
            for (size_t k = 0; k < trns_len / 2u; ++k) P.key[k] = be16(trns + 2u * k) & mask;
        }
    }
    // colour: an iCCP decides; else an sRGB chunk; else gAMA + cHRM together (honor_gama_chrm = true, libpng_decoder.rs:233),
    // which are sRGB when they carry the values the specification gives for it; gAMA alone is ignored (honor_gama_only = false)
    static const uint32_t srgb_chrm[8] = {31270u, 32900u, 64000u, 33000u, 30000u, 60000u, 15000u, 6000u};
    P.has_iccp = have_iccp;
    P.gama = gama; std::memcpy(P.chrm, chrm, sizeof chrm);
    if (have_iccp) P.color_kind = iccp_kind;
    else if (have_srgb) P.color_kind = 1;
    else if (have_gama && have_chrm) P.color_kind = gama == 45455u && std::memcmp(chrm, srgb_chrm, sizeof chrm) == 0 ? 1 : 2;
    else P.color_kind = 0;
    P.inflated = png_inflated_size(P.w, P.h, P.color_type, P.depth, P.interlace);
    P.idat_len = idat_total;
    return IFHIP_OK;
}

}  // namespace ifhip

using namespace ifhip;

extern "C" int ifhip_png_info(const uint8_t* png, size_t len, ifhip_png_file_info* info) {
    if (!info) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    std::memset(info, 0, sizeof *info);
    if (!png) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    PngParsed P;
    if (int rc = parse_png(png, len, &P, false)) return rc;
    info->width = P.w; info->height = P.h; info->bit_depth = P.depth; info->color_type = P.color_type; info->interlace = P.interlace;
    info->alpha_used = P.alpha_used ? 1u : 0u; info->uses_palette = P.uses_palette ? 1u : 0u;
    info->color_kind = P.color_kind;
    return IFHIP_OK;
}
