// webp_read.cpp -- the host side of the WebP decoder: the RIFF walk, the VP8L header facts, the colour policy, and the
// prepare of a lossless stream for the device (csrc/webp_decode.hip) with the token loop of csrc/webp_decode_core.hpp.
// What WebPGetFeatures and the demuxer do for the reference (imageflow_core/src/codecs/webp.rs:20-248, sniffed at
// codecs/mod.rs:130-131).  The container rules are pinned to libwebp 1.6.0 through Pillow (tests/test_webp_decode_entry_points.py):
//   * the RIFF size counts: a size that reaches beyond the buffer is refused, bytes behind a smaller size are ignored,
//     and every chunk with its padding byte lies inside the size;
//   * a file without VP8X starts with its image chunk; with VP8X, unknown chunks may stand anywhere, the canvas equals
//     the image's size, and one image chunk is allowed;
//   * has_alpha is the VP8L header's bit, whatever the VP8X ALPHA flag says;
//   * an ICCP chunk counts where the VP8X ICC flag is set (the demuxer shows no profile otherwise).
#include "webp_read.hpp"

#include <hip/hip_runtime.h>

#include <cstring>

#include "common.hpp"
#include "webp_decode_core.hpp"

namespace ifhip {
namespace {

uint32_t le32(const uint8_t* p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24; }
uint32_t le24(const uint8_t* p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16; }
bool tag_is(const uint8_t* p, const char* t) { return std::memcmp(p, t, 4) == 0; }
int malformed(const char* what) { return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: libwebp decoding error BITSTREAM_ERROR (%s)", what); }

}  // namespace

int parse_webp(const uint8_t* d, size_t len, WebpParsed* out) {
    WebpParsed& P = *out;
    P = WebpParsed();
    if (!d || len < 12u || !tag_is(d, "RIFF") || !tag_is(d + 8, "WEBP")) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: not a WebP (no RIFF / WEBP signature)");
    const uint64_t riff = le32(d + 4);
    if (riff < 12u) return malformed("the RIFF size holds no chunk");
    if (riff + 8u > len) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: libwebp decoding error NOT_ENOUGH_DATA (the RIFF size reaches beyond the file)");
    const size_t end = static_cast<size_t>(riff + 8u);
    size_t pos = 12;
    bool vp8x = false, have_image = false, lossy = false;
    uint32_t flags = 0, canvas_w = 0, canvas_h = 0;
    const uint8_t* iccp = nullptr;
    size_t iccp_len = 0;
    while (pos + 8u <= end) {
        const uint8_t* tag = d + pos;
        const uint64_t n = le32(d + pos + 4), padded = n + (n & 1u);
        if (pos + 8u + padded > end) return malformed("a chunk reaches beyond the RIFF size");
        const uint8_t* q = d + pos + 8;
        const bool first = pos == 12u;
        if (tag_is(tag, "VP8X")) {
            if (!first || n < 10u) return malformed("VP8X out of place");
            vp8x = true; flags = q[0]; canvas_w = le24(q + 4) + 1u; canvas_h = le24(q + 7) + 1u;
        } else if (tag_is(tag, "VP8L") || tag_is(tag, "VP8 ")) {
            if (have_image) return malformed("a second image chunk");
            have_image = true;
            if (tag[3] == 'L') {
                if (n < 5u || q[0] != 0x2Fu || (q[4] >> 5) != 0u) return malformed("the VP8L header");
                const uint32_t bits = le32(q + 1);
                P.lossless = true; P.payload = q; P.payload_len = static_cast<size_t>(n);
                P.w = (bits & 0x3FFFu) + 1u; P.h = ((bits >> 14) & 0x3FFFu) + 1u; P.has_alpha = ((bits >> 28) & 1u) != 0u;
            } else {
                lossy = true; P.vp8 = q; P.vp8_len = static_cast<size_t>(n);
                if (n < 10u || q[3] != 0x9D || q[4] != 0x01 || q[5] != 0x2A) return malformed("the VP8 frame header");
                P.w = (q[6] | static_cast<uint32_t>(q[7]) << 8) & 0x3FFFu; P.h = (q[8] | static_cast<uint32_t>(q[9]) << 8) & 0x3FFFu;
                if (!P.w || !P.h) return malformed("the VP8 frame header");
            }
            if (!vp8x) break;                                               // a simple file is its image chunk
        } else if (!vp8x) {
            return malformed("no image chunk at the start of a file without VP8X");
        } else if (tag_is(tag, "ALPH")) {
            P.has_alpha = true;
            if (!P.alph && !have_image) { P.alph = q; P.alph_len = static_cast<size_t>(n); }
        } else if (tag_is(tag, "ANIM") || tag_is(tag, "ANMF")) {
            P.animated = true;
        } else if (tag_is(tag, "ICCP")) {
            if (!iccp) { iccp = q; iccp_len = static_cast<size_t>(n); }
        }
        pos += 8u + static_cast<size_t>(padded);
    }
    if (vp8x && (flags & 0x02u)) P.animated = true;
    if (P.animated || !lossy) { P.vp8 = P.alph = nullptr; P.vp8_len = P.alph_len = 0; }
    if (P.animated) { P.w = canvas_w; P.h = canvas_h; P.lossless = false; P.payload = nullptr; P.payload_len = 0; P.has_alpha = (flags & 0x10u) != 0u; }
    else if (!have_image) return malformed("no image chunk");
    else if (vp8x && (canvas_w != P.w || canvas_h != P.h)) return malformed("the VP8X canvas is not the image's size");
    if (lossy && !P.animated && vp8x && (flags & 0x10u)) P.has_alpha = true;
    if (vp8x && (flags & 0x20u) && iccp) { P.color_kind = icc_describes_srgb(iccp, iccp_len) ? 1 : 2; P.icc = iccp; P.icc_len = iccp_len; }
    return IFHIP_OK;
}

int parse_webp_for_decode(const uint8_t* d, size_t len, WebpParsed* out) {
    if (int rc = parse_webp(d, len, out)) return rc;
    if (out->animated) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: libwebp decoding error UNSUPPORTED_FEATURE (an animated WebP: WebPDecode answers the same)");
    if (!out->lossless) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "ImageTypeNotSupported: a lossy WebP (VP8%s): the lossy VP8 decoder is not built, only lossless VP8L files are read",
                                    out->has_alpha ? " + ALPH" : "");
    if (out->payload_len > 0x7FFF0000u) return malformed("a VP8L chunk above 2^31 bytes");
    return IFHIP_OK;
}

int parse_webp_lossy_for_decode(const uint8_t* d, size_t len, WebpParsed* out) {
    if (int rc = parse_webp(d, len, out)) return rc;
    if (out->animated) return fail(IFHIP_INVALID_ARGUMENT, "ImageMalformed: libwebp decoding error UNSUPPORTED_FEATURE (an animated WebP: WebPDecode answers the same)");
    if (out->lossless) return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "ImageTypeNotSupported: not a lossy WebP (VP8L): lossless files are read by the lossless decoder");
    if (out->vp8_len > 0x7FFF0000u || out->alph_len > 0x7FFF0000u) return malformed("a chunk above 2^31 bytes");
    return IFHIP_OK;
}

void webp_prepare_job(const WebpParsed& parsed, WebpJob* job) {
    job->parsed = parsed;
    job->prepared = std::make_shared<WebpPrepared>();
    const uint32_t len = static_cast<uint32_t>(parsed.payload_len);
    WebpPrepared& P = *job->prepared;
    P.payload.assign((static_cast<size_t>(len) + 15u) / 16u + 1u, WebpQuad{0u, 0u, 0u, 0u});   // 16-byte aligned, zero-padded
    std::memcpy(P.payload.data(), parsed.payload, len);
    WebpHeadReader reader(reinterpret_cast<const uint8_t*>(P.payload.data()), len);
    job->status = reader.prepare(&P);
}

const char* webp_status_text(uint32_t s) {
    switch (s) {
    case kWebpDecTruncated: return "NOT_ENOUGH_DATA (the VP8L stream ends early)";
    case kWebpDecCodeLengths: return "BITSTREAM_ERROR (a set of code lengths that is no prefix code)";
    case kWebpDecBadCode: return "BITSTREAM_ERROR (bits that are no code)";
    case kWebpDecDistance: return "BITSTREAM_ERROR (a backward reference before the image's start)";
    case kWebpDecCopyEnd: return "BITSTREAM_ERROR (a backward reference past the image's end)";
    case kWebpDecCacheSymbol: return "BITSTREAM_ERROR (a colour cache symbol beyond the cache)";
    case kWebpDecTransform: return "BITSTREAM_ERROR (a transform twice, or colour cache bits outside 1..11)";
    case kWebpDecTooLittle: return "NOT_ENOUGH_DATA (the VP8L header is incomplete)";
    default: return "BITSTREAM_ERROR (the container did not parse)";
    }
}

}  // namespace ifhip

using namespace ifhip;

extern "C" int ifhip_webp_info(const uint8_t* webp, size_t len, ifhip_webp_file_info* info) {
    if (!info) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null out-pointer");
    std::memset(info, 0, sizeof *info);
    if (!webp) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null file pointer");
    WebpParsed P;
    if (int rc = parse_webp(webp, len, &P)) return rc;
    info->width = P.w; info->height = P.h; info->has_alpha = P.has_alpha ? 1u : 0u; info->lossless = P.lossless ? 1u : 0u;
    info->animated = P.animated ? 1u : 0u; info->color_kind = P.color_kind;
    return IFHIP_OK;
}
