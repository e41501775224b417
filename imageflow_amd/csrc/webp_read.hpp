// webp_read.hpp -- what the host learns from a WebP file before the device sees it (csrc/webp_read.cpp): the RIFF walk's
// facts (size, has_alpha, lossless / animated, the colour verdict, where the VP8L payload lies) and, for a decode, the
// prepared stream: the transforms with their sub-images, the entropy image and every group's decode records.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>

namespace ifhip {

struct WebpPrepared;                     // csrc/webp_decode_core.hpp

struct WebpParsed {
    uint32_t w = 0, h = 0;
    bool has_alpha = false;              // what WebPGetFeatures reports: the VP8L header's bit, whatever a VP8X chunk's ALPHA flag says
    bool lossless = false, animated = false;
    int color_kind = 0;                  // 0: no ICCP; 1: an ICCP profile that describes sRGB; 2: any other profile
    const uint8_t* payload = nullptr;    // the VP8L chunk's bytes, inside the caller's file
    size_t payload_len = 0;
    const uint8_t* icc = nullptr;        // the ICCP chunk's bytes behind color_kind 1 or 2, inside the caller's file
    size_t icc_len = 0;
    const uint8_t* vp8 = nullptr;        // a still lossy file: the `VP8 ` chunk's bytes and, where there is one, the `ALPH` chunk's
    size_t vp8_len = 0;
    const uint8_t* alph = nullptr;
    size_t alph_len = 0;
};
// IFHIP_OK, or IFHIP_INVALID_ARGUMENT with an "ImageMalformed: libwebp decoding error ..." message.  A lossy or an animated
// file parses (lossless = false / animated = true): what to answer is the caller's.
int parse_webp(const uint8_t* d, size_t len, WebpParsed* out);
// parse_webp for a decode: IFHIP_METHOD_NOT_IMPLEMENTED "ImageTypeNotSupported: ..." for lossy VP8, ImageMalformed
// naming UNSUPPORTED_FEATURE for an animation
int parse_webp_for_decode(const uint8_t* d, size_t len, WebpParsed* out);
// parse_webp for the lossy decoder (csrc/vp8_read.cpp, csrc/vp8_decode.hip): a still `VP8 ` (+ `ALPH`) file.  A lossless file is
// IFHIP_METHOD_NOT_IMPLEMENTED "ImageTypeNotSupported: not a lossy WebP ...", an animation ImageMalformed naming UNSUPPORTED_FEATURE.
int parse_webp_lossy_for_decode(const uint8_t* d, size_t len, WebpParsed* out);

// A file's stream prepared on the host (header, transforms, entropy image, codes) and its padded payload.
struct WebpJob {
    WebpParsed parsed;
    std::shared_ptr<WebpPrepared> prepared;
    uint32_t status = 0;                 // the IFHIP_WEBP_DEC_* word of the prepare; non-zero: nothing runs for the file
};
void webp_prepare_job(const WebpParsed& parsed, WebpJob* job);
// The device part of a decode (csrc/webp_decode.hip).  jobs[i] == nullptr: the file's container did not parse.
int webp_decode_prepared_device(const WebpJob* const* jobs, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                                const uint32_t* strides, uint32_t* d_status, void* hip_stream);
const char* webp_status_text(uint32_t status);

}  // namespace ifhip
