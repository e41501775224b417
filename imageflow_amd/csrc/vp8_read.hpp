// vp8_read.hpp -- the host stage of the lossy WebP decoder (csrc/vp8_read.cpp): what is serial in a VP8 key frame -- the
// frame tag and header, the bool-decoding of the first partition (segment, skip flag and modes of every macroblock) and of
// the token partitions (the coefficient levels) -- and the ALPH chunk's header byte with, for a VP8L-coded plane, the prepare
// of its header-less stream.  Plain C++: the CPU emulation of the tests includes it without a device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "vp8_decode_core.hpp"
#include "webp_read.hpp"

namespace ifhip {

struct Vp8Frame {
    uint32_t w = 0, h = 0, mbw = 0, mbh = 0;
    uint32_t filter = kVp8FilterNone;    // kVp8FilterNone where the level is 0
    Vp8Quant quant[4];                   // per segment
    std::vector<Vp8Mb> mbs;              // mbw * mbh, raster order
    std::vector<int16_t> levels;         // kVp8MbLevels per macroblock, un-dequantised, each block in raster order
    uint32_t alpha_kind = kVp8AlphaNone, alpha_filter = 0;
    const uint8_t* alpha_data = nullptr; // behind the ALPH header byte, inside the caller's file
    size_t alpha_len = 0;
    std::shared_ptr<WebpPrepared> alpha_prepared;   // kVp8AlphaVp8l: the stream as the device VP8L reader takes it
    uint32_t alpha_vp8l_status = 0;      // the IFHIP_WEBP_DEC_* word of that prepare
    uint32_t status = kVp8DecOk;         // non-zero: nothing runs for the file
};

// The `VP8 ` chunk's bytes -> the frame's records; the status word (also left in out->status).
uint32_t vp8_read_frame(const uint8_t* payload, size_t len, Vp8Frame* out);
// The `ALPH` chunk's bytes for a frame whose size is known; the status word (kVp8DecAlphaHeader / kVp8DecAlphaStream), kept in
// out->status where the frame was fine so far.
uint32_t vp8_read_alpha(const uint8_t* alph, size_t len, Vp8Frame* out);
const char* vp8_status_text(uint32_t status);

// A file walked (parse_webp_lossy_for_decode) and read on the host, and the device part of a decode (csrc/vp8_decode.hip).
// jobs[i] == nullptr: the file's container did not parse; frame.status == kVp8DecNotLossy: a lossless file, which gets no frame.
struct Vp8Job {
    WebpParsed parsed;
    Vp8Frame frame;
};
void vp8_prepare_job(const WebpParsed& parsed, Vp8Job* job);
int vp8_decode_prepared_device(const Vp8Job* const* jobs, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                               const uint32_t* strides, uint32_t* d_status, void* hip_stream);

}  // namespace ifhip
