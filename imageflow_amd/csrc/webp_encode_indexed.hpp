// webp_encode_indexed.hpp -- what webp_encode.hip's batch call launches of webp_encode_indexed.hip when the stage carries
// IFHIP_WEBP_ENC_COLOR_INDEXING: the front (count, palette, bundle) ahead of the plain coder's own residual / parse / codes,
// the back (the packed image's parse and codes, the layout that sizes both files and picks one, the emit of that one) behind
// them; webp_finish_kernel closes either file.
#pragma once
#include <hip/hip_runtime.h>

#include "webp_encode_device.hpp"

namespace ifhip {

constexpr uint32_t kWebpSetSlots = 1024;                // the hash set of an image's colours: at most 257 of them are ever needed
constexpr uint32_t kWebpSetWords = kWebpSetSlots + 4u;  // ... and behind them: the colours inserted, overflow, opaque white seen, unused
// What the palette kernel leaves of an image: n_colours 0 where the frame has more than 256 (it is written plain).
struct WebpIndexRecord {
    uint32_t n_colours, width_bits, packed_w, unused;
    uint32_t palette[kWebpMaxPalette];
};
struct WebpIndexArgs {
    uint32_t* sets;                     // [n_images][kWebpSetWords], zeroed per batch
    WebpIndexRecord* rec;               // [n_images]
};

// Both return IFHIP_OK or a failed call's status.  `packed` is `plain` with the packed image's own scratch (resid holds the bundled pixels; modes is unused); both share
// `image`, the files and the outputs, and both carry the stage's full geometry, from which the grids are sized.
int webp_indexed_front(const WebpArgs& packed, const WebpIndexArgs& ix, hipStream_t st);
int webp_indexed_back(const WebpArgs& plain, const WebpArgs& packed, const WebpIndexArgs& ix, hipStream_t st);

}  // namespace ifhip
