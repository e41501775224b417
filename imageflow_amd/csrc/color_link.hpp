// color_link.hpp -- a GRAY or LUT-based ICC profile turned into what the link kernel needs (csrc/color_link.cpp): a table of
// 256 bytes, or 33^3 nodes sampled through the profile's A2B0 and lcms2's built-in sRGB.  Host only, and free of the rest of
// the library: tests link color_link.cpp alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "color_profile.hpp"

namespace ifhip {

constexpr int kColorLinkGray = 1, kColorLinkRgb = 2;       // IFHIP_COLOR_LINK_GRAY / _RGB

struct ColorLink {
    int kind = 0;
    uint8_t gray[256] = {};
    std::vector<uint64_t> nodes;     // kColorLinkRgb: kLinkNodes of R | G << 16 | B << 32, the R index slowest
};
// status and reason as color_plan_from_icc's; `out` is filled only when PLANNED
ColorPlanResult color_link_from_icc(const uint8_t* icc, size_t len, bool frame_is_gray, ColorLink* out);

}  // namespace ifhip
