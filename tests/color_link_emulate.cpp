// color_link_emulate.cpp -- the CPU emulation of the colour link kernel (csrc/color_link.hip): the same per-pixel arithmetic
// (csrc/color_link_core.hpp) on the same links (csrc/color_link.cpp), built with g++ by tests/color_link_emulation.py.  No HIP,
// no device.
#include <cstring>

#include "../imageflow_amd/csrc/color_link.cpp"

namespace {
void copy_reason(const char* why, char* reason, size_t cap) {
    if (!reason || !cap) return;
    std::strncpy(reason, why ? why : "", cap - 1);
    reason[cap - 1] = 0;
}
}  // namespace

extern "C" {

// kind 0 (no link), 1 (gray: 256 bytes written to `gray`) or 2 (rgb: 33^3 * 3 uint16 written to `nodes`)
int cl_emu_link_from_icc(const uint8_t* icc, size_t len, int frame_is_gray, int* kind, uint8_t* gray, uint16_t* nodes, char* reason, size_t cap) {
    ifhip::ColorLink link;
    const ifhip::ColorPlanResult r = ifhip::color_link_from_icc(icc, len, frame_is_gray != 0, &link);
    copy_reason(r.reason, reason, cap);
    *kind = r.status == IFHIP_COLOR_PLANNED ? link.kind : 0;
    if (*kind == ifhip::kColorLinkGray) std::memcpy(gray, link.gray, 256);
    if (*kind == ifhip::kColorLinkRgb)
        for (uint32_t i = 0; i < ifhip::kLinkNodes; ++i)
            for (uint32_t c = 0; c < 3u; ++c) nodes[3u * i + c] = static_cast<uint16_t>(link.nodes[i] >> (16u * c));
    return r.status;
}

// in place over h rows of w BGRA pixels, `stride` bytes apart; bytes between the rows are not touched
void cl_emu_transform(uint8_t* bgra, uint32_t w, uint32_t h, size_t stride, int kind, const uint8_t* gray, const uint16_t* nodes) {
    const auto node = [nodes](uint32_t i) { return nodes[3u * i] | static_cast<uint64_t>(nodes[3u * i + 1u]) << 16 | static_cast<uint64_t>(nodes[3u * i + 2u]) << 32; };
    for (uint32_t y = 0; y < h; ++y) {
        uint8_t* row = bgra + static_cast<size_t>(y) * stride;
        for (uint32_t x = 0; x < w; ++x) {
            uint32_t px;
            std::memcpy(&px, row + 4u * x, 4);
            px = kind == ifhip::kColorLinkGray ? ifhip::link_gray_pixel(px, gray) : ifhip::link_pixel(px, node);
            std::memcpy(row + 4u * x, &px, 4);
        }
    }
}

}  // extern "C"
