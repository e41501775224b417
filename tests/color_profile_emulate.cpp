// color_profile_emulate.cpp -- the CPU emulation of the colour conversion kernel (csrc/color_profile.hip): the same per-pixel
// arithmetic (csrc/color_profile_core.hpp), the same plans (csrc/color_profile.cpp) and the same linear->sRGB table
// (csrc/color.cpp), built with g++ by tests/color_profile_emulation.py.  No HIP, no device.
#include <cstring>

#include "../imageflow_amd/csrc/color.cpp"
#include "../imageflow_amd/csrc/color_profile.cpp"
#include "../imageflow_amd/csrc/color_profile_core.hpp"

namespace {
void copy_reason(const char* why, char* reason, size_t cap) {
    if (!reason || !cap) return;
    std::strncpy(reason, why ? why : "", cap - 1);
    reason[cap - 1] = 0;
}
}  // namespace

extern "C" {

int cp_emu_plan_from_icc(const uint8_t* icc, size_t len, ifhip_color_plan* out, char* reason, size_t cap) {
    const ifhip::ColorPlanResult r = ifhip::color_plan_from_icc(icc, len, out);
    copy_reason(r.reason, reason, cap);
    return r.status;
}

int cp_emu_plan_from_gamma_primaries(double gamma, const double* xy, ifhip_color_plan* out, char* reason, size_t cap) {
    const ifhip::ColorPlanResult r = ifhip::color_plan_from_gamma_primaries(gamma, xy, out);
    copy_reason(r.reason, reason, cap);
    return r.status;
}

const char* cp_emu_status_text(int status) { return ifhip::color_plan_status_text(status); }

void cp_emu_l2s(uint8_t* out16384) { std::memcpy(out16384, ifhip::color_tables().l2s, 16384); }

// in place over h rows of w BGRA pixels, `stride` bytes apart; bytes between the rows are not touched
void cp_emu_transform(uint8_t* bgra, uint32_t w, uint32_t h, size_t stride, const ifhip_color_plan* plan) {
    const uint8_t* l2s = ifhip::color_tables().l2s;
    for (uint32_t y = 0; y < h; ++y) {
        uint8_t* row = bgra + static_cast<size_t>(y) * stride;
        for (uint32_t x = 0; x < w; ++x) {
            uint32_t px;
            std::memcpy(&px, row + 4u * x, 4);
            px = ifhip::color_pixel(px, plan->linear[0][(px >> 16) & 255u], plan->linear[1][(px >> 8) & 255u], plan->linear[2][px & 255u], plan->matrix, l2s);
            std::memcpy(row + 4u * x, &px, 4);
        }
    }
}

}  // extern "C"
