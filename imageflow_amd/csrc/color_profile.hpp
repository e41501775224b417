// color_profile.hpp -- a colour profile turned into what the conversion kernel needs (csrc/color_profile.cpp): the plan of
// include/imageflow_hip.h, built on the host from ICC bytes or from a PNG's gAMA + cHRM.  Host only, and free of the rest of
// the library: tests link color_profile.cpp alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/imageflow_hip.h"

namespace ifhip {

struct ColorPlanResult {
    int status;              // ifhip_color_plan_status
    const char* reason;      // a literal that names the case ("" when planned)
};
ColorPlanResult color_plan_from_icc(const uint8_t* icc, size_t len, ifhip_color_plan* out);
ColorPlanResult color_plan_from_gamma_primaries(double gamma, const double xy[8], ifhip_color_plan* out);
const char* color_plan_status_text(int status);

}  // namespace ifhip
