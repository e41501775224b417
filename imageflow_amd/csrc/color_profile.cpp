// color_profile.cpp -- profile -> plan on the host, for codecs/cms.rs::transform_to_srgb pinned to the reference's lcms2
// back end (codecs/lcms2_transform.rs):
//   ICC bytes        :219-242  Profile::new_icc + Transform::new(.., Intent::Perceptual): lcms2's matrix-shaper for an RGB
//                    profile with XYZ PCS and no A2B0 -- the colourants as stored (no chad, no wtpt), the TRCs per channel
//   gAMA + cHRM      :245-283  cmsCreateRGBProfile: the primaries' matrix scaled to the white, Bradford to D50, x^(1/gamma)
// The destination is lcms2's built-in sRGB profile: its colourants rounded to s15.16 as its tags hold them; its curve is
// the library's LINEAR_TO_SRGB table on the device.  f64 throughout, f32 at the very end.  No HIP, no other file of the
// library: a crafted profile is this file's business alone, and tests link it alone under sanitizers.
#include "color_profile.hpp"

#include <cmath>
#include <cstring>

#include "color_icc.hpp"

namespace ifhip {
namespace {

using namespace icc;

double srgb_to_linear(double s) { return s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4); }

// `xyz_from_rgb`: the source's colourants, columns R, G, B
bool finish_matrix(const Mat3& xyz_from_rgb, ifhip_color_plan* out) {
    Mat3 inv;
    if (!srgb_from_xyz(&inv)) return false;
    const Mat3 m = mul(inv, xyz_from_rgb);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            if (!std::isfinite(m.m[i][j])) return false;
            out->matrix[3 * i + j] = static_cast<float>(m.m[i][j]);
        }
    return true;
}
void identity_plan(ifhip_color_plan* out) {
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 256; ++i) out->linear[c][i] = static_cast<float>(srgb_to_linear(i / 255.0));
    for (int k = 0; k < 9; ++k) out->matrix[k] = k % 4 == 0 ? 1.0f : 0.0f;
}


}  // namespace

const char* color_plan_status_text(int status) {
    switch (status) {
    case IFHIP_COLOR_PLANNED: return "planned";
    case IFHIP_COLOR_NOT_CONVERTIBLE: return "not convertible here";
    case IFHIP_COLOR_MALFORMED: return "malformed";
    }
    return "unknown status";
}

ColorPlanResult color_plan_from_icc(const uint8_t* icc, size_t len, ifhip_color_plan* out) {
    const auto bad = [](const char* why) { return ColorPlanResult{IFHIP_COLOR_MALFORMED, why}; };
    const auto no = [](const char* why) { return ColorPlanResult{IFHIP_COLOR_NOT_CONVERTIBLE, why}; };
    if (!icc || !out) return bad("null argument");
    if (len < 132u) return bad("the profile is shorter than an ICC header and a tag count");
    // the profile ends where its header says, or where the bytes end (lcms2 clamps the same way)
    const uint32_t size = static_cast<uint32_t>(len < be32(icc) ? len : be32(icc));
    if (size < 132u) return bad("the profile's own size field is smaller than a header");
    if (be32(icc + 36) != sig('a', 'c', 's', 'p')) return bad("the profile lacks the 'acsp' signature");
    const uint32_t count = be32(icc + 128);
    if (count > 100u) return bad("the tag table claims more than 100 tags");
    if (132u + 12u * count > size) return bad("the tag table runs past the profile");
    const uint32_t cls = be32(icc + 12), space = be32(icc + 16), pcs = be32(icc + 20);
    if (space == sig('G', 'R', 'A', 'Y')) return no("a GRAY colour space");
    if (space == sig('C', 'M', 'Y', 'K')) return no("a CMYK colour space");
    if (space != sig('R', 'G', 'B', ' ')) return no("a colour space other than RGB");
    if (cls == sig('l', 'i', 'n', 'k') || cls == sig('a', 'b', 's', 't') || cls == sig('n', 'm', 'c', 'l')) return no("a device-link, abstract or named-colour profile");
    if (pcs == sig('L', 'a', 'b', ' ')) return no("a Lab connection space");
    if (pcs != sig('X', 'Y', 'Z', ' ')) return bad("the connection space is neither XYZ nor Lab");
    if (find_tag(icc, size, count, sig('A', '2', 'B', '0')).p || find_tag(icc, size, count, sig('D', '2', 'B', '0')).p)
        return no("a LUT-based profile (A2B0)");                           // lcms2 reads the LUT whenever there is one
    Mat3 c;
    static const uint32_t xyz_tags[3] = {sig('r', 'X', 'Y', 'Z'), sig('g', 'X', 'Y', 'Z'), sig('b', 'X', 'Y', 'Z')};
    static const uint32_t trc_tags[3] = {sig('r', 'T', 'R', 'C'), sig('g', 'T', 'R', 'C'), sig('b', 'T', 'R', 'C')};
    for (int k = 0; k < 3; ++k) {
        const Tag t = find_tag(icc, size, count, xyz_tags[k]);
        if (!t.p) return bad("the profile lacks a colourant (rXYZ, gXYZ or bXYZ) inside its length");
        if (t.n < 20u || be32(t.p) != sig('X', 'Y', 'Z', ' ')) return bad("a colourant element is not an XYZ element of one value");
        for (int i = 0; i < 3; ++i) c.m[i][k] = s15f16(t.p + 8 + 4 * i);
    }
    for (int k = 0; k < 3; ++k) {
        Curve cv;
        if (const char* why = read_curve(find_tag(icc, size, count, trc_tags[k]), &cv)) return bad(why);
        for (int i = 0; i < 256; ++i) out->linear[k][i] = static_cast<float>(cv.eval(i / 255.0));
        // cmsLinkProfiles forces black point compensation wherever a version 4 profile meets the perceptual intent, and lcms2's
        // built-in sRGB profile is one.  It is the identity while the source's black is XYZ 0, that is while every curve maps 0
        // to 0 (below 1e-4 it moves no byte by half a step); a curve that lifts black would need lcms2's black point
        // detection, which is not built
        if (cv.eval(0.0) > 1e-4) return no("a tone curve that lifts black (lcms2 compensates the black point)");
    }
    if (!finish_matrix(c, out)) return bad("the colourants give no finite matrix");
    return ColorPlanResult{IFHIP_COLOR_PLANNED, ""};
}

ColorPlanResult color_plan_from_gamma_primaries(double gamma, const double xy[8], ifhip_color_plan* out) {
    if (!xy || !out) return ColorPlanResult{IFHIP_COLOR_MALFORMED, "null argument"};
    // source_profile.rs:225-242: degenerate values, and a neutral gamma with sRGB's primaries, are SourceProfile::Srgb
    bool as_srgb = !(gamma > 0.0) || !std::isfinite(gamma);
    for (int k = 0; k < 8; ++k) as_srgb = as_srgb || !std::isfinite(xy[k]);
    as_srgb = as_srgb || xy[1] == 0.0 || xy[3] == 0.0 || xy[5] == 0.0 || xy[7] == 0.0;
    if (!as_srgb && std::fabs(gamma * 2.2 - 1.0) < 0.05) {
        static const double srgb[8] = {0.3127, 0.3290, 0.64, 0.33, 0.30, 0.60, 0.15, 0.06};
        bool same = true;
        for (int k = 0; k < 8; ++k) same = same && std::fabs(xy[k] - srgb[k]) < 0.01;
        as_srgb = same;
    }
    if (as_srgb) { identity_plan(out); return ColorPlanResult{IFHIP_COLOR_PLANNED, ""}; }
    Mat3 adapted;
    if (!adapted_colourants(xy, &adapted)) return ColorPlanResult{IFHIP_COLOR_MALFORMED, "the cHRM primaries lie on one line"};
    const double exponent = 1.0 / gamma;
    for (int i = 0; i < 256; ++i) {
        const float v = static_cast<float>(clamp01(std::pow(i / 255.0, exponent)));
        out->linear[0][i] = out->linear[1][i] = out->linear[2][i] = v;
    }
    if (!finish_matrix(adapted, out)) return ColorPlanResult{IFHIP_COLOR_MALFORMED, "the gAMA and cHRM values give no finite matrix"};
    return ColorPlanResult{IFHIP_COLOR_PLANNED, ""};
}

}  // namespace ifhip
