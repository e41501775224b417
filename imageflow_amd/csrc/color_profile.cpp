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

namespace ifhip {
namespace {

uint32_t be32(const uint8_t* p) { return static_cast<uint32_t>(p[0]) << 24 | static_cast<uint32_t>(p[1]) << 16 | static_cast<uint32_t>(p[2]) << 8 | p[3]; }
uint32_t be16(const uint8_t* p) { return static_cast<uint32_t>(p[0]) << 8 | p[1]; }
double s15f16(const uint8_t* p) { return static_cast<double>(static_cast<int32_t>(be32(p))) / 65536.0; }
constexpr uint32_t sig(char a, char b, char c, char d) {
    return static_cast<uint32_t>(static_cast<uint8_t>(a)) << 24 | static_cast<uint32_t>(static_cast<uint8_t>(b)) << 16 | static_cast<uint32_t>(static_cast<uint8_t>(c)) << 8 | static_cast<uint8_t>(d);
}

struct Mat3 { double m[3][3]; };
bool invert(const Mat3& a, Mat3* out) {
    const double (*m)[3] = a.m;
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    if (!std::isfinite(det) || std::fabs(det) < 1e-10) return false;
    out->m[0][0] = c00 / det; out->m[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det; out->m[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
    out->m[1][0] = c01 / det; out->m[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det; out->m[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
    out->m[2][0] = c02 / det; out->m[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det; out->m[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
    return true;
}
Mat3 mul(const Mat3& a, const Mat3& b) {
    Mat3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return r;
}

// cmsCreateRGBProfile -> _cmsBuildRGB2XYZtransferMatrix + _cmsAdaptMatrixToD50: the primaries xy[2..8] scaled so that
// R = G = B = 1 is the white xy[0..2], then Bradford (lcms2's LamRigg cone matrix) from that white to D50 = (0.9642, 1, 0.8249).
// Columns R, G, B.  false: the primaries lie on one line.
bool adapted_colourants(const double xy[8], Mat3* out) {
    const double wx = xy[0], wy = xy[1];
    Mat3 prim, prim_inv;
    for (int k = 0; k < 3; ++k) { prim.m[0][k] = xy[2 + 2 * k]; prim.m[1][k] = xy[3 + 2 * k]; prim.m[2][k] = 1.0 - xy[2 + 2 * k] - xy[3 + 2 * k]; }
    if (!invert(prim, &prim_inv)) return false;
    const double white[3] = {wx / wy, 1.0, (1.0 - wx - wy) / wy};
    Mat3 m;
    for (int k = 0; k < 3; ++k) {
        const double coef = prim_inv.m[k][0] * white[0] + prim_inv.m[k][1] * white[1] + prim_inv.m[k][2] * white[2];
        for (int i = 0; i < 3; ++i) m.m[i][k] = coef * prim.m[i][k];
    }
    const Mat3 cone = {{{0.8951, 0.2664, -0.1614}, {-0.7502, 1.7135, 0.0367}, {0.0389, -0.0685, 1.0296}}};
    Mat3 cone_inv;
    if (!invert(cone, &cone_inv)) return false;
    static const double d50[3] = {0.9642, 1.0, 0.8249};
    Mat3 scale = {{{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}};
    for (int i = 0; i < 3; ++i) {
        const double src = cone.m[i][0] * white[0] + cone.m[i][1] * white[1] + cone.m[i][2] * white[2];
        const double dst = cone.m[i][0] * d50[0] + cone.m[i][1] * d50[1] + cone.m[i][2] * d50[2];
        scale.m[i][i] = dst / src;
    }
    *out = mul(mul(cone_inv, mul(scale, cone)), m);
    return true;
}

// the colourants of lcms2's built-in sRGB profile as its rXYZ / gXYZ / bXYZ tags hold them, rounded to s15.16:
// cmsCreate_sRGBProfile is cmsCreateRGBProfile of D65 = (0.3127, 0.3290) and the BT.709 primaries, so its blue Z is 0.7139 --
// lcms2's D50 -- where the sRGB profile of the IEC has 0.7141
bool srgb_from_xyz(Mat3* out) {
    static const double srgb[8] = {0.3127, 0.3290, 0.64, 0.33, 0.30, 0.60, 0.15, 0.06};
    Mat3 s;
    if (!adapted_colourants(srgb, &s)) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s.m[i][j] = std::nearbyint(s.m[i][j] * 65536.0) / 65536.0;
    return invert(s, out);
}
double clamp01(double v) { return v >= 0.0 ? (v <= 1.0 ? v : 1.0) : 0.0; }          // NaN -> 0
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

// ---- ICC -------------------------------------------------------------------------------------------------------------
struct Tag { const uint8_t* p; uint32_t n; };
// the first element of that signature that lies inside the profile (lcms2's _cmsReadHeader drops the others silently)
Tag find_tag(const uint8_t* icc, uint32_t size, uint32_t count, uint32_t want) {
    for (uint32_t i = 0; i < count; ++i) {
        const uint8_t* e = icc + 132u + 12u * i;
        const uint32_t off = be32(e + 4), n = be32(e + 8);
        if (be32(e) != want) continue;
        if (off > size || n > size - off) continue;
        return Tag{icc + off, n};
    }
    return Tag{nullptr, 0u};
}

struct Curve {
    int kind = 0;                   // 0 identity, 1 gamma, 2 table, 3 + t: para of function type t
    double g = 1.0, p[6] = {0, 0, 0, 0, 0, 0};      // gamma; a b c d e f
    const uint8_t* table = nullptr; // n big-endian u16
    uint32_t n = 0;
    double powp(double e) const { return e > 0.0 ? std::pow(e, g) : 0.0; }
    double eval(double x) const {
        const double a = p[0], b = p[1], c = p[2], d = p[3], e = p[4], f = p[5];
        double y = x;
        switch (kind) {
        case 0: break;
        case 1: case 3: y = std::pow(x, g); break;
        case 2: {
            const double pos = x * static_cast<double>(n - 1u);
            uint32_t k = static_cast<uint32_t>(pos);
            if (k >= n - 1u) { y = be16(table + 2u * (n - 1u)) / 65535.0; break; }
            const double y0 = be16(table + 2u * k) / 65535.0, y1 = be16(table + 2u * k + 2u) / 65535.0;
            y = y0 + (y1 - y0) * (pos - static_cast<double>(k));
            break;
        }
        case 4: y = a == 0.0 ? 0.0 : (x >= -b / a ? powp(a * x + b) : 0.0); break;              // lcms2 cmsgamma.c, type 2
        case 5: y = a == 0.0 ? 0.0 : (x >= -b / a ? powp(a * x + b) + c : c); break;            // type 3
        case 6: y = x >= d ? powp(a * x + b) : c * x; break;                                    // type 4
        case 7: y = x >= d ? powp(a * x + b) + e : c * x + f; break;                            // type 5
        }
        return clamp01(y);
    }
};
const char* read_curve(Tag t, Curve* c) {
    if (!t.p) return "the profile lacks a tone curve (rTRC, gTRC or bTRC) inside its length";
    if (t.n < 12u) return "a tone curve element is shorter than its header";
    const uint32_t type = be32(t.p);
    if (type == sig('c', 'u', 'r', 'v')) {
        const uint32_t n = be32(t.p + 8);
        if (n > 0x7FFFu) return "a curv element claims more than 32767 entries";
        if (12u + 2u * static_cast<uint64_t>(n) > t.n) return "a curv element's entries run past the element";
        if (n == 0u) c->kind = 0;
        else if (n == 1u) { c->kind = 1; c->g = be16(t.p + 12) / 256.0; }
        else { c->kind = 2; c->table = t.p + 12; c->n = n; }
        return nullptr;
    }
    if (type == sig('p', 'a', 'r', 'a')) {
        static const uint32_t n_params[5] = {1u, 3u, 4u, 5u, 7u};
        const uint32_t ft = be16(t.p + 8);
        if (ft > 4u) return "a para element has a function type above 4";
        if (12u + 4u * n_params[ft] > t.n) return "a para element's parameters run past the element";
        c->kind = 3 + static_cast<int>(ft);
        c->g = s15f16(t.p + 12);
        for (uint32_t k = 1; k < n_params[ft]; ++k) c->p[k - 1u] = s15f16(t.p + 12u + 4u * k);
        return nullptr;
    }
    return "a tone curve element is neither curv nor para";
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
