// color_icc.hpp -- what the two readers of ICC bytes share (csrc/color_profile.cpp: matrix/TRC profiles as plans;
// csrc/color_link.cpp: GRAY and LUT-based profiles as links): big-endian fields, the tag table, 3 x 3 matrices in f64 and
// the curv / para elements.  Host only, every read bounds-checked against the element's own length; no other file of the
// library.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace ifhip {
namespace icc {

inline uint32_t be32(const uint8_t* p) { return static_cast<uint32_t>(p[0]) << 24 | static_cast<uint32_t>(p[1]) << 16 | static_cast<uint32_t>(p[2]) << 8 | p[3]; }
inline uint32_t be16(const uint8_t* p) { return static_cast<uint32_t>(p[0]) << 8 | p[1]; }
inline double s15f16(const uint8_t* p) { return static_cast<double>(static_cast<int32_t>(be32(p))) / 65536.0; }
constexpr uint32_t sig(char a, char b, char c, char d) {
    return static_cast<uint32_t>(static_cast<uint8_t>(a)) << 24 | static_cast<uint32_t>(static_cast<uint8_t>(b)) << 16 | static_cast<uint32_t>(static_cast<uint8_t>(c)) << 8 | static_cast<uint8_t>(d);
}

struct Mat3 { double m[3][3]; };
inline bool invert(const Mat3& a, Mat3* out) {
    const double (*m)[3] = a.m;
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    if (!std::isfinite(det) || std::fabs(det) < 1e-10) return false;
    out->m[0][0] = c00 / det; out->m[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det; out->m[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
    out->m[1][0] = c01 / det; out->m[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det; out->m[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
    out->m[2][0] = c02 / det; out->m[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det; out->m[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
    return true;
}
inline Mat3 mul(const Mat3& a, const Mat3& b) {
    Mat3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return r;
}
// cmsCreateRGBProfile -> _cmsBuildRGB2XYZtransferMatrix + _cmsAdaptMatrixToD50: the primaries xy[2..8] scaled so that
// R = G = B = 1 is the white xy[0..2], then Bradford (lcms2's LamRigg cone matrix) from that white to D50 = (0.9642, 1, 0.8249).
// Columns R, G, B.  false: the primaries lie on one line.
inline bool adapted_colourants(const double xy[8], Mat3* out) {
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
inline bool srgb_from_xyz(Mat3* out) {
    static const double srgb[8] = {0.3127, 0.3290, 0.64, 0.33, 0.30, 0.60, 0.15, 0.06};
    Mat3 s;
    if (!adapted_colourants(srgb, &s)) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s.m[i][j] = std::nearbyint(s.m[i][j] * 65536.0) / 65536.0;
    return invert(s, out);
}
inline double clamp01(double v) { return v >= 0.0 ? (v <= 1.0 ? v : 1.0) : 0.0; }          // NaN -> 0

struct Tag { const uint8_t* p; uint32_t n; };
// the first element of that signature that lies inside the profile (lcms2's _cmsReadHeader drops the others silently)
inline Tag find_tag(const uint8_t* icc, uint32_t size, uint32_t count, uint32_t want) {
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
inline const char* read_curve(Tag t, Curve* c) {
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

}  // namespace icc
}  // namespace ifhip
