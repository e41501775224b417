// color_link.cpp -- profile -> link on the host, for the two kinds of source profile codecs/lcms2_transform.rs hands to
// lcms2 that csrc/color_profile.cpp turns away:
//   GRAY + kTRC, XYZ PCS   :132-186  TYPE_GRAY_8 -> sRGB: the curve, Y on the D50 axis, sRGB's matrix and curve.  lcms2 resamples
//                          that to 33 nodes and interpolates linearly (cmsopt.c OptimizeByResampling, cmsintrp.c Eval1Input);
//                          here the 256 results are the link
//   RGB + A2B0             :117-130  the LUT element's stages (cmstypes.c Type_LUT8 / Type_LUT16 / Type_LUTA2B_Read; lut8 and
//                          lut16 with an XYZ PCS only), the PCS brought to XYZ, black point compensation, sRGB's matrix and curve, sampled at 33^3 nodes
// The pipeline is restated as lcms2 evaluates it while it samples (cmslut.c): f32 between the stages, 16-bit steps inside the
// tabulated curves and the profile's CLUT (the interpolation of csrc/color_link_core.hpp), f64 inside matrices and
// parametric curves.  The intent is perceptual: A2B0 is the only LUT consulted, D2B0 is refused.  lcms2 forces black point
// compensation here because its sRGB profile is version 4; the source's black is the fixed perceptual black for a version 4
// LUT profile and the L* of device black (at most 50, a = b = 0) otherwise, the destination's is 0.
// Not restated: the pre-linearisation curves lcms2 derives from the transform's grey axis before it samples
// (OptimizeByComputingLinearization); the link samples at uniform device values, and tests/test_color_link_plan.py states what
// that leaves.  No HIP, no other file of the library: tests link this file alone under sanitizers.
#include "color_link.hpp"

#include <cmath>
#include <cstring>

#include "color_icc.hpp"
#include "color_link_core.hpp"

namespace ifhip {
namespace {

using namespace icc;

constexpr double kMaxXyz = 1.0 + 32767.0 / 32768.0;                 // the PCS's XYZ encoding: 0xFFFF is 1.99997
constexpr double kD50[3] = {0.9642, 1.0, 0.8249};                    // lcms2's D50
constexpr double kTolerance = 0.0001;                                // MATRIX_DET_TOLERANCE

uint16_t saturate_word(double d) {                                   // _cmsQuickSaturateWord; NaN -> 0
    d += 0.5;
    if (!(d > 0.0)) return 0;
    if (d >= 65535.0) return 0xFFFFu;
    return static_cast<uint16_t>(std::floor(d));
}

// one curve of a stage: tabulated (16-bit steps, cmsintrp.c LinLerp1D) or parametric (f64, cmsgamma.c DefaultEvalParametricFn)
struct LinkCurve {
    std::vector<uint16_t> table;
    Curve para;                                                      // table.empty(): kind 0 identity, 1 gamma, 3.. para
    void set(const Curve& c) {
        para = c;
        if (c.kind == 2) {
            table.resize(c.n);
            for (uint32_t i = 0; i < c.n; ++i) table[i] = static_cast<uint16_t>(be16(c.table + 2u * i));
        }
    }
    uint16_t eval16(uint16_t v) const {
        const uint32_t domain = static_cast<uint32_t>(table.size()) - 1u;
        if (v == 0xFFFFu || domain == 0u) return table[domain];
        const uint32_t pos = link_fixed_domain(domain * v);          // domain <= 32766: below 2^31
        const uint32_t cell = pos >> 16, rest = pos & 0xFFFFu;
        const uint32_t lo = table[cell], hi = table[cell + 1u];
        return static_cast<uint16_t>((((hi - lo) * rest + 0x8000u) >> 16) + lo);
    }
    double raw(double r) const {
        const double g = para.g, a = para.p[0], b = para.p[1], c = para.p[2], d = para.p[3], e = para.p[4], f = para.p[5];
        const auto powp = [g](double v) { return v > 0.0 ? std::pow(v, g) : 0.0; };
        switch (para.kind) {
        case 1: case 3: return r < 0.0 ? (std::fabs(g - 1.0) < kTolerance ? r : 0.0) : std::pow(r, g);
        case 4: return std::fabs(a) < kTolerance ? 0.0 : (r >= -b / a ? powp(a * r + b) : 0.0);
        case 5: {
            if (std::fabs(a) < kTolerance) return 0.0;
            const double disc = -b / a < 0.0 ? 0.0 : -b / a;
            if (r < disc) return c;
            return a * r + b > 0.0 ? std::pow(a * r + b, g) + c : 0.0;
        }
        case 6: return r >= d ? powp(a * r + b) : r * c;
        case 7: return r >= d ? powp(a * r + b) + e : r * c + f;
        }
        return r;
    }
    float eval(float v) const {
        if (!table.empty()) return static_cast<float>(eval16(saturate_word(v * 65535.0)) / 65535.0);
        return static_cast<float>(raw(v));
    }
};

struct Stage {
    enum Kind { kCurves, kMatrix, kClut, kLabToXyz, kSrgbCurve } kind = kCurves;
    LinkCurve curve[3];
    double m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, off[3] = {0, 0, 0};
    uint32_t grid[3] = {0, 0, 0};
    std::vector<uint16_t> clut;                                      // [r][g][b][3]
};

double lab_f_inverse(double t) { return t <= 24.0 / 116.0 ? (108.0 / 841.0) * (t - 16.0 / 116.0) : t * t * t; }
void lab_to_xyz(double L, double a, double b, double xyz[3]) {      // cmspcs.c cmsLab2XYZ, D50
    const double y = (L + 16.0) / 116.0;
    xyz[0] = lab_f_inverse(y + 0.002 * a) * kD50[0];
    xyz[1] = lab_f_inverse(y) * kD50[1];
    xyz[2] = lab_f_inverse(y - 0.005 * b) * kD50[2];
}
double srgb_curve_inverse(double r) {                                // parametric type -4 of sRGB's own parameters
    const double g = 2.4, a = 1.0 / 1.055, b = 0.055 / 1.055, c = 1.0 / 12.92, d = 0.04045;
    const double disc = std::pow(a * d + b, g);
    return r >= disc ? (std::pow(r, 1.0 / g) - b) / a : r / c;
}

void run_stage(const Stage& s, float v[3]) {
    switch (s.kind) {
    case Stage::kCurves:
        for (int k = 0; k < 3; ++k) v[k] = s.curve[k].eval(v[k]);
        break;
    case Stage::kMatrix: {
        float o[3];
        for (int i = 0; i < 3; ++i) {
            double t = 0.0;
            for (int j = 0; j < 3; ++j) t += static_cast<double>(v[j]) * s.m[3 * i + j];
            o[i] = static_cast<float>(t + s.off[i]);
        }
        std::memcpy(v, o, sizeof o);
        break;
    }
    case Stage::kClut: {                                             // cmsintrp.c TetrahedralInterp16 on the profile's own grid
        uint32_t cell[3], rest[3];
        for (int k = 0; k < 3; ++k) {
            const uint32_t in = saturate_word(v[k] * 65535.0);
            const uint32_t pos = link_fixed_domain(in * (s.grid[k] - 1u));
            cell[k] = pos >> 16; rest[k] = pos & 0xFFFFu;
        }
        const uint32_t sz = 3u, sy = 3u * s.grid[2], sx = sy * s.grid[1];
        const uint16_t* t = s.clut.data() + cell[0] * sx + cell[1] * sy + cell[2] * sz;
        const LinkWalk w = link_walk(rest[0], rest[1], rest[2], sx, sy, sz);
        for (uint32_t c = 0; c < 3u; ++c)
            v[c] = link_interp(t[c], t[w.da + c], t[w.da + w.db + c], t[w.da + w.db + w.dc + c], w.ra, w.rb, w.rc) / 65535.0f;
        break;
    }
    case Stage::kLabToXyz: {                                         // cmslut.c EvaluateLab2XYZ: the version 4 encoding
        double xyz[3];
        lab_to_xyz(v[0] * 100.0, v[1] * 255.0 - 128.0, v[2] * 255.0 - 128.0, xyz);
        for (int k = 0; k < 3; ++k) v[k] = static_cast<float>(xyz[k] / kMaxXyz);
        break;
    }
    case Stage::kSrgbCurve:
        for (int k = 0; k < 3; ++k) v[k] = static_cast<float>(srgb_curve_inverse(v[k]));
        break;
    }
}

typedef std::vector<Stage> Pipeline;

struct Failure { int status; const char* why; };
constexpr Failure kFine{IFHIP_COLOR_PLANNED, ""};
Failure bad(const char* why) { return Failure{IFHIP_COLOR_MALFORMED, why}; }
Failure no(const char* why) { return Failure{IFHIP_COLOR_NOT_CONVERTIBLE, why}; }

bool is_identity(const double m[9]) {                                // _cmsMAT3isIdentity: within 1 / 65535
    for (int k = 0; k < 9; ++k)
        if (std::fabs(m[k] - (k % 4 == 0 ? 1.0 : 0.0)) > 1.0 / 65535.0) return false;
    return true;
}

// mft1 / mft2: [matrix] [input tables] [CLUT] [output tables]
Failure read_lut8_or_16(Tag t, bool wide, Pipeline* p) {
    const uint32_t head = wide ? 52u : 48u;
    if (t.n < head) return bad("a lut8 or lut16 element is shorter than its header");
    const uint32_t n_in = t.p[8], n_out = t.p[9], grid = t.p[10];
    if (n_in != 3u || n_out != 3u) return bad("the A2B0 element of an RGB profile does not have 3 inputs and 3 outputs");
    if (grid < 2u) return bad("the A2B0 element has a grid of fewer than 2 points");
    Stage mat;
    mat.kind = Stage::kMatrix;
    for (int k = 0; k < 9; ++k) mat.m[k] = s15f16(t.p + 12 + 4 * k);
    if (!is_identity(mat.m)) p->push_back(mat);                      // lcms2 applies it whatever the connection space is
    const uint32_t in_entries = wide ? be16(t.p + 48) : 256u, out_entries = wide ? be16(t.p + 50) : 256u;
    if (in_entries > 0x7FFFu || out_entries > 0x7FFFu) return bad("a lut16 element claims tables of more than 32767 entries");
    if (in_entries == 1u || out_entries == 1u) return bad("a lut16 element claims tables of one entry");
    const uint64_t width = wide ? 2u : 1u;
    const uint64_t clut_values = static_cast<uint64_t>(grid) * grid * grid * 3u;
    const uint64_t need = head + width * (3ull * in_entries + clut_values + 3ull * out_entries);
    if (need > t.n) return bad("the tables of a lut8 or lut16 element run past the element");
    const uint8_t* q = t.p + head;
    const auto value = [&](uint64_t i) { return static_cast<uint16_t>(wide ? be16(q + 2u * i) : q[i] * 257u); };
    const auto tables = [&](uint32_t entries) {
        if (!entries) return;
        Stage s;
        s.kind = Stage::kCurves;
        for (int k = 0; k < 3; ++k) {
            s.curve[k].table.resize(entries);
            for (uint32_t i = 0; i < entries; ++i) s.curve[k].table[i] = value(static_cast<uint64_t>(k) * entries + i);
        }
        p->push_back(std::move(s));
        q += width * 3u * entries;
    };
    tables(in_entries);
    {
        Stage s;
        s.kind = Stage::kClut;
        s.grid[0] = s.grid[1] = s.grid[2] = grid;
        s.clut.resize(clut_values);
        for (uint64_t i = 0; i < clut_values; ++i) s.clut[i] = value(i);
        p->push_back(std::move(s));
        q += width * clut_values;
    }
    tables(out_entries);
    return kFine;
}

// three curv / para elements one behind the other, each padded to 4 bytes
Failure read_curve_set(Tag t, uint32_t offset, Pipeline* p) {
    Stage s;
    s.kind = Stage::kCurves;
    for (int k = 0; k < 3; ++k) {
        if (offset > t.n || t.n - offset < 12u) return bad("a curve of the mAB element lies past the element");
        const Tag one{t.p + offset, t.n - offset};
        Curve c;
        if (const char* why = read_curve(one, &c)) return bad(why);
        s.curve[k].set(c);
        static const uint32_t n_params[5] = {1u, 3u, 4u, 5u, 7u};
        const uint32_t size = be32(one.p) == sig('c', 'u', 'r', 'v') ? 12u + 2u * be32(one.p + 8) : 12u + 4u * n_params[be16(one.p + 8)];
        offset += (size + 3u) & ~3u;
    }
    p->push_back(std::move(s));
    return kFine;
}

// mAB: A curves, CLUT, M curves, matrix, B curves -- whichever the element has, in that order
Failure read_lut_a_to_b(Tag t, Pipeline* p) {
    if (t.n < 32u) return bad("an mAB element is shorter than its header");
    if (t.p[8] != 3u || t.p[9] != 3u) return bad("the A2B0 element of an RGB profile does not have 3 inputs and 3 outputs");
    const uint32_t off_b = be32(t.p + 12), off_mat = be32(t.p + 16), off_m = be32(t.p + 20), off_c = be32(t.p + 24), off_a = be32(t.p + 28);
    Failure f = kFine;
    if (off_a && (f = read_curve_set(t, off_a, p)).status) return f;
    if (off_c) {
        if (off_c > t.n || t.n - off_c < 20u) return bad("the CLUT of the mAB element lies past the element");
        const uint8_t* q = t.p + off_c;
        Stage s;
        s.kind = Stage::kClut;
        uint64_t values = 3u;
        for (int k = 0; k < 3; ++k) {
            s.grid[k] = q[k];
            if (s.grid[k] < 2u) return bad("the A2B0 element has a grid of fewer than 2 points");
            values *= s.grid[k];
        }
        const uint32_t width = q[16];
        if (width != 1u && width != 2u) return bad("the CLUT of the mAB element has entries of neither 1 nor 2 bytes");
        if (values * width > t.n - off_c - 20u) return bad("the CLUT of the mAB element runs past the element");
        s.clut.resize(values);
        for (uint64_t i = 0; i < values; ++i) s.clut[i] = static_cast<uint16_t>(width == 2u ? be16(q + 20u + 2u * i) : q[20u + i] * 257u);
        p->push_back(std::move(s));
    }
    if (off_m && (f = read_curve_set(t, off_m, p)).status) return f;
    if (off_mat) {
        if (off_mat > t.n || t.n - off_mat < 48u) return bad("the matrix of the mAB element lies past the element");
        Stage s;
        s.kind = Stage::kMatrix;
        for (int k = 0; k < 9; ++k) s.m[k] = s15f16(t.p + off_mat + 4 * k);
        for (int k = 0; k < 3; ++k) s.off[k] = s15f16(t.p + off_mat + 36 + 4 * k);
        p->push_back(s);
    }
    if (off_b && (f = read_curve_set(t, off_b, p)).status) return f;
    return kFine;
}

// cmsio1.c / cmscnvrt.c: what follows the source's own stages.  `black`: the source's black point, XYZ
void append_pcs_to_srgb(bool pcs_lab, const double black[3], Pipeline* p, bool* fine) {
    if (pcs_lab) { Stage s; s.kind = Stage::kLabToXyz; p->push_back(s); }
    if (black[0] != 0.0 || black[1] != 0.0 || black[2] != 0.0) {    // ComputeBlackPointCompensation towards sRGB's black, 0
        Stage s;
        s.kind = Stage::kMatrix;
        for (int k = 0; k < 3; ++k) {
            const double t = black[k] - kD50[k];
            s.m[4 * k] = (0.0 - kD50[k]) / t;
            s.off[k] = -kD50[k] * (0.0 - black[k]) / t / kMaxXyz;
        }
        p->push_back(s);
    }
    Mat3 inv{};
    *fine = srgb_from_xyz(&inv);
    Stage s;
    s.kind = Stage::kMatrix;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s.m[3 * i + j] = inv.m[i][j] * kMaxXyz;
    p->push_back(s);
    Stage c;
    c.kind = Stage::kSrgbCurve;
    p->push_back(c);
}

// cmssamp.c BlackPointAsDarkerColorant: the L* of device black, at most 50 and neutral, as XYZ
void black_from_lightness(double L, double black[3]) {
    L = L > 0.0 ? (L < 50.0 ? L : 50.0) : 0.0;                       // NaN -> 0
    lab_to_xyz(L, 0.0, 0.0, black);
}
double lightness_of_y(double y) {
    const double f = y <= (24.0 / 116.0) * (24.0 / 116.0) * (24.0 / 116.0) ? (841.0 / 108.0) * y + 16.0 / 116.0 : std::cbrt(y);
    return 116.0 * f - 16.0;
}

void sample(const Pipeline& p, const float in[3], uint16_t out[3]) {
    float v[3] = {in[0], in[1], in[2]};
    for (const Stage& s : p) run_stage(s, v);
    for (int k = 0; k < 3; ++k) out[k] = saturate_word(v[k] * 65535.0);
}
uint16_t grid_value(uint32_t i) { return saturate_word(i * 65535.0 / (kLinkGrid - 1u)); }   // _cmsQuantizeVal

Failure gray_link(const uint8_t* icc, uint32_t size, uint32_t count, uint32_t pcs, ColorLink* out) {
    if (find_tag(icc, size, count, sig('A', '2', 'B', '0')).p || find_tag(icc, size, count, sig('D', '2', 'B', '0')).p)
        return no("a GRAY profile with a LUT (A2B0)");
    if (pcs == sig('L', 'a', 'b', ' ')) return no("a GRAY profile with a Lab connection space");
    const Tag trc = find_tag(icc, size, count, sig('k', 'T', 'R', 'C'));
    if (!trc.p) return bad("the GRAY profile lacks its tone curve (kTRC) inside its length");
    Curve c;
    if (const char* why = read_curve(trc, &c)) return bad(why);
    LinkCurve curve;
    curve.set(c);
    // cmsio1.c BuildGrayInputMatrixPipeline: the curve, then Y along D50 in the PCS's encoding
    double black[3];
    black_from_lightness(lightness_of_y(curve.eval(0.0f)), black);
    Pipeline tail;
    bool fine = true;
    append_pcs_to_srgb(false, black, &tail, &fine);
    if (!fine) return bad("sRGB's colourants give no matrix");
    uint16_t node[kLinkGrid];                                        // lcms2 keeps three channels; they are equal up to the matrix's rounding: G stands for all
    for (uint32_t i = 0; i < kLinkGrid; ++i) {
        const float y = curve.eval(grid_value(i) / 65535.0f);
        float v[3];
        for (int k = 0; k < 3; ++k) v[k] = static_cast<float>(static_cast<double>(y) * (kD50[k] / kMaxXyz));
        uint16_t o[3];
        sample(tail, v, o);
        node[i] = o[1];
    }
    for (uint32_t g = 0; g < 256u; ++g) {                            // cmsintrp.c Eval1Input on 257 * g
        const uint32_t pos = link_position(g), cell = pos >> 16, rest = pos & 0xFFFFu;
        const uint32_t lo = node[cell], hi = node[rest ? cell + 1u : cell];
        out->gray[g] = static_cast<uint8_t>(link_to_byte(((((hi - lo) * rest + 0x8000u) >> 16) + lo) & 0xFFFFu));
    }
    out->kind = kColorLinkGray;
    return kFine;
}

Failure rgb_link(const uint8_t* icc, uint32_t size, uint32_t count, uint32_t pcs, bool v4, ColorLink* out) {
    if (find_tag(icc, size, count, sig('D', '2', 'B', '0')).p) return no("a floating-point LUT (D2B0)");
    const Tag lut = find_tag(icc, size, count, sig('A', '2', 'B', '0'));
    if (!lut.p) return no("an RGB profile without A2B0 (a matrix/TRC profile is a plan, not a link)");
    if (lut.n < 12u) return bad("the A2B0 element is shorter than its header");
    const bool pcs_lab = pcs == sig('L', 'a', 'b', ' ');
    const uint32_t type = be32(lut.p);
    // measured against lcms2 (tests/test_color_link_plan.py): with a Lab PCS behind lut8 / lut16 tables the uniform sampling lands
    // up to 14 away from lcms2's pre-linearised one, and not only where a channel clips; mAB stays within 1
    if (pcs_lab && (type == sig('m', 'f', 't', '1') || type == sig('m', 'f', 't', '2'))) return no("a lut8 or lut16 element with a Lab connection space");
    Pipeline p;
    Failure f = kFine;
    if (type == sig('m', 'f', 't', '1')) f = read_lut8_or_16(lut, false, &p);
    else if (type == sig('m', 'f', 't', '2')) f = read_lut8_or_16(lut, true, &p);
    else if (type == sig('m', 'A', 'B', ' ')) f = read_lut_a_to_b(lut, &p);
    else return bad("the A2B0 element is neither mft1, mft2 nor mAB");
    if (f.status) return f;
    double black[3] = {0.00336, 0.0034731, 0.00287};                 // cmsPERCEPTUAL_BLACK: every version 4 LUT profile
    if (!v4) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        for (const Stage& s : p) run_stage(s, v);
        black_from_lightness(pcs_lab ? v[0] * 100.0 : lightness_of_y(v[1] * kMaxXyz), black);
    }
    bool fine = true;
    append_pcs_to_srgb(pcs_lab, black, &p, &fine);
    if (!fine) return bad("sRGB's colourants give no matrix");
    out->nodes.resize(kLinkNodes);
    float in[3];
    uint16_t o[3];
    for (uint32_t r = 0; r < kLinkGrid; ++r)
        for (uint32_t g = 0; g < kLinkGrid; ++g)
            for (uint32_t b = 0; b < kLinkGrid; ++b) {
                in[0] = grid_value(r) / 65535.0f; in[1] = grid_value(g) / 65535.0f; in[2] = grid_value(b) / 65535.0f;
                sample(p, in, o);
                out->nodes[(r * kLinkGrid + g) * kLinkGrid + b] = o[0] | static_cast<uint64_t>(o[1]) << 16 | static_cast<uint64_t>(o[2]) << 32;
            }
    out->kind = kColorLinkRgb;
    return kFine;
}

}  // namespace

ColorPlanResult color_link_from_icc(const uint8_t* icc, size_t len, bool frame_is_gray, ColorLink* out) {
    const auto done = [](Failure f) { return ColorPlanResult{f.status, f.why}; };
    if (!icc || !out) return done(bad("null argument"));
    if (len < 132u) return done(bad("the profile is shorter than an ICC header and a tag count"));
    const uint32_t size = static_cast<uint32_t>(len < be32(icc) ? len : be32(icc));
    if (size < 132u) return done(bad("the profile's own size field is smaller than a header"));
    if (be32(icc + 36) != sig('a', 'c', 's', 'p')) return done(bad("the profile lacks the 'acsp' signature"));
    const uint32_t count = be32(icc + 128);
    if (count > 100u) return done(bad("the tag table claims more than 100 tags"));
    if (132u + 12u * count > size) return done(bad("the tag table runs past the profile"));
    const uint32_t cls = be32(icc + 12), space = be32(icc + 16), pcs = be32(icc + 20);
    if (space == sig('C', 'M', 'Y', 'K')) return done(no("a CMYK colour space"));
    if (space != sig('R', 'G', 'B', ' ') && space != sig('G', 'R', 'A', 'Y')) return done(no("a colour space other than RGB and GRAY"));
    if (cls == sig('l', 'i', 'n', 'k') || cls == sig('a', 'b', 's', 't') || cls == sig('n', 'm', 'c', 'l')) return done(no("a device-link, abstract or named-colour profile"));
    if (pcs != sig('X', 'Y', 'Z', ' ') && pcs != sig('L', 'a', 'b', ' ')) return done(bad("the connection space is neither XYZ nor Lab"));
    ColorLink link;
    Failure f = kFine;
    if (space == sig('G', 'R', 'A', 'Y')) {
        if (!frame_is_gray) return done(no("a GRAY profile on a colour frame"));
        f = gray_link(icc, size, count, pcs, &link);
    } else {
        f = rgb_link(icc, size, count, pcs, be32(icc + 8) >= 0x04000000u, &link);
    }
    if (f.status == IFHIP_COLOR_PLANNED) *out = std::move(link);
    return done(f);
}

}  // namespace ifhip
