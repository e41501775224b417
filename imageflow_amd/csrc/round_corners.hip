// round_corners.hip -- gfx950 kernel + C ABI for graphics/rounded_corners.rs::flow_bitmap_bgra_clear_around_rounded_corners
// (:187-346), the pixel work of RoundImageCornersMut (flow/nodes/round_corners.rs:56-93) and of the querystring's
// s.roundcorners key.
//
// The reference walks the quadrants TL, TR, BL, BR in turn; each fills the rows above / below a circle, the edge strips
// beside it and, row by row, the matte outside its arc, and blends the anti-aliased ring.  Quadrants may touch the same
// pixel (a radius of 49.5 on a 99-px side reaches row 49 from both halves) and a blend reads what an earlier quadrant
// wrote, so the result depends on that order.  The host here restates get_radius and plan_quadrants in f32 exactly, and
// covers every pixel any quadrant touches with disjoint rectangles; ONE launch runs one lane per covered pixel, and that
// lane applies the four quadrants' actions in the reference's order (fill, blend or nothing), reading the pixel only
// when it blends and writing it only when something changed.
//
// Rust semantics kept: f32 throughout (-ffp-contract=off, correctly rounded sqrtf), `f32::max / min` drop a NaN
// operand, `ceil` / `floor` then `as usize` saturate, linear_to_srgb_lut(NaN) reads index 0, the alpha is uchar_clamp_ff,
// a fill writes the matte's raw bytes, and the blend reads the stored alpha byte whatever the frame's format.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "hip_entry.hpp"

namespace ifhip {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxRects = 64;

// one QuadrantInfo (:146-159) with everything the per-pixel actions need, worked out on the host
struct Quad {
    uint32_t fill_top;          // TopLeft of a tall circle: rows [0, fill_top) := matte (:218-221); else 0
    uint32_t fill_bottom;       // BottomLeft of a tall circle: rows [fill_bottom, h) := matte (:222-225); else h
    uint32_t strip_x0, strip_x1;            // edge strips (:248-257): columns [strip_x0, strip_x1) of the rows
    uint32_t strip_a0, strip_a1, strip_b0, strip_b1;   // [a0, a1) and [b0, b1)
    uint32_t arc_y0, arc_y1;    // rows start_y..end_y (:226-236)
    uint32_t is_left;
    float cx, cy, roi, ros, raw, roi2, ros2; // centre, radius of influence / solid, aliasing width, squares (:263-268)
};

struct Args {
    uint8_t* bgra;
    size_t image_bytes;
    uint32_t w, h, stride, n_rects;
    uint32_t matte;             // B, G, R, A bytes (Color32 0xAARRGGBB)
    float mb, mg, mr, ma;       // srgb_to_floatspace of the matte channels, matte alpha / 255 (:200-205)
    const float* s2l;
    const uint8_t* l2s;
    Quad q[4];
    uint32_t rect[kMaxRects][4];            // x0, y0, w, h -- disjoint, together covering every touched pixel
    uint32_t block0[kMaxRects + 1];         // first workgroup of each rectangle; block0[n_rects] = workgroups per frame
};

__host__ __device__ inline uint32_t sat_u32(float v) {     // `as usize` (saturating, NaN -> 0), then held in 32 bits
    return !(v > 0.0f) ? 0u : v >= 4294967296.0f ? 0xFFFFFFFFu : static_cast<uint32_t>(v);
}

__device__ __forceinline__ uint8_t uchar_clamp_ff(float v) {        // graphics/color.rs:101-108 (as resample_device.hpp)
    const float c = __builtin_fminf(v, 300.0f);
    const float f = __builtin_floorf(c);
    int i = static_cast<int>(f) + ((c - f) >= 0.5f ? 1 : 0);
    i = i > 255 ? 255 : i;
    return (v >= 0.0f) ? static_cast<uint8_t>(i) : static_cast<uint8_t>(0);
}

__device__ __forceinline__ uint32_t l2s(const Args& a, float v) {  // linear_to_srgb_lut (lut.rs:4-8): NaN -> index 0
    const float s = __builtin_fminf(__builtin_fmaxf(v * 16383.0f, 0.0f), 16383.0f);
    return a.l2s[static_cast<uint32_t>(s)];
}

// :314-340 -- the anti-aliased blend of the matte over the stored pixel
__device__ __forceinline__ uint32_t blend(const Args& a, uint32_t px, float intensity) {
    const float pa = static_cast<float>(static_cast<int>(px >> 24)) * (1.0f / 255.0f) * (1.0f - intensity);
    const float ma = (1.0f - pa) * a.ma;
    const float fa = ma + pa;                                   // 0 with a transparent matte over alpha 0: 0/0 = NaN -> 0
    const uint32_t b = l2s(a, (a.s2l[px & 255u] * pa + a.mb * ma) / fa);
    const uint32_t g = l2s(a, (a.s2l[(px >> 8) & 255u] * pa + a.mg * ma) / fa);
    const uint32_t r = l2s(a, (a.s2l[(px >> 16) & 255u] * pa + a.mr * ma) / fa);
    return b | (g << 8) | (r << 16) | (static_cast<uint32_t>(uchar_clamp_ff(255.0f * fa)) << 24);
}

__global__ void __launch_bounds__(kThreads) round_corners_kernel(const Args a) {
    // the rectangle of this workgroup (uniform): the last r with block0[r] <= blockIdx.x
    uint32_t lo = 0, hi = a.n_rects;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.block0[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    const uint32_t rw = a.rect[lo][2];
    const uint32_t i = (blockIdx.x - a.block0[lo]) * kThreads + threadIdx.x;
    if (i >= rw * a.rect[lo][3]) return;
    const uint32_t ry = i / rw;
    const uint32_t x = a.rect[lo][0] + (i - ry * rw), y = a.rect[lo][1] + ry;
    uint32_t* p = reinterpret_cast<uint32_t*>(a.bgra + static_cast<size_t>(blockIdx.y) * a.image_bytes + static_cast<size_t>(y) * a.stride) + x;
    uint32_t px = 0;
    bool have = false, dirty = false;
    const float xf = static_cast<float>(x) + 0.5f, yf = static_cast<float>(y) + 0.5f, W = static_cast<float>(a.w);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Quad& q = a.q[k];
        bool fill = y < q.fill_top || y >= q.fill_bottom;
        fill |= x >= q.strip_x0 && x < q.strip_x1 && ((y >= q.strip_a0 && y < q.strip_a1) || (y >= q.strip_b0 && y < q.strip_b1));
        if (!fill && y >= q.arc_y0 && y < q.arc_y1) {                                  // :270-342
            const float yd = __builtin_fabsf(q.cy - yf);
            const float yd2 = yd * yd;
            const float xs = __builtin_sqrtf(__builtin_fmaxf(q.ros2 - yd2, 0.0f));
            const float xi = __builtin_sqrtf(__builtin_fmaxf(q.roi2 - yd2, 0.0f));
            uint32_t from, to;
            if (q.is_left) {
                const uint32_t ei1 = sat_u32(__builtin_fmaxf(__builtin_floorf(q.cx - xi), 0.0f));
                fill = x < ei1;                                                         // row_pixels[0..ei1].fill
                from = ei1; to = sat_u32(__builtin_fmaxf(__builtin_ceilf(q.cx - xs), 0.0f));
            } else {
                const uint32_t ei2 = sat_u32(__builtin_fminf(__builtin_ceilf(q.cx + xi), W));
                fill = x >= ei2;                                                        // row_pixels[ei2..w].fill
                from = sat_u32(__builtin_fminf(__builtin_floorf(q.cx + xs), W)); to = ei2;
            }
            if (!fill && x >= from && x < to) {
                const float dx = q.cx - xf;
                const float d = __builtin_sqrtf(dx * dx + yd2);
                if (d > q.roi) fill = true;
                else if (d > q.ros) {
                    if (!have) { px = *p; have = true; }
                    px = blend(a, px, (d - q.ros) / q.raw);
                    dirty = true;
                }
            }
        }
        if (fill) { px = a.matte; have = true; dirty = true; }
    }
    if (dirty) *p = px;
}

// get_radius (:5-32) -> the four radii TL, TR, BL, BR, or circle
bool get_radius(int mode, const float* radii, uint32_t w, uint32_t h, float out[4]) {
    const float sd = static_cast<float>(std::min(w, h));
    auto clampf = [](float v, float lo, float hi) { return v < lo ? lo : v > hi ? hi : v; };   // f32::clamp: NaN stays NaN
    auto pct = [&](float p) { return sd * clampf(p, 0.0f, 100.0f) / 200.0f; };
    auto pxl = [&](float p) { return clampf(p, 0.0f, sd / 2.0f); };
    const float tl = radii[0], tr = radii[1], br = radii[2], bl = radii[3];           // JSON order
    switch (mode) {
        case IFHIP_ROUND_CORNERS_PERCENTAGE: out[0] = out[1] = out[2] = out[3] = pct(tl); return false;
        case IFHIP_ROUND_CORNERS_PIXELS: out[0] = out[1] = out[2] = out[3] = pxl(tl); return false;
        case IFHIP_ROUND_CORNERS_PERCENTAGE_CUSTOM: out[0] = pct(tl); out[1] = pct(tr); out[2] = pct(bl); out[3] = pct(br); return false;
        default: out[0] = pxl(tl); out[1] = pxl(tr); out[2] = pxl(bl); out[3] = pxl(br); return false;   // PIXELS_CUSTOM
        case IFHIP_ROUND_CORNERS_CIRCLE: return true;
    }
}

// plan_quadrants (:40-137) and the per-quadrant set-up of :217-268, in the reference's f32 arithmetic
void plan(int mode, const float* radii, uint32_t w, uint32_t h, Quad q[4]) {
    float r[4];
    uint32_t sw = w, sh = h, ox = 0, oy = 0;
    if (get_radius(mode, radii, w, h, r)) {                                              // Circle (:46-62)
        sw = sh = std::min(w, h);
        ox = static_cast<uint32_t>(std::max<int64_t>(static_cast<int64_t>(w) - h, 0) / 2);
        oy = static_cast<uint32_t>(std::max<int64_t>(static_cast<int64_t>(h) - w, 0) / 2);
        r[0] = r[1] = r[2] = r[3] = static_cast<float>(sw) / 2.0f;
    }
    const uint32_t rhw = sw / 2, bhh = sh / 2, lhw = sw - rhw, thh = sh - bhh;
    const uint32_t qx[4] = {0, lhw, 0, lhw}, qy[4] = {0, 0, thh, thh}, qw[4] = {lhw, rhw, lhw, rhw}, qh[4] = {thh, thh, bhh, bhh};
    const float SW = static_cast<float>(sw), SH = static_cast<float>(sh);
    const float cxs[4] = {r[0], SW - r[1], r[2], SW - r[3]}, cys[4] = {r[0], r[1], SH - r[2], SH - r[3]};
    const float vo = 0.56419f;                                                           // :212
    for (int k = 0; k < 4; ++k) {
        Quad& o = q[k];
        const bool top = k < 2, left = (k & 1) == 0;
        const uint64_t x = qx[k] + ox, y = qy[k] + oy, right = x + qw[k], bottom = y + qh[k];
        const float rad = r[k];
        o.fill_top = k == 0 && y > 0 ? static_cast<uint32_t>(y) : 0u;
        o.fill_bottom = k == 2 && h > bottom ? static_cast<uint32_t>(bottom) : h;
        const uint64_t rc = static_cast<uint64_t>(std::isnan(rad) || rad <= 0.f ? 0.f : std::ceil(rad));   // `ceil() as usize`
        const uint64_t start_y = top ? y : bottom - rc, end_y = top ? y + rc : bottom;  // (usize; never wraps: rc <= side)
        o.arc_y0 = static_cast<uint32_t>(std::min<uint64_t>(start_y, 0xFFFFFFFFu));
        o.arc_y1 = static_cast<uint32_t>(std::min<uint64_t>(end_y, 0xFFFFFFFFu));
        o.strip_x0 = left ? 0u : static_cast<uint32_t>(right);
        o.strip_x1 = left ? static_cast<uint32_t>(x) : w;
        if (o.strip_x0 == o.strip_x1) o.strip_x0 = o.strip_x1 = 0;
        o.strip_a0 = static_cast<uint32_t>(y); o.strip_a1 = static_cast<uint32_t>(start_y);   // `quadrant.y..start_y as u32`
        o.strip_b0 = static_cast<uint32_t>(end_y); o.strip_b1 = static_cast<uint32_t>(bottom);
        o.is_left = left ? 1u : 0u;
        o.cx = cxs[k] + static_cast<float>(ox);                                          // :58-59 (+= 0 when not a circle)
        o.cy = cys[k] + static_cast<float>(oy);
        o.roi = rad + (1.0f - vo);
        o.ros = rad - vo;
        o.raw = o.roi - o.ros;
        o.roi2 = o.roi * o.roi;
        o.ros2 = o.ros * o.ros;
    }
}

struct Box { uint32_t x0, x1, y0, y1; };

// disjoint rectangles covering every pixel a quadrant may touch: the boxes of the fills, strips and arc rows, cut on their
// edges, the covered cells of each band of rows merged into runs, equal runs of consecutive bands into one rectangle.
// More than kMaxRects pieces: the whole frame (always a valid cover -- the lanes decide exactly).
uint32_t cover(const Quad q[4], uint32_t w, uint32_t h, uint32_t rects[kMaxRects][4]) {
    std::vector<Box> boxes;
    auto add = [&](uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1) {
        x1 = std::min(x1, w); y1 = std::min(y1, h);
        if (x0 < x1 && y0 < y1) boxes.push_back({x0, x1, y0, y1});
    };
    for (int k = 0; k < 4; ++k) {
        const Quad& o = q[k];
        add(0, w, 0, o.fill_top);
        add(0, w, o.fill_bottom, h);
        add(o.strip_x0, o.strip_x1, o.strip_a0, o.strip_a1);
        add(o.strip_x0, o.strip_x1, o.strip_b0, o.strip_b1);
        if (o.arc_y0 < o.arc_y1) {
            // left: every touched column is below ceil(cx) (ei1 <= floor(cx), es1 <= ceil(cx)); right: at or above floor(cx)
            if (o.is_left) add(0, sat_u32(std::ceil(o.cx)) == 0xFFFFFFFFu ? w : sat_u32(std::ceil(o.cx)) + 1u, o.arc_y0, o.arc_y1);
            else { const uint32_t f = sat_u32(std::floor(o.cx)); add(f > 0 ? f - 1u : 0u, w, o.arc_y0, o.arc_y1); }
        }
    }
    if (boxes.empty()) return 0;
    std::vector<uint32_t> xs{0, w}, ys{0, h};
    for (const Box& b : boxes) { xs.push_back(b.x0); xs.push_back(b.x1); ys.push_back(b.y0); ys.push_back(b.y1); }
    std::sort(xs.begin(), xs.end()); xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    std::sort(ys.begin(), ys.end()); ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
    std::vector<Box> out, open;                          // open: the rectangles of the previous band (may grow down)
    for (size_t j = 0; j + 1 < ys.size(); ++j) {
        const uint32_t y0 = ys[j], y1 = ys[j + 1];
        std::vector<Box> runs;
        for (size_t i = 0; i + 1 < xs.size(); ++i) {
            const uint32_t x0 = xs[i], x1 = xs[i + 1];
            bool covered = false;
            for (const Box& b : boxes) covered |= b.x0 <= x0 && x1 <= b.x1 && b.y0 <= y0 && y1 <= b.y1;
            if (!covered) continue;
            if (!runs.empty() && runs.back().x1 == x0) runs.back().x1 = x1;
            else runs.push_back({x0, x1, y0, y1});
        }
        std::vector<Box> next;
        for (Box r : runs) {
            auto it = std::find_if(open.begin(), open.end(), [&](const Box& b) { return b.x0 == r.x0 && b.x1 == r.x1 && b.y1 == y0; });
            if (it != open.end()) { r.y0 = it->y0; open.erase(it); }
            next.push_back(r);
        }
        out.insert(out.end(), open.begin(), open.end());
        open = next;
    }
    out.insert(out.end(), open.begin(), open.end());
    if (out.size() > kMaxRects) out.assign(1, Box{0, w, 0, h});
    for (size_t i = 0; i < out.size(); ++i) {
        rects[i][0] = out[i].x0; rects[i][1] = out[i].y0; rects[i][2] = out[i].x1 - out[i].x0; rects[i][3] = out[i].y1 - out[i].y0;
    }
    return static_cast<uint32_t>(out.size());
}

}  // namespace
}  // namespace ifhip

using namespace ifhip;

extern "C" {

int ifhip_round_corners_batch_device(uint8_t* d_bgra, size_t image_bytes, uint32_t n_images, uint32_t w, uint32_t h,
                                     uint32_t stride, int mode, const float* radii, uint32_t matte_bgra, void* hip_stream) {
    if (n_images == 0) return IFHIP_OK;
    if (!radii) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null radii pointer");
    if (mode < IFHIP_ROUND_CORNERS_PERCENTAGE || mode > IFHIP_ROUND_CORNERS_PIXELS_CUSTOM)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: unknown round corners mode %d", mode);
    if (w == 0 || h == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (w > static_cast<uint32_t>(INT32_MAX) || h > static_cast<uint32_t>(INT32_MAX))
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimension overflow");
    int rc = check_frames(d_bgra, image_bytes, w, h, stride, "bitmap");
    if (rc) return rc;
    if ((rc = require_gfx950(nullptr))) return rc;
    Args a{};
    a.bgra = d_bgra; a.image_bytes = image_bytes; a.w = w; a.h = h; a.stride = stride;
    plan(mode, radii, w, h, a.q);
    a.n_rects = cover(a.q, w, h, a.rect);
    if (a.n_rects == 0) return IFHIP_OK;                                                 // radius 0 everywhere: nothing to do
    uint64_t blocks = 0;
    for (uint32_t i = 0; i < a.n_rects; ++i) {
        a.block0[i] = static_cast<uint32_t>(blocks);
        blocks += (static_cast<uint64_t>(a.rect[i][2]) * a.rect[i][3] + kThreads - 1u) / kThreads;
    }
    if (blocks * kThreads > 0xFFFFFFFFull) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: bitmap too large for one launch");
    a.block0[a.n_rects] = static_cast<uint32_t>(blocks);
    const float* s2l = nullptr;
    if ((rc = device_color_tables(&s2l, &a.l2s))) return rc;
    a.s2l = s2l;
    a.matte = matte_bgra;                                                                // :196-205
    a.ma = static_cast<float>(matte_bgra >> 24) * (1.0f / 255.0f);
    const ColorTables& t = color_tables();
    a.mb = t.s2l[matte_bgra & 255u]; a.mg = t.s2l[(matte_bgra >> 8) & 255u]; a.mr = t.s2l[(matte_bgra >> 16) & 255u];
    const hipStream_t st = static_cast<hipStream_t>(hip_stream);
    for (uint32_t i0 = 0; i0 < n_images; i0 += 65535u) {                                 // grid.y is 16-bit
        a.bgra = d_bgra + static_cast<size_t>(i0) * image_bytes;
        hipLaunchKernelGGL(round_corners_kernel, dim3(static_cast<uint32_t>(blocks), std::min(65535u, n_images - i0)), dim3(kThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return IFHIP_OK;
}

int ifhip_round_corners(uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, int mode, const float* radii, uint32_t matte_bgra) {
    if (!radii) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null radii pointer");
    HostFrame s;
    int rc = s.up(bgra, w, h, stride);
    if (rc) return rc;
    if ((rc = ifhip_round_corners_batch_device(s.d, s.image_bytes, 1, w, h, stride, mode, radii, matte_bgra, nullptr))) return rc;
    return s.down(bgra);
}

}  // extern "C"
