"""CPU restatement of graphics/rounded_corners.rs (:5-346) and flow/nodes/round_corners.rs, line for line in float32, for
the tests of csrc/round_corners.hip.  Test infrastructure only: the library has no CPU path.

Rust semantics kept: `f32::clamp` lets NaN through, `f32::max` / `min` return the other operand for NaN, `ceil` / `floor`
then `as usize` saturate (negative and NaN give 0), linear_to_srgb_lut(NaN) reads index 0 (lut.rs:4-8), the alpha is
uchar_clamp_ff (color.rs:101-108) and a fill writes the matte's raw bytes (bitmaps.rs:1504-1548).
"""
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S2L = np.fromfile(os.path.join(GOLDEN, "srgb_to_linear_f32.bin"), np.float32)        # ColorContext(LinearRGB).byte_to_float
L2S = np.fromfile(os.path.join(GOLDEN, "linear_to_srgb_lut.bin"), np.uint8)          # LINEAR_TO_SRGB_LUT

MODES = ("percentage", "pixels", "circle", "percentage_custom", "pixels_custom")     # RoundCornersMode (imageflow_types lib.rs:1254-1268)


def _clamp(v, lo, hi):                       # f32::clamp: NaN stays NaN
    v = f32(v)
    return lo if v < lo else hi if v > hi else v


def _usize(v):                               # `f32 as usize`: saturating, NaN -> 0
    v = float(v)
    return 0 if v != v or v <= 0 else (1 << 64) - 1 if v >= 2.0 ** 64 else int(v)


def _fmax(a, b):                             # f32::max / f32::min: a NaN operand yields the other
    return b if a != a else a if b != b else max(a, b)


def _fmin(a, b):
    return b if a != a else a if b != b else min(a, b)


def get_radius(mode, radii, w, h):
    """:5-32 -> ("all", r) | ("circle",) | ("custom", [tl, tr, bl, br]); radii in JSON order tl, tr, br, bl."""
    sd = f32(min(w, h))
    tl, tr, br, bl = (f32(r) for r in radii)
    pct = lambda p: sd * _clamp(p, f32(0), f32(100)) / f32(200)                      # noqa: E731
    px = lambda p: _clamp(p, f32(0), sd / f32(2))                                     # noqa: E731
    if mode == "percentage":
        return ("all", pct(tl))
    if mode == "pixels":
        return ("all", px(tl))
    if mode == "circle":
        return ("circle",)
    if mode == "percentage_custom":
        return ("custom", [pct(tl), pct(tr), pct(bl), pct(br)])                       # :16-21: bl before br
    if mode == "pixels_custom":
        return ("custom", [px(tl), px(tr), px(bl), px(br)])
    raise ValueError(mode)


def plan_quadrants(radius, w, h):
    """:40-137 -> four dicts in the order TopLeft, TopRight, BottomLeft, BottomRight."""
    if radius[0] == "circle":
        sd = f32(min(w, h))
        ox, oy = max(w - h, 0) // 2, max(h - w, 0) // 2
        qs = plan_quadrants(("all", sd / f32(2)), min(w, h), min(w, h))
        for q in qs:
            q["x"] += ox
            q["y"] += oy
            q["cx"] = f32(q["cx"] + f32(ox))
            q["cy"] = f32(q["cy"] + f32(oy))
        return qs
    if radius[0] == "all":
        v = radius[1]
        return plan_quadrants(("custom", [v, v, v, v]), w, h)
    tl, tr, bl, br = radius[1]
    rw, bh = w // 2, h // 2
    lw, th = w - rw, h - bh
    W, H = f32(w), f32(h)
    return [dict(top=True, left=True, x=0, y=0, w=lw, h=th, r=tl, cx=tl, cy=tl),
            dict(top=True, left=False, x=lw, y=0, w=rw, h=th, r=tr, cx=W - tr, cy=tr),
            dict(top=False, left=True, x=0, y=th, w=lw, h=bh, r=bl, cx=bl, cy=H - bl),
            dict(top=False, left=False, x=lw, y=th, w=rw, h=bh, r=br, cx=W - br, cy=H - br)]


def _l2s(v):
    s = f32(v) * f32(16383)
    return int(L2S[0 if s != s else int(min(max(s, f32(0)), f32(16383)))])


def uchar_clamp_ff(v):
    r = int(np.int16(np.float64(v) + 0.5)) & 0xFFFF if np.isfinite(v) and abs(float(v)) < 32767 else None
    if r is None:                            # `as i16` saturates; NaN -> 0
        r = 0 if v != v else (32767 if v > 0 else (-32768) & 0xFFFF)
    if r > 255:
        r = 0 if v < 0 else 255
    return r


def clear_around_rounded_corners(img, mode, radii, matte):
    """flow_bitmap_bgra_clear_around_rounded_corners (:187-346) in place.  img: uint8 [h][w][4] BGRA; matte: Color32
    0xAARRGGBB."""
    h, w, _ = img.shape
    mbytes = np.array([matte & 255, (matte >> 8) & 255, (matte >> 16) & 255, matte >> 24], np.uint8)
    a2f = f32(1.0) / f32(255.0)
    m_a = f32(matte >> 24) * a2f
    m_b, m_g, m_r = S2L[matte & 255], S2L[(matte >> 8) & 255], S2L[(matte >> 16) & 255]
    vo = f32(0.56419)
    for i, q in enumerate(plan_quadrants(get_radius(mode, radii, w, h), w, h)):
        bottom, right = q["y"] + q["h"], q["x"] + q["w"]
        if q["y"] > 0 and i == 0:
            img[0:q["y"], :] = mbytes                                                 # :218-221
        if h > bottom and i == 2:
            img[bottom:h, :] = mbytes                                                 # :222-225
        rc = _usize(np.ceil(q["r"]))
        M = (1 << 64) - 1
        start_y = q["y"] if q["top"] else (bottom - rc) & M                           # usize arithmetic
        end_y = q["y"] + rc if q["top"] else bottom
        start_x = q["x"] if q["left"] else (right - rc) & M                           # noqa: F841 (unused, as :237-246)
        cf, ct = (0, q["x"]) if q["left"] else (right, w)
        if cf != ct:                                                                  # :252-257
            for y in list(range(q["y"], start_y & 0xFFFFFFFF)) + list(range(end_y & 0xFFFFFFFF, bottom)):
                img[y, cf:ct] = mbytes
        roi = q["r"] + (f32(1) - vo)
        ros = q["r"] - vo
        raw = roi - ros
        roi2, ros2 = roi * roi, ros * ros
        cx, cy = q["cx"], q["cy"]
        for y in range(start_y, end_y):
            yd = abs(cy - (f32(y) + f32(0.5)))
            yd2 = yd * yd
            xs = np.sqrt(_fmax(ros2 - yd2, f32(0)))
            xi = np.sqrt(_fmax(roi2 - yd2, f32(0)))
            es1 = _usize(_fmax(np.ceil(cx - xs), f32(0)))
            es2 = _usize(_fmin(np.floor(cx + xs), f32(w)))
            ei1 = _usize(_fmax(np.floor(cx - xi), f32(0)))
            ei2 = _usize(_fmin(np.ceil(cx + xi), f32(w)))
            if q["left"]:
                img[y, 0:ei1] = mbytes
                af, at = ei1, es1
            else:
                img[y, ei2:w] = mbytes
                af, at = es2, ei2
            for x in range(af, at):
                dx = cx - (f32(x) + f32(0.5))
                d = np.sqrt(dx * dx + yd2)
                if d > roi:
                    img[y, x] = mbytes
                elif d > ros:
                    inten = (d - ros) / raw
                    b, g, r, a = (int(c) for c in img[y, x])
                    pa = f32(a) * a2f * (f32(1) - inten)
                    ma = (f32(1) - pa) * m_a
                    fa = ma + pa
                    with np.errstate(invalid="ignore", divide="ignore"):
                        img[y, x] = [_l2s((S2L[b] * pa + m_b * ma) / fa), _l2s((S2L[g] * pa + m_g * ma) / fa),
                                     _l2s((S2L[r] * pa + m_r * ma) / fa), uchar_clamp_ff(f32(255) * fa)]
    return img


def round_image_corners(img, alpha_meaningful, mode, radii, matte):
    """RoundImageCorners::expand (round_corners.rs:22-53) + the mutate node (:66-93): EnableTransparency first when the
    colour is not opaque (an unused alpha becomes 255), then the clear.  Returns the new alpha_meaningful."""
    if (matte >> 24) != 255 and not alpha_meaningful:
        img[..., 3] = 255
        alpha_meaningful = True
    clear_around_rounded_corners(img, mode, radii, matte)
    return alpha_meaningful
