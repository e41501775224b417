"""CPU restatement of the reference's whitespace detector, imageflow_core/src/graphics/whitespace.rs (line numbers below are
that file's), plus CropWhitespace's padding (flow/nodes/clone_crop_fill_expand.rs:564-627).  Vectorised per window with
numpy, so a 4K frame takes seconds; every scalar step keeps the reference's types: u32 wrap-around, f32 products and
floors, the i64 area test.  Test infrastructure only -- the library computes this on the device (csrc/whitespace.hip).

`trace` (optional list) receives ("branch", "full"|"inward") and ("window", x, y, w, h) events."""
import numpy as np

M32 = 0xFFFFFFFF
TOP, RIGHT, BOTTOM, LEFT, NONDIR = range(5)
F = np.float32

# :30-123 SCAN_QUICK_REGIONS (edge, x1%, y1%, x2%, y2%)
QUICK = [(LEFT, 0, .5, .5, .5), (RIGHT, .5, .5, 1, .5), (LEFT, 0, .677, .5, .677), (RIGHT, .5, .677, 1, .677),
         (LEFT, 0, .333, .5, .333), (RIGHT, .5, .333, 1, .333), (TOP, .5, 0, .5, .5), (TOP, .677, 0, .677, .5),
         (TOP, .333, 0, .333, .5), (BOTTOM, .5, .5, .5, 1), (BOTTOM, .677, .5, .677, 1), (BOTTOM, .333, .5, .333, 1)]
INWARD = [(TOP, 0, 0, 1, 1), (RIGHT, 0, 0, 1, 1), (BOTTOM, 0, 0, 1, 1), (LEFT, 0, 0, 1, 1)]      # :125-154
FULL = (NONDIR, 0, 0, 1, 1)                                                                   # :155-161
BUF_SIZE = 2048                                                                                # :187-193


def approximate_grayscale(frame, alpha_meaningful):
    """:437-529 for one BGRA frame [h][w][4]: Bgra32 (alpha meaningful) or Bgr32."""
    b, g, r = (frame[..., i].astype(np.uint32) for i in range(3))
    s = 233 * b + 1197 * g + 610 * r
    if alpha_meaningful:                                                                       # :477-490
        gray = (s * frame[..., 3].astype(np.uint32) + 524287) // 524288                        # div_ceil
        return np.minimum(gray, 255).astype(np.uint8)
    return (s // 2048).astype(np.uint8)                                                        # :506-519


def _f2u32(v):
    """`f32 as u32` (saturating, NaN -> 0)"""
    v = float(v)
    return 0 if v != v or v <= 0 else M32 if v >= 4294967295.0 else int(v)


class Search:                                                                                  # :203-211
    def __init__(self, w, h, threshold):
        self.w, self.h, self.threshold = w, h, threshold & M32
        self.min_x, self.max_x, self.min_y, self.max_y = w, 0, h, 0

    def get_search_rect(self, region):                                                         # :214-282
        edge, px1, py1, px2, py2 = region
        fl = lambda p, side: _f2u32(np.floor(F(p) * F((side - 1) & M32)))                     # noqa: E731
        x1 = max(0, min(self.w, fl(px1, self.w)))
        x2 = max(0, min(self.w, fl(px2, self.w)))
        y1 = max(0, min(self.h, fl(py1, self.h)))
        y2 = max(0, min(self.h, fl(py2, self.h)))
        if edge == LEFT:                                                                       # :234-255
            x1, x2 = 0, min(x2, self.min_x)
        elif edge == RIGHT:
            x1, x2 = max(x1, self.max_x), self.w
        elif edge == TOP:
            y1, y2 = 0, min(y2, self.min_y)
        elif edge == BOTTOM:
            y1, y2 = max(y1, self.max_y), self.h
        if x1 == x2 or y1 == y2:                                                               # :257-259
            return None
        mrw = 3 if edge in (RIGHT, LEFT) else 7                                                # :262-265
        mrh = 3 if edge in (TOP, BOTTOM) else 7
        while ((y2 - y1) & M32) < mrh and (y1 > 0 or y2 < self.h):                             # :267-274
            y1 = y1 - 1 if y1 > 0 else 0
            y2 = min(self.h, y2 + 1)
        while ((x2 - x1) & M32) < mrw and (x1 > 0 or x2 < self.w):
            x1 = x1 - 1 if x1 > 0 else 0
            x2 = min(self.w, x2 + 1)
        return x1, y1, x2, y2


def _window_box(g, bx, by, bw, bh, thr):
    """:531-634 sobel_scharr_detect over one window of the grey frame: the box of its hits in frame coordinates, or None"""
    G = g[by:by + bh, bx:bx + bw].astype(np.int32)
    a11, a12, a13 = G[:-2, :-2], G[:-2, 1:-1], G[:-2, 2:]
    a21, a22, a23 = G[1:-1, :-2], G[1:-1, 1:-1], G[1:-1, 2:]
    a31, a32, a33 = G[2:, :-2], G[2:, 1:-1], G[2:, 2:]
    gx = 3 * a11 + 10 * a21 + 3 * a31 - 3 * a13 - 10 * a23 - 3 * a33                          # :556-568
    gy = 3 * a11 + 10 * a12 + 3 * a13 - 3 * a31 - 10 * a32 - 3 * a33
    hit = (np.abs(gx) + np.abs(gy)) > thr                                                      # :570-572
    if not hit.any():
        return None
    rows = ((a11, a12, a13), (a21, a22, a23), (a31, a32, a33))
    sh = hit.shape
    mnx, mxx = np.full(sh, 2), np.full(sh, 1)                                                  # :576-579
    mny, mxy = np.full(sh, 2), np.full(sh, 1)
    for my in range(3):                                                                        # :582-599
        e1 = np.abs(rows[my][0] - rows[my][1]) > thr
        e2 = np.abs(rows[my][1] - rows[my][2]) > thr
        mnx = np.where(e1, np.minimum(mnx, 1), mnx)
        mxx = np.where(e1, np.maximum(mxx, 1), mxx)
        mnx = np.where(e2, np.minimum(mnx, 2), mnx)
        mxx = np.where(e2, np.maximum(mxx, 2), mxx)
        mny = np.where(e1 | e2, np.minimum(mny, my), mny)
        mxy = np.where(e1 | e2, np.maximum(mxy, my + 1), mxy)
    for mx in range(3):                                                                        # :600-615
        e1 = np.abs(rows[0][mx] - rows[1][mx]) > thr
        e2 = np.abs(rows[1][mx] - rows[2][mx]) > thr
        mny = np.where(e1, np.minimum(mny, 1), mny)
        mxy = np.where(e1, np.maximum(mxy, 1), mxy)
        mny = np.where(e2, np.minimum(mny, 2), mny)
        mxy = np.where(e2, np.maximum(mxy, 2), mxy)
        mnx = np.where(e1 | e2, np.minimum(mnx, mx), mnx)
        mxx = np.where(e1 | e2, np.maximum(mxx, mx + 1), mxx)
    yy, xx = np.nonzero(hit)                                                                   # centre = window + index + 1
    cx, cy = bx + xx + 1, by + yy + 1
    return (int((mnx[yy, xx] + cx - 1).min()), int((mny[yy, xx] + cy - 1).min()),              # :617-633
            int((mxx[yy, xx] + cx - 1).max()), int((mxy[yy, xx] + cy - 1).max()))


def check_region(s, g, region, trace=None):                                                    # :336-434
    r = s.get_search_rect(region)
    if r is None:
        return
    x1, y1, x2, y2 = r
    w, h = (x2 - x1) & M32, (y2 - y1) & M32
    ww = min(w, BUF_SIZE // 7 if region[0] == NONDIR else int(np.ceil(np.sqrt(F(BUF_SIZE)))))  # :352-359
    wh = min(h, BUF_SIZE // ww)
    vwin = _f2u32(np.ceil(F(h) / F((wh - 2) & M32)))                                           # :361-362
    hwin = _f2u32(np.ceil(F(w) / F((ww - 2) & M32)))
    thr = s.threshold - (1 << 32) if s.threshold >= 1 << 31 else s.threshold                   # `threshold as i32`
    for row in range(vwin):                                                                    # :364-365
        for col in range(hwin):
            bx = (x1 + (ww - 2) * col) & M32                                                   # :369-374
            by = (y1 + (wh - 2) * row) & M32
            bw = min(max(3, (x2 - bx) & M32), ww)
            bh = min(max(3, (y2 - by) & M32), wh)
            bx2, by2 = (bx + bw) & M32, (by + bh) & M32
            ex_x = s.min_x < bx and s.max_x > bx2                                              # :376-381
            ex_y = s.min_y < by and s.max_y > by2
            if ex_x and ex_y:
                continue
            if ex_y and s.min_x < bx2 < s.max_x:                                               # :383-388
                bw = max(3, (s.min_x - bx) & M32)
            elif ex_y and s.max_x > bx > s.min_x:
                bx = min((bx2 - 3) & M32, s.max_x)
                bw = (bx2 - bx) & M32
            if ex_x and s.min_y < by2 < s.max_y:                                               # :389-394
                bh = max(3, (s.min_y - by) & M32)
            elif ex_x and s.max_y > by > s.min_y:
                by = min((by2 - 3) & M32, s.max_y)
                bh = (by2 - by) & M32
            if ((by + bh) & M32) > s.h:                                                        # :396-415
                if bh <= s.h:
                    by = (s.h - bh) & M32
                else:
                    by, bh = 0, s.h
            if ((bx + bw) & M32) > s.w:
                if bw <= s.w:
                    bx = (s.w - bw) & M32
                else:
                    bx, bw = 0, s.w
            if trace is not None:
                trace.append(("window", bx, by, bw, bh))
            box = _window_box(g, bx, by, bw, bh, thr)                                          # :417-419
            if box is not None:
                s.min_x, s.min_y = min(s.min_x, box[0]), min(s.min_y, box[1])
                s.max_x, s.max_y = max(s.max_x, box[2]), max(s.max_y, box[3])


def detect_content_gray(g, threshold, trace=None):
    """:284-334 on a grey frame [h][w] -> (x1, y1, x2, y2)"""
    h, w = g.shape
    if w < 3 or h < 3:                                                                         # :288-290
        return 0, 0, w, h
    s = Search(w, h, threshold)
    for region in QUICK:                                                                       # :304-306
        check_region(s, g, region, trace)
    area = (s.min_x * s.h + s.min_y * s.w + (s.w - s.max_x) * s.h + (s.h - s.max_y) * s.w)    # :309-312 (i64)
    if area > s.h * s.w:                                                                       # :314-316
        if trace is not None:
            trace.append(("branch", "full"))
        check_region(s, g, FULL, trace)
    else:
        if trace is not None:
            trace.append(("branch", "inward"))
        for region in INWARD:                                                                  # :318-323
            check_region(s, g, region, trace)
    if s.min_x == w and s.max_x == 0 and s.min_y == h and s.max_y == 0:                        # :326-333
        return 0, 0, w, h
    return s.min_x, s.min_y, s.max_x, s.max_y


def detect_content(frame, alpha_meaningful, threshold, trace=None):
    """detect_content on a BGRA frame [h][w][4]"""
    return detect_content_gray(approximate_grayscale(frame, alpha_meaningful), threshold, trace)


def full_frame_box(frame, alpha_meaningful, threshold):
    """What a one-pass reduction over every interior pixel would give (NOT the reference's answer)"""
    g = approximate_grayscale(frame, alpha_meaningful)
    h, w = g.shape
    if w < 3 or h < 3:
        return 0, 0, w, h
    thr = threshold - (1 << 32) if threshold >= 1 << 31 else threshold
    box = _window_box(g, 0, 0, w, h, thr)
    return (0, 0, w, h) if box is None else box


def padded_rect(rect, w, h, percent_padding):
    """CropWhitespaceDef::expand (clone_crop_fill_expand.rs:585-603): the detected rectangle grown by the padding, clamped
    to the frame; ValueError for the reference's 'invalid rectangle' error"""
    x1, y1, x2, y2 = rect
    if x2 <= x1 or y2 <= y1:
        raise ValueError("Whitespace detection returned invalid rectangle")
    p = float(np.ceil(F(percent_padding) / F(100) * F(x2 - x1 + y2 - y1) / F(2)))             # f32, then `.ceil() as i64`
    pad = 0 if p != p else int(max(min(p, 2.0 ** 63 - 1), -2.0 ** 63))
    return max(0, x1 - pad), max(0, y1 - pad), min(w, x2 + pad), min(h, y2 + pad)


def crop_whitespace_rect(frame, alpha_meaningful, threshold, percent_padding):
    h, w = frame.shape[:2]
    return padded_rect(detect_content(frame, alpha_meaningful, threshold), w, h, percent_padding)
