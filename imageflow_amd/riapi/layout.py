"""Ir4Layout (imageflow_riapi/src/ir4/layout.rs) over sizing.rs: get_precrop, get_initial_copy_window, get_wh_from_all,
get_ideal_target_size, build_constraints as step lists run by execute_all, get_crop_and_layout, align.  AspectRatio's own
arithmetic (proportional, box_of) is the restatement tools/fuzz_shim_chains.py already holds for process_constraint."""
import importlib.util
import math
import os

import numpy as np

from .parse import NotModelled

_spec = importlib.util.spec_from_file_location(
    "_ifhip_fuzz_shim_chains", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools", "fuzz_shim_chains.py"))
_F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_F)
LayoutError = _F.LayoutError
I32_MAX = 2 ** 31 - 1


def _ar(w, h):
    if w > I32_MAX or h > I32_MAX:
        raise NotModelled("a side beyond i32")
    return _F._create(w, h)


def _as_i32(v):                                        # `f64 as i32`: NaN is 0, the rest saturates
    return 0 if math.isnan(v) else int(max(-2.0 ** 31, min(v, float(I32_MAX))))


def _round(v):                                         # f64::round
    return v if math.isnan(v) or math.isinf(v) else _F._rround(v)


def _scaled(v, snaps):                                 # proportional (sizing.rs:118-181): a side that ROUNDS to i32::MAX or beyond is
    if v >= I32_MAX and v not in snaps:                # Err; one that snaps to a side it was given is that side
        raise LayoutError("ValueScalingFailed")
    return v


def _box_of(a, target, inner):
    return tuple(_scaled(v, tuple(a) + tuple(target)) for v in _F._box_of(a, target, inner))


def _other_side(source, basis, basis_is_width):        # AspectRatio::height_for / width_for without a rounding target
    return _scaled(_F._proportional(source[0], source[1], basis, basis_is_width), source)


class Layout:                                           # sizing::Layout (:272-468)
    def __init__(self, original, target):
        self.source = self.canvas = self.image = original
        self.target = target

    def _distort_with(self, s, old, new):               # mult_fraction truncates, in i64
        return _ar(s[0] * new[0] // old[0], s[1] * new[1] // old[1])

    def cmp(self):
        return tuple((c > t) - (c < t) for c, t in zip(self.canvas, self.target))

    def scale_canvas(self, inner):
        nc = _box_of(self.canvas, self.target, inner)
        self.image, self.canvas = self._distort_with(self.image, self.canvas, nc), nc

    def distort_canvas(self, t):
        self.image, self.canvas = self._distort_with(self.image, self.canvas, t), t

    def virtual_canvas(self, t):
        ni = _ar(min(self.image[0], t[0]), min(self.image[1], t[1]))
        self.source, self.image, self.canvas = _box_of(ni, self.source, True), ni, t

    def pad_canvas(self, t):
        if self.canvas[0] > t[0] or self.canvas[1] > t[1]:
            raise LayoutError("ImpossiblePad")
        self.canvas = t

    def crop(self, t):
        if t[0] > self.canvas[0] or t[1] > self.canvas[1]:
            raise LayoutError("ImpossibleCrop")
        self.virtual_canvas(t)

    def step(self, s):
        if s == "scale_to_outer":
            self.scale_canvas(False)
        elif s == "scale_to_inner":
            self.scale_canvas(True)
        elif s == "pad":
            self.pad_canvas(self.target)
        elif s == "crop":
            self.crop(self.target)
        elif s == "crop_intersection":
            self.crop(_ar(min(self.image[0], self.target[0]), min(self.image[1], self.target[1])))
        elif s == "crop_aspect":
            self.crop(_box_of(self.target, self.canvas, True))
        elif s == "distort_target":
            self.distort_canvas(self.target)
        elif s == "virtual_canvas_target":
            self.virtual_canvas(self.target)
        elif s == "virtual_canvas_inner_of_target":     # BoxOf {target: Target, ratio_source: CurrentCanvas, kind: Inner}
            self.virtual_canvas(_box_of(self.canvas, self.target, True))
        else:
            raise AssertionError(s)

    def execute_all(self, steps):                       # sizing.rs:436-463
        skipping = False
        for s in steps:
            if isinstance(s, tuple):
                kind, cond = s
                met = {"either_greater": 1 in self.cmp(), "neither_greater": 1 not in self.cmp(), "either_less": -1 in self.cmp(),
                       "larger1d_smaller1d": self.cmp() in ((1, -1), (-1, 1))}[cond]
                if (kind == "skip_if" and met) or (kind == "skip_unless" and not met):
                    skipping = True
            elif s == "new_seq":
                skipping = False
            elif not skipping:
                self.step(s)
        return self


def build_constraints(i):                               # ir4/layout.rs:160-283
    mode = "max" if "w" not in i and "h" not in i else i.get("mode", "pad")
    scale = i.get("scale", "down")
    down, up = ("skip_unless", "either_greater"), ("skip_unless", "neither_greater")
    table = {
        ("max", "down"): [down, "scale_to_inner"],
        ("max", "up"): [up, "scale_to_inner"],
        ("max", "both"): ["scale_to_inner"],
        ("max", "canvas"): [down, "scale_to_inner", "new_seq", "virtual_canvas_inner_of_target"],
        ("pad", "down"): [down, "scale_to_inner", "pad"],
        ("pad", "up"): [up, "scale_to_inner", "pad"],
        ("pad", "both"): ["scale_to_inner", "pad"],
        ("pad", "canvas"): [down, "scale_to_inner", "new_seq", "pad"],
        ("stretch", "down"): [down, "distort_target"],
        ("stretch", "up"): [up, "distort_target"],
        ("stretch", "both"): ["distort_target"],
        ("stretch", "canvas"): [down, "distort_target", "new_seq", "pad"],
        ("crop", "down"): [("skip_if", "either_less"), "scale_to_outer", "crop", "new_seq", ("skip_unless", "larger1d_smaller1d"), "crop_intersection"],
        ("crop", "up"): [up, "scale_to_outer", "crop"],
        ("crop", "both"): ["scale_to_outer", "crop"],
        ("crop", "canvas"): [("skip_if", "either_less"), "scale_to_outer", "crop", "new_seq", ("skip_unless", "larger1d_smaller1d"), "virtual_canvas_target"],
    }
    return ["crop_aspect"] if mode == "aspectcrop" else table[(mode, scale)]


def wh_from_all(i, source):                             # :63-91
    w, h = max(i.get("w", -1), -1), max(i.get("h", -1), -1)
    mw, mh = max(i.get("legacy_max_width", -1), -1), max(i.get("legacy_max_height", -1), -1)
    if mw > 0 and w > 0:
        w, mw = min(mw, w), -1
    if mh > 0 and h > 0:
        h, mh = min(mh, h), -1
    if w != -1 and mh != -1:
        mh = min(mh, _other_side(source, w, True))
    if h != -1 and mw != -1:
        mw = min(mw, _other_side(source, h, False))
    w, h = max(w, mw), max(h, mh)
    return (None if w < 1 else w), (None if h < 1 else h)


def ideal_target_size(i, source, preshrink_ratio):      # :93-131
    unshrunk = (_as_i32(source[0] / preshrink_ratio), _as_i32(source[1] / preshrink_ratio))
    w, h = wh_from_all(i, source)
    if w is None and h is None:
        w, h = unshrunk
    elif h is None:
        h = _other_side(source, w, True)
    elif w is None:
        w = _other_side(source, h, False)
    zoom = max(0.00008, min(float(i["zoom"]) if "zoom" in i else 1.0, 80000.0))
    return _ar(*(_as_i32(max(1.0, min(_round(v * zoom), float(I32_MAX)))) for v in (w, h)))


def initial_copy_window(i, w, h, ref_w, ref_h):         # :700-775
    fl = [0.0, 0.0, float(ref_w), float(ref_h)]
    if "crop" in i:
        units = [i.get("cropxunits") or float(ref_w), i.get("cropyunits") or float(ref_h)]
        vals = []
        for ix, item in enumerate(i["crop"]):
            top = float((ref_w, ref_h)[ix % 2])
            v = item * top / units[ix % 2]
            if (ix < 2 and v < 0) or (ix > 1 and v <= 0):
                v += top
            if v < 0:
                v = 0.0
            if v > top:
                v = top
            vals.append(v)
        if not (_round(vals[3]) <= _round(vals[1]) or _round(vals[2]) <= _round(vals[0])):
            fl = vals
    if (ref_w, ref_h) != (w, h):
        fl = [fl[0] * w / ref_w, fl[1] * h / ref_h, fl[2] * w / ref_w, fl[3] * h / ref_h]
    ints = [max(0, min(_as_i32(_round(v)), (w, h)[ix % 2])) for ix, v in enumerate(fl)]
    return [0, 0, w, h] if ints[3] <= ints[1] or ints[2] <= ints[0] else ints


def align1d(a, inner, outer):                           # :649-660
    kind, pct = a
    if (outer < inner and inner < 1) or outer < 1:
        raise NotModelled("align: .expect() panics")
    if kind == "near":
        return 0
    if kind == "center":
        return int((outer - inner) / 2)                 # i32 division truncates toward zero
    if kind == "far":
        return outer - inner
    return gravity1d(pct, inner, outer)


def gravity1d(pct, inner, outer):                       # :673-683, in f32
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        p = f32(pct)
        ratio = (p if np.isnan(p) else min(max(p, f32(0)), f32(100))) / f32(100)
        v = f32(outer - inner) * ratio
    return max(0, min(_as_i32(_round(float(v))), outer - inner))


def crop_and_layout(i, w, h, ref_w, ref_h):
    """-> (crop [x1, y1, x2, y2] or None, Layout); :414-470"""
    swap = (int(i.get("srotate", 0) / 90) + 4) % 2 != 0
    pw, ph, rw, rh = (h, w, ref_h, ref_w) if swap else (w, h, ref_w, ref_h)
    win = initial_copy_window(i, pw, ph, rw, rh)
    initial = _ar(win[2] - win[0], win[3] - win[1])
    target = ideal_target_size(i, initial, w / ref_w)
    lay = Layout(initial, target).execute_all(build_constraints(i))
    center = ("center", None)
    if "c_gravity" in i:
        with np.errstate(over="ignore"):
            ax, ay = (("percent", np.float32(v)) for v in i["c_gravity"])
    else:
        ax, ay = i.get("anchor", (center, center))
    x1, y1 = win[0] + align1d(ax, lay.source[0], initial[0]), win[1] + align1d(ay, lay.source[1], initial[1])
    crop = [x1, y1, x1 + lay.source[0], y1 + lay.source[1]] if x1 > 0 or y1 > 0 or (pw, ph) != tuple(lay.source) else None
    return crop, lay
