"""Ir4Layout::add_steps (imageflow_riapi/src/ir4/layout.rs:473-647) and Ir4Expand::get_decode_commands (ir4/mod.rs:155-210):
Instructions + the frame they meet -> decoder commands and nodes, in the JSON form v1/execute takes."""
import math

import numpy as np

from .layout import NotModelled, align1d, crop_and_layout
from .parse import parse


def _f(v):
    v = float(v)
    return v if math.isfinite(v) else None


def _rotate(steps, r):
    if r is not None:
        name = {1: "rotate_90", 2: "rotate_180", 3: "rotate_270"}.get((int(r / 90) + 4) % 4)
        if name:
            steps.append(name)


def _flip(steps, f):
    if f:
        steps.extend(n for n, on in zip(("flip_h", "flip_v"), f) if on)


def expand(i, w, h, ref_w, ref_h, watermarks=None):
    """-> {"decoder_commands": [...], "steps": [...], "canvas": [w, h]} for a w x h frame of a ref_w x ref_h image"""
    crop, lay = crop_and_layout(i, w, h, ref_w, ref_h)
    source, image, canvas = lay.source, lay.image, lay.canvas
    # decoder commands: the pre-shrink ratio of the cropped window against the image box -- `to.w` under both sides, as written there
    commands = []
    ratio = i.get("min_precise_scaling_ratio")
    preshrink = (2.1 if ratio is None else float(ratio)) / min(source[0] / image[0], source[1] / image[0])
    gamma_correct = i.get("down_colorspace") != "srgb"
    if i.get("ignoreicc"):
        commands.append("discard_color_profile")
    if preshrink < 1:
        hw, hh = math.floor(w * preshrink), math.floor(h * preshrink)
        commands.append({"jpeg_downscale_hints": {"width": hw, "height": hh, "scale_luma_spatially": gamma_correct,
                                                  "gamma_correct_for_srgb_during_spatial_luma_scaling": gamma_correct}})
        if not gamma_correct:
            commands.append({"webp_decoder_hints": {"width": hw, "height": hh}})
    steps = []
    _rotate(steps, i.get("srotate"))
    _flip(steps, i.get("sflip"))
    if crop:
        steps.append({"crop": dict(zip(("x1", "y1", "x2", "y2"), crop))})
    white = {"srgb": {"hex": "FFFFFFFF"}}
    if "bgcolor" in i:
        c = i["bgcolor"]
        bg = resample_bg = {"srgb": {"hex": "%08X" % (((c << 8) | (c >> 24)) & 0xFFFFFFFF)}}
    else:                                               # white "if targeting jpeg": format=jpg -- and, for the resample alone, a
        bg = white if i.get("format_jpeg") else "transparent"              # quality that is no number (this library's own rule)
        resample_bg = white if i.get("jpeg_out") else "transparent"
    downscaling = image[0] < source[0] or image[1] < source[1]
    space = i.get("down_colorspace" if downscaling else "up_colorspace")
    hints = {}
    if "f_sharpen" in i:
        hints["sharpen_percent"] = _f(i["f_sharpen"])
    for k in ("down_filter", "up_filter"):
        if k in i:
            hints[k] = i[k]
    if space in ("linear", "srgb"):
        hints["scaling_colorspace"] = space
    hints["background_color"] = resample_bg
    hints["resample_when"] = "size_differs_or_sharpening_requested"
    if "f_sharpen_when" in i:
        hints["sharpen_when"] = i["f_sharpen_when"]
    steps.append({"resample_2d": {"w": image[0], "h": image[1], "hints": hints}})
    if "s_round_corners" in i:
        with np.errstate(over="ignore"):
            q = [np.float32(v) for v in i["s_round_corners"]]
        r64 = i["s_round_corners"]
        if r64[0] == r64[1] == r64[2] == r64[3]:
            radius = {"percentage": _f(q[0])}
        else:
            radius = {"percentage_custom": dict(zip(("top_left", "top_right", "bottom_right", "bottom_left"), map(_f, q)))}
        steps.append({"round_image_corners": {"radius": radius, "background_color": bg}})
    for k in ("alpha", "brightness", "contrast", "saturation"):
        if "s_" + k in i:
            steps.append({"color_filter_srgb": {k: _f(i["s_" + k])}})
    if i.get("s_sepia"):
        steps.append({"color_filter_srgb": "sepia"})
    if "s_grayscale" in i:
        steps.append({"color_filter_srgb": i["s_grayscale"]})
    if i.get("a_balance_white"):
        steps.append({"white_balance_histogram_area_threshold_srgb": {"threshold": None}})

    def of_canvas(mark):
        box = mark.get("fit_box")
        return isinstance(box, dict) and next(iter(box), None) in ("canvas_margins", "canvas_percentage")
    steps.extend({"watermark": m} for m in watermarks or [] if not of_canvas(m))
    center = ("center", None)
    ax, ay = i.get("anchor", (center, center))
    left, top = align1d(ax, image[0], canvas[0]), align1d(ay, image[1], canvas[1])
    right, bottom = canvas[0] - image[0] - left, canvas[1] - image[1] - top
    if max(left, top, right, bottom) > 0:
        if min(left, top, right, bottom) < 0:
            raise NotModelled("negative padding: the reference panics")
        steps.append({"expand_canvas": {"left": left, "top": top, "right": right, "bottom": bottom, "color": bg}})
    steps.extend({"watermark": m} for m in watermarks or [] if of_canvas(m))
    _rotate(steps, i.get("rotate"))
    _flip(steps, i.get("flip"))
    if i.get("watermark_red_dot"):
        steps.append("watermark_red_dot")
    return {"decoder_commands": commands, "steps": steps, "canvas": list(canvas)}


def expand_text(text, w, h, ref_w=None, ref_h=None, watermarks=None):
    return expand(parse(text), w, h, w if ref_w is None else ref_w, h if ref_h is None else ref_h, watermarks)
