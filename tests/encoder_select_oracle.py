"""An independent restatement, in numpy.float32, of the reference's encoder selection for the presets `auto` and `format`
(imageflow_core/src/codecs/auto.rs:368-1242 as built with `c-codecs` and without `zen-codecs`) and of the preset its querystring
layer makes (imageflow_riapi/src/ir4/encoder.rs:5-98), written from the reference's lines for tests/test_encoder_select.py to
compare csrc/encoder_select.cpp with.  It shares no code with the library.

One documented difference is built in: interpolate_value (auto.rs:696-702) panics in the reference when b - a <= 0; here, as in
the library, the expression is evaluated anyway and `State.panicked` records that the reference would not have returned."""
import numpy as np

F = np.float32
FEATURES = {"jxl": False, "avif": False, "webp_animation": False, "jpegli": False}      # auto.rs:1127-1134 without zen-codecs

COLUMNS = ("name", "p", "ssim2", "moz", "jpegli", "webp", "webp_m", "avif", "avif_s", "jxl", "jxl_e", "png", "png_max", "png_s")
ABSOLUTE_LOWEST = dict(zip(COLUMNS, (None, 0.0, 0.0, 0.0, 0.0, 0.0, 5, 0.0, 6, 25.0, 6, 0, 4, 4)))                 # auto.rs:587-602
QUALITY_HINTS = [dict(zip(COLUMNS, row)) for row in (                                                              # auto.rs:604-621
    ("lowest", 15.0, 10.0, 15.0, 15.0, 15.0, 6, 23.0, 6, 13.0, 5, 0, 10, 4),
    ("low", 20.0, 30.0, 20.0, 20.0, 20.0, 6, 34.0, 6, 7.4, 6, 0, 20, 4),
    ("mediumlow", 34.0, 50.0, 34.0, 34.0, 34.0, 6, 45.0, 6, 4.3, 5, 0, 35, 4),
    ("medium", 55.0, 60.0, 57.0, 52.0, 53.0, 5, 44.0, 6, 3.92, 5, 0, 55, 4),
    ("good", 73.0, 70.0, 73.0, 73.0, 76.0, 6, 55.0, 6, 2.58, 5, 50, 100, 4),
    ("high", 91.0, 85.0, 91.0, 91.0, 93.0, 5, 66.0, 6, 1.0, 5, 80, 100, 4),
    ("highest", 96.0, 90.0, 96.0, 96.0, 96.0, 5, 100.0, 6, 0.5, 0, 90, 100, 4),
    ("lossless", 100.0, 100.0, 100.0, 100.0, 100.0, 6, 100.0, 5, 0.0, 6, 100, 100, 4))]
for _row in QUALITY_HINTS + [ABSOLUTE_LOWEST]:
    for _k in ("p", "ssim2", "moz", "jpegli", "webp", "avif", "jxl"):
        _row[_k] = F(_row[_k])


class State:
    panicked = False                    # the reference's interpolate_value would have panicked since the last reset


class NoFormats(Exception):
    """create_encoder_auto's InvalidArgument (auto.rs:376-379)"""


def clamp(v, lo, hi):
    v = F(v)
    return F(lo) if v < F(lo) else F(hi) if v > F(hi) else v


def as_u8(v):
    if v != v:
        return 0
    return int(min(255.0, max(0.0, np.trunc(float(v)))))


def interpolate_value(ratio, a, b):
    a, b = F(a), F(b)
    if F(b - a) <= F(0.0):
        State.panicked = True           # "Invalid interpolation values"
    return F(a + F(ratio * F(b - a)))


def _interpolated(ratio, percent, lower, higher):
    return {"name": None, "p": percent,
            "ssim2": interpolate_value(ratio, lower["ssim2"], higher["ssim2"]),
            "moz": interpolate_value(ratio, lower["moz"], higher["moz"]),
            "jpegli": interpolate_value(ratio, lower["jpegli"], higher["jpegli"]),
            "webp": interpolate_value(ratio, lower["webp"], higher["webp"]),
            "avif": interpolate_value(ratio, lower["avif"], higher["avif"]),
            "jxl": interpolate_value(ratio, higher["jxl"], lower["jxl"]),
            "png": as_u8(clamp(interpolate_value(ratio, F(lower["png"]), F(higher["png"])), 0.0, 100.0)),
            "png_max": as_u8(clamp(interpolate_value(ratio, F(lower["png_max"]), F(higher["png_max"])), 0.0, 100.0)),
            "png_s": higher["png_s"], "jxl_e": higher["jxl_e"], "webp_m": higher["webp_m"], "avif_s": higher["avif_s"]}


def get_quality_hints(qp):                                                                  # auto.rs:725-770
    if isinstance(qp, str):
        return next(q for q in QUALITY_HINTS if q["name"] == qp)
    percent = clamp(qp["percent"], 0.0, 100.0)
    higher = next(q for q in QUALITY_HINTS if q["p"] >= percent)
    if higher["p"] == percent:
        return higher
    lower = next((q for q in reversed(QUALITY_HINTS) if q["p"] < percent), ABSOLUTE_LOWEST)
    assert not (lower["p"] >= higher["p"] or percent < lower["p"] or percent > higher["p"])
    ratio = F(F(percent - lower["p"]) / F(higher["p"] - lower["p"]))
    return _interpolated(ratio, percent, lower, higher)


def get_quality_hints_by_ssim2(ssim2):                                                      # auto.rs:772-803
    percent = clamp(ssim2, 0.0, 100.0)
    higher = next(q for q in QUALITY_HINTS if q["ssim2"] >= percent)
    if higher["ssim2"] == percent:
        return higher
    lower = next((q for q in reversed(QUALITY_HINTS) if q["ssim2"] < percent), ABSOLUTE_LOWEST)
    assert not (lower["ssim2"] >= higher["ssim2"] or percent < lower["ssim2"] or percent > higher["ssim2"])
    ratio = F(F(percent - lower["p"]) / F(higher["p"] - lower["p"]))                          # the reference's quirk: p, not ssim2
    return _interpolated(ratio, percent, lower, higher)


def get_quality_hints_with_dpr(qp, dpr):                                                    # auto.rs:703-724
    hints = get_quality_hints(qp)
    if dpr is None or F(dpr) == F(3.0):
        return hints
    quality_factor = F(F(3.0) / clamp(dpr, 0.1, 12.0))
    target_ssim2 = clamp(F(hints["ssim2"] * quality_factor), 10.0, 90.0)
    return get_quality_hints_by_ssim2(target_ssim2)


def approximate_quality_profile(qp):                                                        # auto.rs:623-628
    return F(90.0) if qp is None else get_quality_hints(qp)["p"]


# ---- AllowedFormats (imageflow_types/src/lib.rs:443-560) --------------------------------------------------------------------
ALLOW_KEYS = ("webp", "jxl", "avif", "jpeg", "jpeg_progressive", "jpeg_xyb", "png", "gif", "all", "web_safe", "modern_web_safe", "color_profiles")


def _allow(**on):
    return {k: on.get(k) for k in ALLOW_KEYS}


def web_safe():
    return _allow(jpeg=True, png=True, gif=True, web_safe=True)


def modern_web_safe():
    a = web_safe()
    a.update(webp=True, modern_web_safe=True, color_profiles=True, jpeg_progressive=True, jpeg_xyb=True)
    return a


def merge(a, b):
    def either(x, y):
        return y if x is None else x if y is None else (x or y)
    return {k: either(a.get(k), b.get(k)) for k in ALLOW_KEYS}


def expand_sets(a):
    a = {k: a.get(k) for k in ALLOW_KEYS}
    if a["all"] is True:
        return {k: True for k in ALLOW_KEYS}
    if a["web_safe"] is True:
        return merge(a, web_safe())
    if a["modern_web_safe"] is True:
        return merge(a, modern_web_safe())
    return a


def any_formats_enabled(a):
    return any(a[k] is True for k in ("webp", "jxl", "avif", "jpeg", "png", "gif"))


# ---- the resolution -----------------------------------------------------------------------------------------------------------
def _opaque(matte):                                          # Color::is_opaque: "black" and an srgb hex without or with FF alpha
    if matte is None or matte == "transparent":
        return False
    if matte == "black":
        return True
    h = matte["srgb"]["hex"].lstrip("#")
    return len(h) in (3, 6) or (len(h) == 4 and h[3] in "fF") or (len(h) == 8 and h[6:].lower() == "ff")


def format_auto_select(d):                                                                  # auto.rs:1136-1242
    allowed = d["allow"]
    if not any_formats_enabled(allowed):
        return None
    if d["needs_animation"]:
        if FEATURES["webp_animation"] and allowed["webp"] is True:
            return "webp"
        return "gif"
    if FEATURES["jxl"] and allowed["jxl"] is True:
        return "jxl"
    if d["needs_lossless"] is True or d["needs_alpha"]:
        if allowed["webp"] is True:
            return "webp"
        if allowed["png"] is True:
            return "png"
        if FEATURES["avif"] and allowed["avif"] is True:
            return "avif"
    can_jpegli = FEATURES["jpegli"] and allowed["jpeg"] is True
    if (d["pixels"] < 3000000 or not can_jpegli) and FEATURES["avif"] and allowed["avif"] is True:
        return "avif"
    if can_jpegli:
        return "jpeg"
    approx = approximate_quality_profile(d["quality_profile"])
    if approx > F(90.0) or allowed["jpeg_progressive"] is not True:
        if allowed["webp"] is True:
            return "webp"
    if allowed["jpeg"] is True:
        return "jpeg"
    if FEATURES["avif"] and allowed["avif"] is True:
        return "avif"
    if allowed["png"] is True:
        return "png"
    if allowed["gif"] is True:
        return "gif"
    return None


def resolve(preset, source, alpha_meaningful, w, h):
    """preset: {"auto": {..}} | {"format": {..}} as JSON; source: None or {"format", "lossless", "animated"}.
    -> {"format", "coder", "params", "matte"}; raises NoFormats.  State.panicked is reset and set."""
    State.panicked = False
    (kind, body), = preset.items()
    fmt = body.get("format") if kind == "format" else None
    qp, dpr, matte = body.get("quality_profile"), body.get("quality_profile_dpr"), body.get("matte")
    lossless, allow = body.get("lossless"), body.get("allow")
    hints = (body.get("encoder_hints") or {}) if kind == "format" else {}
    # build_auto_encoder_details (auto.rs:1042-1111)
    needs_alpha = alpha_meaningful and not _opaque(matte)
    explicit = (source["format"] if source else None) if fmt == "keep" else fmt
    src_lossless = source["lossless"] if source else None
    if lossless == "keep":
        needs_lossless = needs_alpha if src_lossless is None else src_lossless
    else:
        needs_lossless = {"true": True, "false": False, None: None}[lossless]
    if qp == "lossless":
        needs_lossless = True
    d = {"allow": expand_sets(allow) if allow is not None else web_safe(), "needs_animation": bool(source and source["animated"]),
         "needs_alpha": needs_alpha, "needs_lossless": needs_lossless, "pixels": w * h, "quality_profile": qp}
    # create_encoder_auto (auto.rs:368-566)
    final = explicit
    if final is None:
        final = format_auto_select(d)
        if final is None:
            raise NoFormats("No formats enabled; try 'allow': { 'web_safe':true}")
    if final == "jxl" and not FEATURES["jxl"]:
        final = format_auto_select(d) or "jpeg"
    if final == "avif" and not FEATURES["avif"]:
        final = format_auto_select(d) or "jpeg"
    out = {"matte": matte}
    profile = get_quality_hints_with_dpr(qp, dpr) if qp is not None else None
    if final == "gif":
        out.update(format="gif", coder="gif", params={})
    elif final in ("jpeg", "jpg"):                                                           # create_jpeg_auto (:806-874)
        j = hints.get("jpeg") or {}
        progressive = j.get("progressive")
        progressive = True if progressive is None else progressive
        if d["allow"]["jpeg_progressive"] is not True:
            progressive = False
        q = profile["moz"] if profile else F(j["quality"]) if j.get("quality") is not None else F(90.0)
        quality = as_u8(clamp(q, 0.0, 100.0))
        if j.get("mimic") == "libjpegturbo":
            out.update(format="jpeg", coder="libjpeg_turbo",
                       params={"quality": quality, "progressive": progressive, "optimize_huffman_coding": progressive, "matte": matte})
        else:
            out.update(format="jpeg", coder="mozjpeg", params={"quality": quality, "progressive": progressive, "matte": matte})
    elif final == "webp":                                                                    # create_webp_auto (:876-912)
        wh = hints.get("webp") or {}
        manual_lossless = {"keep": bool(src_lossless), "true": True, "false": False, None: None}[wh.get("lossless")]
        manual_quality = clamp(wh["quality"] if wh.get("quality") is not None else 80.0, 0.0, 100.0)
        is_lossless = needs_lossless if needs_lossless is not None else manual_lossless if manual_lossless is not None else False
        if is_lossless:
            out.update(format="webp", coder="webp_lossless", params={})
        else:
            out.update(format="webp", coder="webp_lossy", params={"quality": float(profile["webp"] if profile else manual_quality)})
    else:                                                                                    # create_png_auto (:914-1025)
        assert final == "png", final
        ph = hints.get("png") or {}
        manual_quality, style, manual_lossless = ph.get("quality"), ph.get("mimic") or "default", ph.get("lossless")
        if needs_lossless is True:
            is_lossless = True
        elif manual_lossless == "keep":
            is_lossless = bool(src_lossless)
        elif manual_lossless is not None:
            is_lossless = manual_lossless == "true"
        elif needs_lossless is False:
            is_lossless = False
        else:
            is_lossless = manual_quality is None or style == "libpng"
        max_deflate = ph.get("hint_max_deflate")
        if profile is not None:
            if profile["png"] == 100 or is_lossless:
                out.update(format="png", coder="lodepng", params={"maximum_deflate": max_deflate})
            else:
                out.update(format="png", coder="pngquant", params={"quality": profile["png_max"], "minimum_quality": profile["png"],
                                                                   "speed": profile["png_s"], "maximum_deflate": max_deflate})
        elif style == "libpng":
            out.update(format="png", coder="libpng", params={"depth": "png_32" if needs_alpha else "png_24", "matte": matte,
                                                             "zlib_compression": 9 if max_deflate is True else None})
        elif style in ("pngquant", "default") and not is_lossless:                           # the guarded arm (:995); `lodepng` falls to `_` (:1016)
            u8 = lambda v: None if v is None else as_u8(clamp(v, 0.0, 100.0))               # noqa: E731
            speed = ph.get("quantization_speed")
            out.update(format="png", coder="pngquant", params={"quality": u8(manual_quality), "minimum_quality": u8(ph.get("min_quality")),
                                                               "speed": None if speed is None else min(10, max(1, speed)), "maximum_deflate": max_deflate})
        else:
            out.update(format="png", coder="lodepng", params={"maximum_deflate": max_deflate})
    return out


# ---- calculate_encoder_preset (ir4/encoder.rs:5-98) over the parsed instructions -------------------------------------------
def preset_of_instructions(i):
    """i: the parsed output keys {format: "keep"|"jpeg"|..|"auto"|None, qp, qp_dpr, lossless, quality, jpeg_quality, jpeg_progressive,
    jpeg_turbo, jpeg_li, webp_quality, webp_lossless, png_*, accept_*}; absent keys are None."""
    g = i.get
    allow = web_safe()
    allow["color_profiles"] = bool(g("accept_color_profiles"))
    for k in ("webp", "jxl", "avif"):
        if g("accept_" + k) is not None:
            allow[k] = g("accept_" + k)
    target = g("format") or ("auto" if g("qp") is not None else "keep")
    quality = g("quality")
    if target == "auto":
        default_qp = {"percent": float(quality)} if quality is not None else "high"
        return {"auto": {"quality_profile": g("qp") if g("qp") is not None else default_qp, "quality_profile_dpr": g("qp_dpr"), "matte": None,
                         "lossless": g("lossless"), "allow": allow}}
    first = lambda *v: next((float(x) for x in v if x is not None), None)                    # noqa: E731
    return {"format": {"format": target, "quality_profile": g("qp"), "quality_profile_dpr": g("qp_dpr"), "matte": None, "lossless": g("lossless"),
                       "allow": allow, "encoder_hints": {
                           "webp": {"quality": first(g("webp_quality"), quality), "lossless": g("webp_lossless")},
                           "jpeg": {"quality": first(g("jpeg_quality"), quality), "progressive": g("jpeg_progressive"),
                                    "mimic": "jpegli" if g("jpeg_li") is True else "libjpegturbo" if g("jpeg_turbo") is True else None},
                           "png": {"quality": first(g("png_quality")), "min_quality": first(g("png_min_quality")), "quantization_speed": g("png_quantization_speed"),
                                   "mimic": "libpng" if g("png_libpng") is True else None, "hint_max_deflate": g("png_max_deflate"), "lossless": g("png_lossless")},
                           "gif": {}}}}
