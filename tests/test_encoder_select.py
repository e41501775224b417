"""Encoder selection for the presets `auto` and `format` without a GPU (csrc/encoder_select.cpp through
ifhip_shim_resolve_encoder_preset and ifhip_shim_querystring_encoder_preset): hand-derived anchors from the reference's tables
(imageflow_core/src/codecs/auto.rs), a fixed-seed sweep against the independent float32 restatement in
tests/encoder_select_oracle.py, the points where the reference itself panics (its guarded interpolate_value) against the
documented rule, serde's refusals as InvalidJson, and the header / bindings / library agreement."""
import os
import random
import re

import numpy as np
import pytest

from imageflow_amd import _native
from imageflow_amd import abi
from tests import encoder_select_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ifhip_shim_querystring_encoder_preset", "ifhip_shim_resolve_encoder_preset"]
SOURCES = {"none": dict(source=None), "jpeg": dict(source="jpeg"), "png": dict(source="png", source_lossless=True),
           "png8": dict(source="png", source_lossless=False), "gif": dict(source="gif"), "gif3": dict(source="gif", source_frames=3),
           "webp_ll": dict(source="webp", source_lossless=True), "webp": dict(source="webp", source_lossless=False)}


def resolve_qs(qs, src="none", alpha=False, w=64, h=48):
    return abi.resolve_encoder_preset(abi.querystring_encoder_preset(qs), alpha_meaningful=alpha, w=w, h=h, **SOURCES[src])


def coder(r):
    return r["format"], r["coder"]


# ---- hand-derived anchors (no oracle) ----------------------------------------------------------------------------------------
def test_anchors_opaque_frame_jpeg_source():
    # High is the row p 91 / moz 91 / webp 93; web_safe has no jpeg_progressive, so progressive is off; 91 > 90 prefers webp once allowed
    r = resolve_qs("qp=high", "jpeg")
    assert coder(r) == ("jpeg", "mozjpeg") and r["params"] == {"quality": 91, "progressive": False, "matte": None}
    r = resolve_qs("qp=high&accept.webp=1", "jpeg")
    assert coder(r) == ("webp", "webp_lossy") and r["params"] == {"quality": 93.0}


def test_anchors_frame_with_meaningful_alpha():
    r = resolve_qs("qp=high", "jpeg", alpha=True)                    # no png.quality: lossless defaults to true -> lodepng
    assert coder(r) == ("png", "lodepng") and r["params"] == {"maximum_deflate": None}
    r = resolve_qs("qp=high&accept.webp=1", "jpeg", alpha=True)
    assert coder(r) == ("webp", "webp_lossy") and r["params"] == {"quality": 93.0}


def test_anchors_other_strings():
    # `lossless=true` alone is format=keep: without a source it falls through to auto-selection (with a JPEG source keep is jpeg)
    assert coder(resolve_qs("lossless=true")) == ("png", "lodepng")
    assert coder(resolve_qs("lossless=true&accept.webp=1")) == ("webp", "webp_lossless")
    assert coder(resolve_qs("format=auto&lossless=true", "jpeg")) == ("png", "lodepng")
    assert coder(resolve_qs("format=auto&lossless=true&accept.webp=1", "jpeg")) == ("webp", "webp_lossless")
    assert coder(resolve_qs("lossless=true", "jpeg")) == ("jpeg", "mozjpeg")
    r = resolve_qs("format=png&png.quality=80")
    assert coder(r) == ("png", "pngquant") and r["params"] == {"quality": 80, "minimum_quality": None, "speed": None, "maximum_deflate": None}
    r = resolve_qs("format=png&qp=good&png.lossless=false")
    assert coder(r) == ("png", "pngquant") and r["params"] == {"quality": 100, "minimum_quality": 50, "speed": 4, "maximum_deflate": None}
    r = resolve_qs("format=png&png.libpng=true")
    assert coder(r) == ("png", "libpng") and r["params"] == {"depth": "png_24", "matte": None, "zlib_compression": None}
    assert resolve_qs("format=png&png.libpng=true", alpha=True)["params"]["depth"] == "png_32"
    assert resolve_qs("format=png&png.libpng=true&png.max_deflate=true")["params"]["zlib_compression"] == 9
    r = resolve_qs("format=jpg")
    assert coder(r) == ("jpeg", "mozjpeg") and r["params"] == {"quality": 90, "progressive": False, "matte": None}
    r = resolve_qs("format=jpg&jpeg.turbo=1&quality=70")
    assert coder(r) == ("jpeg", "libjpeg_turbo")
    assert r["params"] == {"quality": 70, "progressive": False, "optimize_huffman_coding": False, "matte": None}
    # good is ssim2 70; dpr 1.5 doubles it, clamped to 90: the `highest` row exactly (moz 96)
    r = resolve_qs("qp=good&qp.dpr=1.5", "jpeg")
    assert coder(r) == ("jpeg", "mozjpeg") and r["params"]["quality"] == 96
    assert resolve_qs("format=jpg&jpeg.li=1")["coder"] == "mozjpeg"                        # mimic jpegli is the mozjpeg route


def test_anchors_png_mimic_without_a_profile():
    """create_png_auto's match on the style (auto.rs:966-1023): libpng first; pngquant only for `pngquant | default` and not lossless;
    everything else -- `mimic: lodepng` whatever quality or lossless say -- is lodepng."""
    def png(hints, **more):
        return abi.resolve_encoder_preset({"format": dict({"format": "png", "encoder_hints": {"png": hints}}, **more)})
    assert coder(png({"mimic": "lodepng", "quality": 80})) == ("png", "lodepng")
    assert coder(png({"mimic": "lodepng", "quality": 80}, lossless="false")) == ("png", "lodepng")
    assert coder(png({"mimic": "lodepng", "lossless": "false", "hint_max_deflate": True})) == ("png", "lodepng")
    assert png({"mimic": "lodepng", "lossless": "false", "hint_max_deflate": True})["params"] == {"maximum_deflate": True}
    r = png({"mimic": "pngquant", "quality": 80})
    assert coder(r) == ("png", "pngquant") and r["params"] == {"quality": 80, "minimum_quality": None, "speed": None, "maximum_deflate": None}
    assert coder(png({"mimic": "default", "quality": 80})) == ("png", "pngquant")
    assert coder(png({"quality": 80})) == ("png", "pngquant")
    assert coder(png({"mimic": "pngquant"})) == ("png", "lodepng")                         # no quality: lossless defaults to true
    assert coder(png({"mimic": "pngquant"}, lossless="false")) == ("png", "pngquant")
    assert coder(png({"mimic": "libpng", "quality": 80}, lossless="false")) == ("png", "libpng")
    # with a profile the style is not looked at (:945-964): lossy unless the profile's png is 100 or lossless holds
    assert coder(png({"mimic": "lodepng"}, quality_profile="good", lossless="false")) == ("png", "pngquant")
    assert coder(png({"mimic": "pngquant"}, quality_profile="lossless")) == ("png", "lodepng")


def test_anchors_keep_and_sources():
    want = {"png": ("png", "lodepng"), "gif": ("gif", "gif"), "webp_ll": ("webp", "webp_lossy"), "webp": ("webp", "webp_lossy"), "jpeg": ("jpeg", "mozjpeg")}
    for src, expected in want.items():
        assert coder(resolve_qs("format=keep", src)) == expected, src
        assert coder(resolve_qs("w=32", src)) == expected, src                             # no output key at all: keep
    assert resolve_qs("format=keep", "webp")["params"] == {"quality": 80.0}
    assert coder(resolve_qs("lossless=keep", "webp_ll")) == ("webp", "webp_lossless")
    assert coder(resolve_qs("lossless=keep", "webp")) == ("webp", "webp_lossy")
    assert coder(resolve_qs("format=auto", "gif3")) == ("gif", "gif")                      # an animated source: gif before the frame is looked at
    assert coder(resolve_qs("format=auto", "gif3", alpha=True)) == ("gif", "gif")
    assert coder(resolve_qs("format=auto", "gif")) == ("jpeg", "mozjpeg")
    assert coder(resolve_qs("format=avif", "jpeg")) == ("jpeg", "mozjpeg")                 # not built: format_auto_select(..).unwrap_or(Jpeg)
    assert coder(resolve_qs("format=jxl", "jpeg", alpha=True)) == ("png", "lodepng")
    assert coder(resolve_qs("format=keep", "none", alpha=True)) == ("png", "lodepng")      # the raw container: keep falls through
    with pytest.raises(abi.EncoderSelectError) as e:
        abi.resolve_encoder_preset({"auto": {"quality_profile": "high", "allow": {}}})
    assert e.value.status == abi.SELECT_INVALID and str(e.value) == "InvalidArgument: No formats enabled; try 'allow': { 'web_safe':true}"
    assert coder(abi.resolve_encoder_preset({"format": {"format": "avif", "allow": {}}})) == ("jpeg", "mozjpeg")
    assert coder(abi.resolve_encoder_preset({"format": {"format": "png", "allow": {}}})) == ("png", "lodepng")


def test_anchors_matte():
    white = {"srgb": {"hex": "FFFFFF"}}
    r = abi.resolve_encoder_preset({"auto": {"quality_profile": "good", "matte": white}}, alpha_meaningful=True)
    assert coder(r) == ("jpeg", "mozjpeg") and r["matte"] == white and r["params"]["matte"] == white      # an opaque matte: no alpha to keep
    r = abi.resolve_encoder_preset({"auto": {"quality_profile": "good", "matte": {"srgb": {"hex": "FFFFFF80"}}}}, alpha_meaningful=True)
    assert coder(r) == ("png", "lodepng") and r["matte"] == {"srgb": {"hex": "FFFFFF80"}}


# ---- the querystring's preset -------------------------------------------------------------------------------------------------
def test_querystring_presets_against_the_oracle():
    cases = [("", {}), ("w=30&h=20&mode=crop", {}), ("format=png", {"format": "png"}), ("thumbnail=gif", {"format": "gif"}),
             ("format=bogus&thumbnail=webp", {"format": "webp"}), ("format=bogus", {}),
             ("qp=good", {"qp": "good"}), ("qp=medium-low", {"qp": "mediumlow"}), ("qp=MediumHigh", {"qp": "good"}), ("qp=37.5", {"qp": {"percent": 37.5}}),
             ("qp=250", {"qp": {"percent": 100.0}}), ("qp=-3", {"qp": {"percent": 0.0}}), ("qp=nan", {"qp": {"percent": 0.0}}), ("qp=what", {}),
             ("quality=80&format=auto", {"format": "auto", "quality": 80}), ("quality=80", {"quality": 80}), ("quality=80.5", {}),
             ("qp=quality&quality=65", {"qp": {"percent": 65.0}, "quality": 65}), ("qp=quality", {}), ("qp=quality&quality=300", {"qp": {"percent": 300.0}, "quality": 300}),
             ("qp=good&qp.dpr=2", {"qp": "good", "qp_dpr": 2.0}), ("qp=good&qp.dppx=1.5x", {"qp": "good", "qp_dpr": 1.5}),
             ("qp=good&qp.dpr=dpr&zoom=2", {"qp": "good", "qp_dpr": 2.0}), ("qp=good&qp.dpr=zoom&dppx=4x", {"qp": "good", "qp_dpr": 4.0}),
             ("qp=good&qp.dpr=dpr", {"qp": "good"}), ("qp=good&qp.dpr=nope&qp.dppx=6", {"qp": "good", "qp_dpr": 6.0}), ("qp=good&qp.dpr=nan", {"qp": "good"}),
             ("lossless=keep", {"lossless": "keep"}), ("lossless=Preserve", {"lossless": "keep"}), ("lossless=1", {"lossless": "true"}), ("lossless=off", {"lossless": "false"}),
             ("accept.webp=1&accept.avif=true&accept.jxl=0&accept.color_profiles=yes", {"accept_webp": True, "accept_avif": True, "accept_jxl": False, "accept_color_profiles": True}),
             ("format=jpg&jpeg.quality=55&quality=70&jpeg.progressive=true&jpeg.turbo=1", {"format": "jpeg", "jpeg_quality": 55, "quality": 70, "jpeg_progressive": True, "jpeg_turbo": True}),
             ("format=jpeg&jpeg.li=true&jpeg.turbo=true", {"format": "jpeg", "jpeg_li": True, "jpeg_turbo": True}),
             ("format=webp&webp.quality=66.5&webp.lossless=keep&quality=10", {"format": "webp", "webp_quality": 66.5, "webp_lossless": "keep", "quality": 10}),
             ("format=webp&webp.quality=inf", {"format": "webp"}),
             ("format=png&png.quality=80&png.min_quality=%2B20&png.quantization_speed=3&png.libpng=0&png.max_deflate=1&png.lossless=false",
              {"format": "png", "png_quality": 80, "png_min_quality": 20, "png_quantization_speed": 3, "png_libpng": False, "png_max_deflate": True, "png_lossless": "false"}),
             ("format=png&png.quality=256&png.min_quality=-1", {"format": "png"})]
    for spelling in ("jpg", "jpe", "jif", "jfif", "jfi", "exif", "jpeg", "JPEG"):
        cases.append(("format=" + spelling, {"format": "jpeg"}))
    for spelling, fmt in (("png", "png"), ("gif", "gif"), ("webp", "webp"), ("avif", "avif"), ("jxl", "jxl"), ("jpegxl", "jxl"), ("Auto", "auto"), ("keep", "keep")):
        cases.append(("format=" + spelling, {"format": fmt}))
    for qs, parsed in cases:
        assert abi.querystring_encoder_preset(qs) == O.preset_of_instructions(parsed), qs


def test_querystring_refusals_stay():
    for qs in ("avif.quality=50", "jxl.distance=1", "jxl.lossless=true", "subsampling=420", "srcset=webp-70", "frame=2", "page=1", "format=png&bogus=1", "autorotate=false"):
        with pytest.raises(abi.EncoderSelectError) as e:
            abi.querystring_encoder_preset(qs)
        assert e.value.status == abi.SELECT_REFUSED and str(e.value).startswith("ActionNotSupported"), qs


# ---- the sweep ----------------------------------------------------------------------------------------------------------------
PROFILES = ["lowest", "low", "mediumlow", "medium", "good", "high", "highest", "lossless", "percent"]
DPRS = [None, 0.5, 1, 1.5, 2, 3, 4, 6, 9, 12, 20]
FORMATS = ["webp", "jpeg", "jpg", "png", "avif", "jxl", "gif", "keep"]
ALLOWS = [None, {}, {"web_safe": True}, {"modern_web_safe": True}, {"all": True}, {"webp": True}, {"png": True, "gif": True}, {"jpeg": True, "jpeg_progressive": True},
          {"web_safe": True, "webp": True}, {"web_safe": True, "jpeg_progressive": True}, {"jpeg": False, "webp": True, "web_safe": False}, {"gif": True},
          {"modern_web_safe": True, "webp": False}, {"avif": True, "jxl": True}, {"avif": True, "jxl": True, "png": True}]
MATTES = [None, None, None, "black", "transparent", {"srgb": {"hex": "FFFFFF"}}, {"srgb": {"hex": "00FF0080"}}, {"srgb": {"hex": "#abcf"}}]
SWEEP_SOURCES = [(None, {}), ({"format": "jpeg", "lossless": False, "animated": False}, dict(source="jpeg")),
                 ({"format": "png", "lossless": True, "animated": False}, dict(source="png", source_lossless=True)),
                 ({"format": "png", "lossless": False, "animated": False}, dict(source="png", source_lossless=False)),
                 ({"format": "gif", "lossless": False, "animated": False}, dict(source="gif", source_frames=1)),
                 ({"format": "gif", "lossless": False, "animated": True}, dict(source="gif", source_frames=3)),
                 ({"format": "webp", "lossless": True, "animated": False}, dict(source="webp", source_lossless=True)),
                 ({"format": "webp", "lossless": False, "animated": False}, dict(source="webp", source_lossless=False))]
SIZES = [(64, 48), (1731, 1733), (1733, 1732), (2000, 2000)]                               # pixel counts on both sides of 3 000 000


def random_hints(rng):
    def maybe(values):
        return rng.choice(values) if rng.random() < 0.6 else None
    h = {}
    if rng.random() < 0.8:
        h["jpeg"] = {"quality": maybe([0, 37.5, 70, 90, 100, 140, -5]), "progressive": maybe([True, False]), "mimic": maybe(["jpegli", "libjpegturbo", "mozjpeg", "default"])}
    if rng.random() < 0.8:
        h["png"] = {"quality": maybe([0, 55.5, 80, 100, 300]), "min_quality": maybe([0, 20, 99.9, -1]), "quantization_speed": maybe([0, 1, 3, 10, 11, 255]),
                    "mimic": maybe(["libpng", "lodepng", "pngquant", "default"]), "hint_max_deflate": maybe([True, False]), "lossless": maybe(["keep", "true", "false"])}
    if rng.random() < 0.8:
        h["webp"] = {"quality": maybe([0, 33.25, 80, 100, 120, -1]), "lossless": maybe(["keep", "true", "false"])}
    if rng.random() < 0.5:
        h["gif"] = {}
    return h


def sweep_cases():
    rng = random.Random(20260101)
    cases = []
    for percent2 in range(0, 201):                                   # every percent x every dpr, on the JPEG, WebP and PNG tables
        for dpr in DPRS:
            fmt = ("jpeg", "webp", "png")[(percent2 + DPRS.index(dpr)) % 3]
            body = {"format": fmt, "quality_profile": {"percent": percent2 / 2}, "quality_profile_dpr": dpr}
            if fmt == "png":
                body["lossless"] = "false"
            cases.append(({"format": body}, 0, False, (64, 48)))
    while len(cases) < 20000:
        is_auto = rng.random() < 0.4
        qp = rng.choice(PROFILES) if is_auto else rng.choice(PROFILES + [None, None])
        if qp == "percent":
            qp = {"percent": rng.randrange(0, 201) / 2}
        body = {"quality_profile": qp, "quality_profile_dpr": rng.choice(DPRS), "matte": rng.choice(MATTES), "lossless": rng.choice([None, "keep", "true", "false"]),
                "allow": rng.choice(ALLOWS)}
        if not is_auto:
            body["format"] = rng.choice(FORMATS)
            body["encoder_hints"] = random_hints(rng) if rng.random() < 0.8 else None
        body = {k: v for k, v in body.items() if v is not None or rng.random() < 0.5}      # None as null and as a missing field
        if is_auto:
            body.setdefault("quality_profile", "high")
        cases.append(({"auto" if is_auto else "format": body}, rng.randrange(len(SWEEP_SOURCES)), rng.random() < 0.5, rng.choice(SIZES)))
    return cases


def test_sweep_against_the_oracle():
    cases = sweep_cases()
    assert len(cases) >= 20000
    panicked = refused = 0
    coders = set()
    for preset, s, alpha, (w, h) in cases:
        source, kwargs = SWEEP_SOURCES[s]
        try:
            expected = O.resolve(preset, source, alpha, w, h)
        except O.NoFormats as e:
            with pytest.raises(abi.EncoderSelectError) as got:
                abi.resolve_encoder_preset(preset, alpha_meaningful=alpha, w=w, h=h, **kwargs)
            assert got.value.status == abi.SELECT_INVALID and str(got.value) == "InvalidArgument: " + str(e), preset
            refused += 1
            continue
        got = abi.resolve_encoder_preset(preset, alpha_meaningful=alpha, w=w, h=h, **kwargs)
        assert got == expected, (preset, source, alpha, w, h)
        panicked += O.State.panicked                                 # the reference would not have answered here: the documented difference
        coders.add(got["coder"])
    assert coders == {"mozjpeg", "libjpeg_turbo", "lodepng", "pngquant", "libpng", "webp_lossy", "webp_lossless", "gif"}
    assert refused > 100 and 1000 < panicked < len(cases) - 1000


def test_where_the_reference_panics():
    """The documented rule: an interpolated profile panics in the reference unless 55 < percent < 73 on the percent axis and, where
    quality_profile_dpr moves it, 60 < target < 70 on the ssim2 axis; the table's own rows never interpolate.  At every point, marked
    or not, the library's JPEG, WebP and palette-PNG parameters are the ones the oracle's hints give: at the marked ones that is the
    unguarded a + ratio * (b - a)."""

    def library(fmt, percent, dpr, **more):
        body = dict({"format": fmt, "quality_profile": {"percent": percent}, "quality_profile_dpr": dpr}, **more)
        return abi.resolve_encoder_preset({"format": body})["params"]
    row_p = [float(q["p"]) for q in O.QUALITY_HINTS]
    row_s = [float(q["ssim2"]) for q in O.QUALITY_HINTS]
    f32 = np.float32
    panics = 0
    for percent2 in range(0, 201):
        percent = percent2 / 2
        O.State.panicked = False
        base = O.get_quality_hints({"percent": percent})
        first = O.State.panicked
        assert first == (percent not in row_p and not 55 < percent < 73), percent
        for dpr in DPRS:
            O.State.panicked = False
            hints = O.get_quality_hints_with_dpr({"percent": percent}, dpr)
            assert library("jpeg", percent, dpr)["quality"] == O.as_u8(O.clamp(hints["moz"], 0.0, 100.0)), (percent, dpr)
            assert library("webp", percent, dpr) == {"quality": float(hints["webp"])}, (percent, dpr)
            if hints["png"] != 100:
                assert library("png", percent, dpr, lossless="false") == {"quality": hints["png_max"], "minimum_quality": hints["png"], "speed": hints["png_s"],
                                                                          "maximum_deflate": None}, (percent, dpr)
            else:
                assert abi.resolve_encoder_preset({"format": {"format": "png", "quality_profile": {"percent": percent}, "quality_profile_dpr": dpr,
                                                              "lossless": "false"}})["coder"] == "lodepng"
            if dpr is None or dpr == 3:
                assert O.State.panicked == first, (percent, dpr)
            else:
                target = float(O.clamp(f32(base["ssim2"] * f32(f32(3.0) / O.clamp(dpr, 0.1, 12.0))), 10.0, 90.0))
                second = target not in row_s and not 60 < target < 70
                assert O.State.panicked == (first or second), (percent, dpr, target)
            panics += O.State.panicked
    assert 0 < panics < 201 * len(DPRS)
    for name in PROFILES[:8]:                                        # a named profile without dpr is a row
        O.State.panicked = False
        O.get_quality_hints_with_dpr(name, None)
        assert not O.State.panicked


def test_values_inside_the_reference_s_own_intervals():
    # 64 lies in (55, 73): ratio 0.5 -> moz 65, webp 64.5, png 25, png_max 77 (all f32-exact)
    r = abi.resolve_encoder_preset({"format": {"format": "jpeg", "quality_profile": {"percent": 64}}})
    assert r["params"]["quality"] == 65
    r = abi.resolve_encoder_preset({"format": {"format": "webp", "quality_profile": {"percent": 64}}})
    assert r["params"] == {"quality": 64.5}
    r = abi.resolve_encoder_preset({"format": {"format": "png", "quality_profile": {"percent": 64}, "lossless": "false"}})
    assert r["params"] == {"quality": 77, "minimum_quality": 25, "speed": 4, "maximum_deflate": None}
    # the ssim2 quirk: good (ssim2 70) at dpr 3.5 targets 60, the `medium` row itself; at dpr 3.25 it targets 64.615..., inside (60, 70),
    # and the ratio is formed from p: (64.615 - 55) / (73 - 55)
    assert abi.resolve_encoder_preset({"format": {"format": "jpeg", "quality_profile": "good", "quality_profile_dpr": 3.5}})["params"]["quality"] == 57
    target = np.float32(70) * (np.float32(3) / np.float32(3.25))
    moz = np.float32(57) + ((target - np.float32(55)) / np.float32(18)) * np.float32(16)
    assert abi.resolve_encoder_preset({"format": {"format": "jpeg", "quality_profile": "good", "quality_profile_dpr": 3.25}})["params"]["quality"] == int(moz) == 65


# ---- serde's refusals -----------------------------------------------------------------------------------------------------------
def test_reader_errors_are_invalid_json():
    bad = [{"auto": {}}, {"auto": {"quality_profile": None}}, {"auto": {"quality_profile": "Good"}}, {"auto": {"quality_profile": "medium-low"}},
           {"auto": {"quality_profile": {"percent": "80"}}}, {"auto": {"quality_profile": 80}}, {"auto": {"quality_profile": {"percent": 80, "x": 1}}},
           {"auto": "high"}, {"auto": {"quality_profile": "high", "lossless": True}}, {"auto": {"quality_profile": "high", "lossless": "maybe"}},
           {"auto": {"quality_profile": "high", "quality_profile_dpr": "2"}}, {"auto": {"quality_profile": "high", "allow": {"webp": 1}}},
           {"auto": {"quality_profile": "high", "allow": []}}, {"auto": {"quality_profile": "high", "matte": "white"}}, {"auto": {"quality_profile": "high", "matte": 3}},
           {"format": {}}, {"format": {"format": None}}, {"format": {"format": "tiff"}}, {"format": {"format": "PNG"}}, {"format": {"format": 1}},
           {"format": {"format": "png", "encoder_hints": []}}, {"format": {"format": "png", "encoder_hints": {"png": {"quality": "80"}}}},
           {"format": {"format": "png", "encoder_hints": {"png": {"quantization_speed": 256}}}}, {"format": {"format": "png", "encoder_hints": {"png": {"quantization_speed": 1.5}}}},
           {"format": {"format": "png", "encoder_hints": {"png": {"mimic": "optipng"}}}}, {"format": {"format": "png", "encoder_hints": {"png": {"hint_max_deflate": "true"}}}},
           {"format": {"format": "png", "encoder_hints": {"png": {"lossless": False}}}}, {"format": {"format": "jpeg", "encoder_hints": {"jpeg": {"progressive": 1}}}},
           {"format": {"format": "jpeg", "encoder_hints": {"jpeg": {"mimic": "turbo"}}}}, {"format": {"format": "jpeg", "encoder_hints": {"jpeg": 90}}},
           {"format": {"format": "webp", "encoder_hints": {"webp": {"quality": True}}}}, {"format": {"format": "webp", "encoder_hints": {"webp": {"lossless": "yes"}}}},
           {"format": {"format": "gif", "encoder_hints": {"gif": 1}}}, {"mozjpeg": {"quality": 90}}, "gif", {"auto": {"quality_profile": "high"}, "format": {"format": "png"}}]
    for preset in bad:
        with pytest.raises(abi.EncoderSelectError) as e:
            abi.resolve_encoder_preset(preset)
        assert e.value.status == abi.SELECT_INVALID_JSON and str(e.value).startswith("InvalidJson"), preset
    with pytest.raises(abi.EncoderSelectError) as e:
        abi.resolve_encoder_preset(b'{"auto": {"quality_profile": ')
    assert e.value.status == abi.SELECT_INVALID_JSON
    # what serde takes: unknown fields, null for every Option, an `auto` with encoder_hints it never reads
    ok = {"auto": {"quality_profile": {"percent": 64}, "quality_profile_dpr": None, "matte": None, "lossless": None, "allow": None, "encoder_hints": 7, "extra": [1]}}
    assert abi.resolve_encoder_preset(ok)["params"]["quality"] == 65
    with pytest.raises(abi.EncoderSelectError) as e:                 # an argument, not JSON
        abi._select_call(abi._bind().ifhip_shim_resolve_encoder_preset, b"{}", 2, 9, 0, 1, 0, 1, 1)
    assert e.value.status == abi.SELECT_INVALID


# ---- the entry points ---------------------------------------------------------------------------------------------------------
def test_header_bindings_and_library_agree():
    header = open(os.path.join(ROOT, "include", "imageflow_hip_encoder_select.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop_encoder_select.rs")).read()
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "imageflow_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "include", "imageflow_abi_subset.h")).read()
    L = _native.lib()
    declared = re.findall(r"IMAGEFLOW_SHIM_API\s+\w+\s+(\w+)\(", header)
    bound = re.findall(r"\bpub fn (\w+)\(", bindings)
    assert sorted(declared) == sorted(bound) == sorted(ENTRIES)
    for name in ENTRIES:
        assert name + "(" not in main, name
        assert getattr(L, name) is not None
    for name, value in re.findall(r"#define (IFHIP_SELECT_\w+) (\d+)", header):
        assert re.search(r"pub const %s: c_int = %s;" % (name, value), bindings), name
    assert abi.SOURCE_KINDS == {None: 0, "raw": 0, "jpeg": 1, "png": 2, "gif": 3, "webp": 4}
    for name in os.listdir(os.path.join(ROOT, "include")):
        assert not re.search(r'#include\s*"imageflow_hip_encoder_select\.h"', open(os.path.join(ROOT, "include", name)).read()), name
    assert re.search(r"IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_encoder_selection\(struct imageflow_context \*context, int on\)", shim)
    assert L.ifhip_shim_context_set_encoder_selection is not None
    for cite in ("auto.rs", "encoder.rs", "interpolate_value"):
        assert cite in header, cite


def test_the_switch_is_off_by_default_and_answers():
    with abi.Context() as c:
        assert c.set_encoder_selection(True) and c.set_encoder_selection(False)


def test_short_buffers_report_the_size():
    import ctypes as C
    L = abi._bind()
    needed = C.c_size_t()
    assert L.ifhip_shim_querystring_encoder_preset(b"format=png", None, 0, C.byref(needed)) == 0 and needed.value > 100
    small = C.create_string_buffer(8)
    assert L.ifhip_shim_querystring_encoder_preset(b"format=png", small, 8, C.byref(needed)) == 0 and small.value == b""
    assert L.ifhip_shim_querystring_encoder_preset(None, None, 0, C.byref(needed)) == abi.SELECT_INVALID
