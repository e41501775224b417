"""Encoder selection in jobs on an MI355X (Context.set_encoder_selection; csrc/shim_encode.cpp Job::encode_selected over
csrc/encoder_select.cpp): with the switch off the presets `auto` and `format` stay the raw container and the querystring's
format=png stays refused; with it on each of the eight routes writes byte for byte the file of the equivalent named preset, the
preset's matte is applied before every coder, the querystring's output keys pick the coder, a string without one keeps the
source's format, and an animated GIF source passes through a resolved GIF encode frame by frame."""
import io

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra  # noqa: E402
from imageflow_amd.graphics import blend  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import util as U  # noqa: E402
from tests import webp_frames as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = 64, 48
MIME = {"jpg": "image/jpeg", "png": "image/png", "webp": "image/webp", "gif": "image/gif", "ifbgra": "application/x-imageflow-bgra"}


def rows_of(bgra):
    h, w, _ = bgra.shape
    out = np.zeros((h, U.stride_for(w)), np.uint8)
    out[:, :4 * w] = bgra.reshape(h, 4 * w)
    return out


ALPHA = F.photo(W, H, alpha=True, seed=71)
OPAQUE = F.photo(W, H, seed=72)
OPAQUE[..., 3] = 255
RAW = {True: pack_raw_bgra(rows_of(ALPHA), W, H, alpha_meaningful=True), False: pack_raw_bgra(rows_of(OPAQUE), W, H, alpha_meaningful=False)}


def pillow_file(fmt, bgra, **kw):
    b = io.BytesIO()
    rgba = np.ascontiguousarray(bgra[..., [2, 1, 0, 3]])
    (Image.fromarray(rgba, "RGBA") if fmt != "JPEG" else Image.fromarray(np.ascontiguousarray(rgba[..., :3]), "RGB")).save(b, fmt, **kw)
    return b.getvalue()


def animation():
    """three 32 x 24 frames of few colours, 70 ms apart, looping"""
    frames = []
    for k in range(3):
        a = np.zeros((24, 32, 3), np.uint8)
        a[..., 0] = (np.arange(32)[None, :] // 8) * 60
        a[4 + 5 * k:10 + 5 * k, 3 + 7 * k:12 + 7 * k] = (250, 40 * k, 10)
        frames.append(Image.fromarray(a, "RGB").quantize(16))
    b = io.BytesIO()
    frames[0].save(b, "GIF", save_all=True, append_images=frames[1:], duration=70, loop=0)
    return b.getvalue()


def context(selection=True):
    c = Context()
    assert c.set_gif_encoder(True) and c.set_webp_lossy_encoder(True)          # for the named presets the files are compared with
    if selection:
        assert c.set_encoder_selection(True)
    return c


def execute(c, data, job, outputs=(1,), expect=200):
    c.add_input_buffer(0, data)
    for o in outputs:
        c.add_output_buffer(o)
    status, r = c.send_json("v1/execute", job)
    assert status == expect, (status, r, c.error_message())
    if expect != 200:
        return None, None
    entries = {e["io_id"]: e for e in r["data"]["job_result"]["encodes"]}
    return [bytes(c.get_output_buffer(o)) for o in outputs], entries


def steps(*nodes):
    return {"framewise": {"steps": [{"decode": {"io_id": 0}}] + list(nodes)}}


def two_encodes(first, second):
    """one decoded frame into two encode nodes: io 1 and io 2"""
    return {"framewise": {"graph": {"nodes": {"0": {"decode": {"io_id": 0}}, "1": {"encode": {"io_id": 1, "preset": first}}, "2": {"encode": {"io_id": 2, "preset": second}}},
                                    "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 0, "to": 2, "kind": "input"}]}}}


def encode(preset, data, selection=True):
    with context(selection) as c:
        (out,), entries = execute(c, data, steps({"encode": {"io_id": 1, "preset": preset}}))
    return out, entries[1]


def pillow_bgra(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im, np.asarray(im.convert("RGBA"))[..., [2, 1, 0, 3]]


# ---- switch off ---------------------------------------------------------------------------------------------------------------
def test_with_the_switch_off_nothing_changes():
    tap, entry = encode("lodepng", RAW[True], selection=False)              # the raw tap every unknown preset has always been
    assert tap[:7] == b"IFBGRA1" and entry["preferred_extension"] == "ifbgra"
    for preset in ({"format": {"format": "png"}}, {"auto": {"quality_profile": "good"}}, {"auto": {}}):
        out, entry = encode(preset, RAW[True], selection=False)
        assert out == tap and entry["preferred_mime_type"] == MIME["ifbgra"], preset
    with context(False) as c:
        execute(c, RAW[True], {"framewise": {"steps": [{"command_string": {"kind": "ir4", "value": "w=32&format=png", "decode": 0, "encode": 1}}]}}, expect=400)
        assert c.error_code() == 8 and c.error_message()[0].startswith("ActionNotSupported: querystring format=png")


# ---- the eight routes ---------------------------------------------------------------------------------------------------------
WHITE = {"srgb": {"hex": "FFFFFF"}}
ROUTES = {
    "mozjpeg": ({"format": {"format": "jpeg", "quality_profile": "good"}}, {"mozjpeg": {"quality": 73, "progressive": False}}, False, "jpg", False),
    "libjpeg_turbo": ({"format": {"format": "jpg", "encoder_hints": {"jpeg": {"quality": 70, "mimic": "libjpegturbo"}}}},
                      {"libjpeg_turbo": {"quality": 70, "progressive": False, "optimize_huffman_coding": False}}, False, "jpg", False),
    "libpng": ({"format": {"format": "png", "encoder_hints": {"png": {"mimic": "libpng", "hint_max_deflate": True}}}}, {"libpng": {"depth": "png_32", "zlib_compression": 9}}, True, "png", True),
    "lodepng_rgba": ({"format": {"format": "png"}}, {"libpng": {"depth": "png_32"}}, True, "png", True),
    "lodepng_rgb": ({"auto": {"quality_profile": "good", "lossless": "true"}}, {"libpng": {"depth": "png_24"}}, False, "png", True),
    "pngquant": ({"format": {"format": "png", "encoder_hints": {"png": {"quality": 80, "quantization_speed": 3}}}}, {"pngquant": {"quality": 80, "speed": 3}}, True, "png", False),
    "webp_lossless": ({"format": {"format": "webp", "lossless": "true"}}, "webplossless", True, "webp", True),
    "webp_lossy": ({"auto": {"quality_profile": "good", "allow": {"webp": True}}}, {"webplossy": {"quality": 76.0}}, True, "webp", False),
    "gif": ({"format": {"format": "gif"}}, "gif", True, "gif", False)}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_each_route_writes_the_file_of_its_named_preset(route):
    selected, named, alpha, ext, lossless = ROUTES[route]
    with context() as c:
        (out, want), entries = execute(c, RAW[alpha], two_encodes(selected, named), outputs=(1, 2))
    assert out == want and out[:7] != b"IFBGRA1"
    for e in (entries[1], entries[2]):
        assert (e["preferred_mime_type"], e["preferred_extension"], e["w"], e["h"]) == (MIME[ext], ext, W, H)
    im, got = pillow_bgra(out)
    assert im.size == (W, H) and im.format == {"jpg": "JPEG", "png": "PNG", "webp": "WEBP", "gif": "GIF"}[ext]
    if lossless:
        frame = ALPHA if alpha else OPAQUE
        assert np.array_equal(got[..., 3], frame[..., 3])
        seen = frame[..., 3] > 0
        assert np.array_equal(got[seen], frame[seen])


# ---- matte --------------------------------------------------------------------------------------------------------------------
MATTE_ROUTES = {"pngquant": {"format": "png", "encoder_hints": {"png": {"quality": 80}}}, "lodepng": {"format": "png"},
                "webp_lossless": {"format": "webp", "lossless": "true"}, "webp_lossy": {"format": "webp", "quality_profile": "good"}}


def flattened(matte_color32):
    """the alpha frame through the apply_matte wrapper, as the raw container a job decodes"""
    b = Bitmap.from_numpy(np.ascontiguousarray(rows_of(ALPHA)[None]), W, H, U.stride_for(W), DEV, alpha_meaningful=True)
    blend.apply_matte(b, matte_color32)
    torch.cuda.synchronize()
    return pack_raw_bgra(b.to_numpy()[0], W, H, alpha_meaningful=b.alpha_meaningful)


@pytest.mark.parametrize("matte", [("336699", 0xFF336699), ("33669980", 0x80336699)])
@pytest.mark.parametrize("route", sorted(MATTE_ROUTES))
def test_the_matte_is_applied_before_the_coder(route, matte):
    hex_, color32 = matte
    body = MATTE_ROUTES[route]
    out, _ = encode({"format": dict(body, matte={"srgb": {"hex": hex_}})}, RAW[True])
    want, _ = encode({"format": body}, flattened(color32))
    plain, _ = encode({"format": body}, RAW[True])
    assert out == want and out != plain


def test_an_opaque_matte_under_auto_picks_jpeg_and_a_shared_frame_stays_as_it_was():
    out, entry = encode({"auto": {"quality_profile": "good", "matte": WHITE}}, RAW[True])
    want, _ = encode({"mozjpeg": {"quality": 73, "progressive": False, "matte": WHITE}}, RAW[True])
    assert out == want and entry["preferred_mime_type"] == "image/jpeg"
    assert encode({"auto": {"quality_profile": "good"}}, RAW[True])[1]["preferred_mime_type"] == "image/png"
    plain, _ = encode({"format": {"format": "png"}}, RAW[True])
    with context() as c:                                                    # the matte's encode runs first, on a copy of its own
        (first, second), _ = execute(c, RAW[True], two_encodes({"format": {"format": "png", "matte": WHITE}}, {"format": {"format": "png"}}), outputs=(1, 2))
    assert second == plain and first != plain


# ---- querystring jobs -----------------------------------------------------------------------------------------------------------
def querystring_job(value, data, named, split="w=32"):
    """(the file of command_string `value` with its own encode, the file of command_string `split` and then an `encode` with `named`)"""
    with context() as c:
        (out,), entries = execute(c, data, steps({"command_string": {"kind": "ir4", "value": value, "encode": 1}}))
    with context() as c:
        (want,), _ = execute(c, data, steps({"command_string": {"kind": "ir4", "value": split}}, {"encode": {"io_id": 1, "preset": named}}))
    return out, want, entries[1]


@pytest.mark.parametrize("value,named,ext", [("w=32&format=png", {"libpng": {"depth": "png_32"}}, "png"), ("w=32&format=webp&webp.lossless=true", "webplossless", "webp"),
                                             ("w=32&format=gif", "gif", "gif"), ("w=32&qp=good&accept.webp=1", {"webplossy": {"quality": 76.0}}, "webp")])
def test_output_keys_on_an_alpha_png_source(value, named, ext):
    out, want, entry = querystring_job(value, pillow_file("PNG", ALPHA), named)
    assert out == want and (entry["preferred_mime_type"], entry["preferred_extension"], entry["w"], entry["h"]) == (MIME[ext], ext, 32, 24)
    assert pillow_bgra(out)[0].size == (32, 24)


@pytest.mark.parametrize("source", ["png", "gif", "webp", "jpeg"])
def test_a_string_without_an_output_key_keeps_the_format(source):
    data, named, ext = {"png": (pillow_file("PNG", ALPHA), {"libpng": {}}, "png"), "gif": (pillow_file("GIF", OPAQUE), "gif", "gif"),
                        "webp": (pillow_file("WEBP", OPAQUE, lossless=True), {"webplossy": {"quality": 80.0}}, "webp"),        # keep names the format, not lossless
                        "jpeg": (pillow_file("JPEG", OPAQUE, quality=90), {"mozjpeg": {"quality": 90, "progressive": False}}, "jpg")}[source]
    out, want, entry = querystring_job("w=32", data, named)
    assert out == want and (entry["preferred_mime_type"], entry["preferred_extension"]) == (MIME[ext], ext)
    assert pillow_bgra(out)[0].size == (32, 24)


# ---- animation --------------------------------------------------------------------------------------------------------------------
def test_an_animated_gif_passes_through_a_resolved_gif_encode():
    data = animation()
    files = []
    for nodes in ([{"command_string": {"kind": "ir4", "value": "w=16", "encode": 1}}],
                  [{"command_string": {"kind": "ir4", "value": "w=16"}}, {"encode": {"io_id": 1, "preset": "gif"}}]):
        with context() as c:
            assert c.set_gif_animation(True)
            (out,), entries = execute(c, data, steps(*nodes))
        assert (entries[1]["preferred_mime_type"], entries[1]["w"], entries[1]["h"]) == ("image/gif", 16, 12)
        files.append(out)
    assert files[0] == files[1]
    im = Image.open(io.BytesIO(files[0]))
    assert im.n_frames == 3 and im.size == (16, 12)


def test_in_a_graph_only_the_gif_encode_under_the_animated_decode_collects_frames():
    """two branches of one graph, both ending in `format: gif`: the animated source's keeps its three frames, the still source's
    takes frame 0 -- as the same nodes do in steps"""
    gif = {"format": {"format": "gif"}}
    job = {"framewise": {"graph": {"nodes": {"0": {"decode": {"io_id": 0}}, "1": {"encode": {"io_id": 1, "preset": gif}},
                                             "2": {"decode": {"io_id": 2}}, "3": {"encode": {"io_id": 3, "preset": gif}}},
                                   "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 2, "to": 3, "kind": "input"}]}}}
    with context() as c:
        assert c.set_gif_animation(True)
        c.add_input_buffer(2, RAW[False])
        (moving, still), entries = execute(c, animation(), job, outputs=(1, 3))
    assert Image.open(io.BytesIO(moving)).n_frames == 3 and (entries[1]["w"], entries[1]["h"]) == (32, 24)
    im = Image.open(io.BytesIO(still))
    assert getattr(im, "n_frames", 1) == 1 and im.size == (W, H) and entries[3]["preferred_mime_type"] == "image/gif"
