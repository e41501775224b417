"""`command_string` with the full RIAPI key set on the GPU: a querystring job gives, byte for byte, the job built from the
decoder commands and nodes the Python restatement of imageflow_riapi (imageflow_amd/riapi) expands the same string to.
Three small sources, chosen so that the differences the layout has to split are odd: a 97x61 raw frame with meaningful
alpha, a 40x90 opaque raw frame, a 640x400 4:2:0 JPEG.  Every job takes milliseconds."""
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd import riapi  # noqa: E402
from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402

RAW = {"lodepng": {"maximum_deflate": False}}       # this shim writes its raw BGRA container for non-JPEG presets
_cache = {}


def source(name):
    if name in _cache:
        return _cache[name]
    rng = np.random.default_rng(len(name))
    if name in ("alpha", "opaque", "big"):
        w, h = {"alpha": (97, 61), "opaque": (40, 90), "big": (600, 450)}[name]
        y, x = np.mgrid[0:h, 0:w]
        f = np.empty((h, w, 4), np.uint8)
        f[..., 0] = 30 + (x * 200) // w
        f[..., 1] = 40 + (y * 180) // h
        f[..., 2] = rng.integers(0, 256, (h, w))
        f[..., 3] = 255 if name != "alpha" else np.clip(((x + y) * 300) // (w + h) + rng.integers(0, 20, (h, w)), 0, 255)
        r = (pack_raw_bgra(np.ascontiguousarray(f).reshape(h, 4 * w), w, h, alpha_meaningful=name == "alpha"), w, h)
    else:
        PIL = pytest.importorskip("PIL.Image")
        y, x = np.mgrid[0:400, 0:640]
        img = np.stack([(x * 255) // 640, (y * 255) // 400, 128 + 100 * np.sin(x / 9.0) * np.cos(y / 7.0)], -1) + rng.integers(-8, 9, (400, 640, 3))
        b = io.BytesIO()
        PIL.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(b, "JPEG", quality=90, subsampling="4:2:0")
        r = (b.getvalue(), 640, 400)
    _cache[name] = r
    return r


def run(steps, data, marks=(), expect=200):
    with Context() as c:
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        for k, m in enumerate(marks):
            c.add_input_buffer(2 + k, m)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": steps}})
        assert status == expect, (status, r, steps)
        return bytes(c.get_output_buffer(1)) if expect == 200 else r


def decoded_size(w, h, commands):
    """MzDec::apply_downscaling (mozjpeg_decoder.rs:588-618): the smallest i/8 (7 is skipped) that covers the hints"""
    for cmd in commands:
        if isinstance(cmd, dict) and "jpeg_downscale_hints" in cmd:
            hw, hh = cmd["jpeg_downscale_hints"]["width"], cmd["jpeg_downscale_hints"]["height"]
            if hw > 0 and hh > 0 and (w > hw or h > hh):
                for i in (1, 2, 3, 4, 5, 6):
                    if -(-w * i // 8) >= hw and -(-h * i // 8) >= hh:
                        return -(-w * i // 8), -(-h * i // 8)
    return w, h


def explicit_job(qs, name, watermarks=None, preset=RAW):
    """decode with the mirror's decoder commands, the mirror's steps for the size that decode gives, a raw-container encode"""
    data, w, h = source(name)
    commands = riapi.expand_text(qs, w, h, watermarks=watermarks)["decoder_commands"]
    dw, dh = decoded_size(w, h, commands) if name == "jpeg" else (w, h)
    steps = riapi.expand_text(qs, dw, dh, w, h, watermarks)["steps"]
    decode = {"io_id": 0, "commands": commands} if commands else {"io_id": 0}
    return [{"decode": decode}] + steps + [{"encode": {"io_id": 1, "preset": preset}}]


def querystring_job(qs, watermarks=None):
    node = {"kind": "ir4", "value": qs, "decode": 0, "encode": 1}
    if watermarks is not None:
        node["watermarks"] = watermarks
    return [{"command_string": node}]


MODES = ["max", "pad", "crop", "stretch"]
SCALES = ["down", "up", "both", "canvas"]
TABLE = ["w=%d&h=%d&mode=%s&scale=%s" % (w, h, m, s) for m in MODES for s in SCALES for w, h in ((120, 60), (30, 60))] + [
    "w=120&h=60&mode=aspectcrop", "w=30&h=60&mode=aspectcrop", "w=120&h=60", "w=30&h=60", "w=200&h=100&scale=both&mode=crop", "zoom=0.5", "w=33&zoom=2&scale=both",
    "crop=10,5,-7,-9", "crop=10,20,90,80&cropxunits=100&cropyunits=100&w=30", "c=5,5,95,60&h=25", "w=31&h=31&mode=crop&c.gravity=20,80&scale=both",
    "w=31&h=31&mode=crop&anchor=bottomright&scale=both", "w=70&h=70&anchor=bottomright&bgcolor=aaeeff", "srotate=90&sflip=x&w=30", "rotate=270&flip=y&w=30",
    "srotate=180&crop=0,0,20,20&rotate=90&flip=xy", "w=50&h=50&bgcolor=aaeeff&mode=pad", "w=50&h=50&bgcolor=ff000080&mode=pad&scale=both",
    "w=30&s.alpha=0.5", "w=30&s.brightness=0.2", "w=30&s.contrast=-0.3", "w=30&s.saturation=0.7", "w=30&s.sepia=true", "w=30&s.grayscale=bt709",
    "w=30&s.alpha=0.5&s.brightness=0.2&s.contrast=-0.3&s.saturation=0.7&s.sepia=true&s.grayscale=flat", "f.sharpen=15", "f.sharpen=15&f.sharpen_when=downscaling",
    "w=30&f.sharpen=40&f.sharpen_when=sizediffers", "w=150&scale=both&up.filter=ginseng", "w=150&scale=both&up.colorspace=srgb", "w=30&down.colorspace=srgb&up.colorspace=linear",
    "w=30&down.filter=mitchell&up.filter=box", "w=45&h=45&s.roundcorners=20&bgcolor=red", "maxwidth=35&maxheight=35", "w=50&h=50&mode=pad&watermark_red_dot=true&rotate=90",
    "w=30&a.balancewhite=true&s.grayscale=ry"]


@pytest.mark.parametrize("qs", TABLE)
def test_querystring_job_equals_the_explicit_job(qs):
    for name in ("alpha", "opaque") + (("jpeg",) if TABLE.index(qs) % 3 == 0 or "crop" in qs or "rotate" in qs else ()):
        data = source(name)[0]
        got, want = run(querystring_job(qs), data), run(explicit_job(qs, name), data)
        assert got == want, (qs, name, unpack_raw_bgra(got)[1:], unpack_raw_bgra(want)[1:])                # the container: pixels, size, alpha flag
        # the form with a parent frame and decode: null runs the same nodes on the full-size decode
        w, h = source(name)[1:]
        parent = [{"decode": {"io_id": 0}}, {"command_string": {"kind": "ir4", "value": qs, "decode": None}}, {"encode": {"io_id": 1, "preset": RAW}}]
        nodes = [{"decode": {"io_id": 0}}] + riapi.expand_text(qs, w, h)["steps"] + [{"encode": {"io_id": 1, "preset": RAW}}]
        assert run(parent, data) == run(nodes, data), (qs, name)


def test_format_jpg_pads_onto_white():
    PIL = pytest.importorskip("PIL.Image")
    qs = "w=50&h=50&format=jpg&mode=pad"
    for name in ("alpha", "jpeg"):
        data = source(name)[0]
        got = run(querystring_job(qs), data)
        assert got == run(explicit_job(qs, name, preset={"libjpeg_turbo": {"quality": 90}}), data)
        im = np.asarray(PIL.open(io.BytesIO(got)).convert("RGB"))
        assert im.shape == (50, 50, 3) and im[0, 25].min() >= 250 and im[49, 25].min() >= 250


def test_two_sides_without_a_mode_give_the_padded_canvas():
    rows, w, h, alpha = unpack_raw_bgra(run(querystring_job("width=80&height=80"), source("alpha")[0]))
    assert (w, h) == (80, 80) and alpha                          # 97x61 -> 80x50, 15 rows of transparent padding above and below
    px = rows[:, :320].reshape(80, 80, 4)
    assert not px[:15].any() and not px[65:].any() and px[15:65, :, 3].any()
    assert unpack_raw_bgra(run(querystring_job("width=80&height=80&mode=max"), source("alpha")[0]))[1:3] == (80, 50)


def test_preshrink_follows_the_crop():
    data, w, h = source("jpeg")
    qs = "w=100&h=100&mode=crop"
    commands = riapi.expand_text(qs, w, h)["decoder_commands"]
    assert commands[0]["jpeg_downscale_hints"]["width"] == 336 and decoded_size(w, h, commands) == (400, 250)           # 5/8; the whole frame's ratio would pick less
    assert unpack_raw_bgra(run([{"decode": {"io_id": 0, "commands": commands}}, {"encode": {"io_id": 1, "preset": RAW}}], data))[1:3] == (400, 250)
    got = run(querystring_job(qs), data)
    assert got == run(explicit_job(qs, "jpeg"), data) and unpack_raw_bgra(got)[1:3] == (100, 100)
    # a larger ratio: no pre-shrink at 4 / 4, the full-size decode -- other bytes
    qs4 = qs + "&decoder.min_precise_scaling_ratio=4"
    assert riapi.expand_text(qs4, w, h)["decoder_commands"] == []
    full = run(querystring_job(qs4), data)
    assert full == run(explicit_job(qs4, "jpeg"), data) and full != got
    # ignoreicc=true: a Display-P3-tagged copy goes through with the untagged file's bytes; without the key it is refused
    from tests.test_jpeg_headers import P3_XYZ, icc_app2, make_icc
    p3 = data[:2] + icc_app2(make_icc(xyz=P3_XYZ)) + data[2:]
    assert "ICC profile" in run(querystring_job(qs), p3, expect=400)["message"]
    assert run(querystring_job(qs + "&ignoreicc=true"), p3) == got


def test_red_dot():
    data, w, h = source("big")
    qs = "w=70&h=70&mode=max&rotate=90"
    rows, ow, oh, alpha = unpack_raw_bgra(run(querystring_job(qs + "&watermark_red_dot=true"), data))
    plain, pw, ph, palpha = unpack_raw_bgra(run(querystring_job(qs), data))
    assert (ow, oh) == (pw, ph) == (53, 70)
    a, b = rows[:, :4 * ow].reshape(oh, ow, 4).copy(), plain[:, :4 * pw].reshape(ph, pw, 4).copy()
    assert (a[-3:, -3:] == (0, 0, 255, 255)).all()
    a[-3:, -3:] = b[-3:, -3:] = 0
    assert np.array_equal(a, b)
    # the node as a step does the same; on a 3x3 frame it does nothing
    small = pack_raw_bgra(np.full((5, 32), 77, np.uint8), 8, 5, alpha_meaningful=False)
    px = unpack_raw_bgra(run([{"decode": {"io_id": 0}}, "watermark_red_dot", {"encode": {"io_id": 1, "preset": RAW}}], small))[0][:, :32].reshape(5, 8, 4).copy()
    same = unpack_raw_bgra(run([{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": RAW}}], small))[0][:, :32].reshape(5, 8, 4).copy()
    assert (px[-3:, -3:] == (0, 0, 255, 255)).all()
    px[-3:, -3:] = same[-3:, -3:] = 0
    assert np.array_equal(px, same)
    tiny = pack_raw_bgra(np.full((3, 12), 77, np.uint8), 3, 3, alpha_meaningful=False)
    assert run([{"decode": {"io_id": 0}}, "watermark_red_dot", {"encode": {"io_id": 1, "preset": RAW}}], tiny) == run(
        [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": RAW}}], tiny)


def test_watermarks_go_before_and_behind_the_padding():
    mark = pack_raw_bgra(np.tile(np.array([10, 200, 250, 255], np.uint8), (12, 20)), 20, 12, alpha_meaningful=True)
    marks = [{"io_id": 2, "fit_box": {"image_percentage": {"x1": 10, "y1": 10, "x2": 60, "y2": 90}}, "opacity": 0.8},
             {"io_id": 3, "fit_box": {"canvas_margins": {"left": 2, "top": 3, "right": 40, "bottom": 60}}, "gravity": {"percentage": {"x": 0, "y": 0}}}]
    qs = "width=80&height=80"
    job = explicit_job(qs, "alpha", watermarks=marks)
    assert [next(iter(s)) for s in job] == ["decode", "resample_2d", "watermark", "expand_canvas", "watermark", "encode"]
    assert job[2]["watermark"]["io_id"] == 2 and job[4]["watermark"]["io_id"] == 3
    data = source("alpha")[0]
    got = run(querystring_job(qs, marks), data, marks=[mark, mark])
    assert got == run(job, data, marks=[mark, mark])
    assert got != run(querystring_job(qs), data)
    px = unpack_raw_bgra(got)[0][:, :320].reshape(80, 80, 4)
    assert px[3:10, 2:10, 3].min() == 255                       # the canvas mark sits in the padding, where the image mark cannot reach
