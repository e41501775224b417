"""The device palette coder on an MI355X (csrc/png_quantize.hip through imageflow_amd.codecs.pngquant and the `pngquant`
preset of `encode`): palettes, counts, index planes and whole files equal the CPU emulation's (tests/png_quantize_emulate.cpp,
the same core header) byte for byte, at the shapes where the remap's skewed wavefront can go wrong; a batch gives every
frame the bytes it gets alone; an image that misses minimum_quality is dropped alone; and the preset writes palette files
that Pillow and this library's own decoder read, with the lossless fall-back of the reference."""
import ctypes as C
import io
import json
import struct

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import pngquant as Q  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import png_oracle as P  # noqa: E402
from tests import png_quantize_emu as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 1x1; no right neighbour / no row below; fewer columns than twice a wave's lanes and more rows than a wave; wider; more
# rows than the workgroup has lanes (the roll-over to row r + 1024 and the last lane's error row in LDS)
SHAPES = [(1, 1), (1, 200), (200, 1), (70, 130), (300, 70), (257, 1100)]


def bitmap(frames, w, h, alpha=True):
    frames = np.ascontiguousarray(frames)
    return Bitmap.from_numpy(frames, w, h, frames.shape[-1], DEV, alpha_meaningful=alpha)


def device(rgba_frames, alpha, stride=None, **kw):
    """The device's answer for a batch of RGBA frames: (files, status, taps)."""
    h, w, _ = rgba_frames[0].shape
    rows = np.stack([E.bgra_rows(f, stride) for f in rgba_frames])
    stage = Q.PngQuantStage(w, h, len(rgba_frames), DEV)
    return stage.quantize(bitmap(rows, w, h, alpha), taps=True, **kw)


def assert_equals_emulation(rgba, alpha, got_file, got_status, got_tap, **kw):
    want = E.quantize(rgba, alpha=alpha, **kw)
    palette, indices, mse = got_tap
    assert got_status == want["status"]
    assert np.array_equal(palette, want["palette"]), "palette and count"
    assert np.array_equal(indices, want["indices"]), "index plane"
    assert got_file == want["file"], "the complete file"
    assert abs(mse - want["mse"]) <= 1e-12 * max(1.0, want["mse"])
    return want


@pytest.mark.parametrize("dither", [False, True], ids=["plain", "dither"])
@pytest.mark.parametrize("alpha", [False, True], ids=["opaque", "alpha"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_emulation(shape, alpha, dither):
    w, h = shape
    rgba = E.photo_rgba(w, h, seed=3, alpha=alpha)
    files, status, taps = device([rgba], alpha, stride=4 * w + 8, dither=dither)
    want = assert_equals_emulation(rgba, alpha, files[0], status[0], taps[0], dither=dither, stride=4 * w + 8)
    assert status[0] == 0
    E.check_palette_file(files[0], w, h, want["palette"], want["indices"])
    assert int(taps[0][1].max()) < len(taps[0][0])


def test_a_frame_of_256_colours_is_kept_exactly():
    w, h = 64, 48
    for alpha in (False, True):
        rgba = E.colour_frame(w, h, 255 if alpha else 256, seed=5, alpha=alpha)
        if alpha:
            rgba[:3, :5] = (9, 8, 7, 0)                                 # transparent pixels with a colour: the 256th value, 00 00 00 00
        files, status, taps = device([rgba], alpha, minimum_quality=100)
        assert status == [0]
        palette, indices, mse = taps[0]
        assert mse == 0.0
        assert np.array_equal(palette[indices], E.normalized(rgba, alpha)), "dithering changes nothing"
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[0])).convert("RGBA")), E.normalized(rgba, alpha))


def test_a_batch_gives_every_frame_the_bytes_it_gets_alone_on_every_run():
    w, h = 120, 90
    frames = [E.photo_rgba(w, h, seed=11, alpha=True), E.colour_frame(w, h, 200, seed=2, alpha=True), E.photo_rgba(w, h, seed=12, alpha=True),
              np.zeros((h, w, 4), np.uint8)]
    files, status, taps = device(frames, True)
    assert status == [0, 0, 0, 0]
    for i, f in enumerate(frames):
        one, st, tap = device([f], True)
        assert one[0] == files[i] and np.array_equal(tap[0][1], taps[i][1])
    again, _, _ = device(frames, True)
    assert again == files
    assert_equals_emulation(frames[0], True, files[0], status[0], taps[0])


def test_an_image_below_minimum_quality_is_dropped_alone():
    w, h = 120, 90
    frames = [E.colour_frame(w, h, 200, seed=2), E.photo_rgba(w, h, seed=11), E.colour_frame(w, h, 17, seed=3)]
    files, status, _ = device(frames, False, minimum_quality=100)
    assert status == [0, Q.PNG_QUALITY_TOO_LOW, 0] and files[1] is None
    for i in (0, 2):
        assert files[i] == device([frames[i]], False)[0][0], "the neighbours' files are unchanged"


def test_the_host_buffer_form_equals_the_device_form():
    w, h, stride = 37, 23, 4 * 37 + 8
    rgba = E.photo_rgba(w, h, seed=4, alpha=True)
    host, status = Q.quantize_png_host(E.bgra_rows(rgba, stride), w, h, stride, True)
    assert status == 0 and host == device([rgba], True, stride=stride)[0][0]
    none, status = Q.quantize_png_host(E.bgra_rows(rgba, stride), w, h, stride, True, minimum_quality=100)
    assert none is None and status == Q.PNG_QUALITY_TOO_LOW


def test_guard_regions_and_file_overflow():
    """Where the zlib body lands and what a pitch below the file does, on a stream of two deflate chunks (201 x 170 bytes):
    nothing outside a file's own bytes is written, and a file that does not fit its pitch is dropped with the status word."""
    w, h, n = 200, 170, 3
    frames = [E.photo_rgba(w, h, seed=21 + i) for i in range(n)]
    alone = [device([f], False)[0][0] for f in frames]
    frames_dev = bitmap(np.stack([E.bgra_rows(f) for f in frames]), w, h, False)
    stage = Q.PngQuantStage(w, h, n, DEV)
    L, guard = Q._bind(), 4096

    def run(pitch):
        files = torch.full((n * pitch + guard,), 0x5C, dtype=torch.uint8, device=DEV)
        lengths = torch.full((n + 64,), -7, dtype=torch.int32, device=DEV)
        status = torch.full((n + 64,), -9, dtype=torch.int32, device=DEV)
        with torch.cuda.device(DEV):
            assert L.ifhip_png_quantize_batch_device(stage._h, frames_dev.data.data_ptr(), frames_dev.image_bytes, frames_dev.stride, 0, n, -1, -1, -1,
                                                     Q.MAX_COLORS, 1, Q.DEFAULT_ZLIB_LEVEL, files.data_ptr(), pitch, lengths.data_ptr(), status.data_ptr(),
                                                     None, None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            torch.cuda.synchronize()
        assert bool((lengths[n:] == -7).all()) and bool((status[n:] == -9).all()), "the unused length / status words"
        return files.cpu().numpy(), lengths[:n].cpu().tolist(), status[:n].cpu().tolist()

    pitch = (stage.max_file_bytes + 15) // 16 * 16
    host, ln, st = run(pitch)
    assert st == [0] * n
    assert (host[n * pitch:] == 0x5C).all(), "nothing behind the last pitch is touched"
    for i in range(n):
        assert 0 < ln[i] <= stage.max_file_bytes
        assert host[i * pitch:i * pitch + ln[i]].tobytes() == alone[i], "the file the frame gets alone"
        assert (host[i * pitch + ln[i]:(i + 1) * pitch] == 0x5C).all(), "nothing behind a file's end is touched"
    # a pitch below the files (and above the entry's minimum, which is an argument error): every image is dropped with the
    # status word, nothing is written
    small = 2048
    assert all(len(f) > small for f in alone)
    host, ln, st = run(small)
    assert ln == [0] * n and st == [Q.PNG_FILE_OVERFLOW] * n
    assert (host == 0x5C).all()


# ---- the `pngquant` preset of `encode` (csrc/abi_shim.cpp) ----------------------------------------------------------------------

def _run(ctx, job, expect=200):
    status, r = ctx.send_json("v1/execute", job)
    assert status == expect, (status, r, ctx.error_message())
    return r


def _jpeg_input(w=160, h=100):
    b = io.BytesIO()
    Image.fromarray(P.photo_frame(w, h, 9)).save(b, "JPEG", quality=85)
    return b.getvalue()


def _encode(data, preset, steps=None, graph=False):
    """(file, response entry) of decode -> encode with `preset`, as steps or as a graph."""
    with Context() as c:
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        if graph:
            job = {"framewise": {"graph": {"nodes": {"0": {"decode": {"io_id": 0}}, "1": {"encode": {"io_id": 1, "preset": preset}}},
                                           "edges": [{"from": 0, "to": 1, "kind": "input"}]}}}
        else:
            job = {"framewise": {"steps": (steps or [{"decode": {"io_id": 0}}]) + [{"encode": {"io_id": 1, "preset": preset}}]}}
        r = _run(c, job)
        return bytes(c.get_output_buffer(1)), r["data"]["job_result"]["encodes"][0]


def _source_rgba(data):
    """The decoded frame as the raw tap of the `lodepng` preset returns it: (RGBA [h, w, 4], alpha_meaningful)."""
    raw, _ = _encode(data, {"lodepng": {}})
    assert raw[:7] == b"IFBGRA1"
    rows, w, h, alpha = unpack_raw_bgra(raw)
    return np.ascontiguousarray(np.ascontiguousarray(rows)[:, :4 * w].reshape(h, w, 4)[..., [2, 1, 0, 3]]), alpha


def _color_type(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">IIBB", data[16:26])[3]


def test_the_preset_writes_a_palette_png_that_pillow_and_this_decoder_read():
    data = _jpeg_input()
    got, enc = _encode(data, {"pngquant": {"quality": 100}})
    assert got[:8] == b"\x89PNG\r\n\x1a\n", got[:8]
    assert _color_type(got) == 3
    assert (enc["preferred_mime_type"], enc["preferred_extension"], enc["w"], enc["h"]) == ("image/png", "png", 160, 100)
    kinds = [k for k, _ in E.chunks(got)]
    assert kinds == [b"IHDR", b"PLTE", b"IDAT", b"IEND"], kinds
    im = Image.open(io.BytesIO(got))
    assert im.mode == "P" and im.size == (160, 100)
    seen = np.asarray(im.convert("RGBA"))
    src, alpha = _source_rgba(data)
    assert not alpha
    assert ((seen[..., :3].astype(np.float64) - src[..., :3]) ** 2).sum(-1).mean() < 3 * 40.0 ** 2, "the picture, not noise"
    again, alpha2 = _source_rgba(got)                                   # this library's own decoder, in a second job
    assert np.array_equal(again[..., :3], seen[..., :3])
    graph, _ = _encode(data, {"pngquant": {"quality": 100}}, graph=True)
    assert graph == got, "steps and the graph form give the same bytes"
    # the same frame through the mirror's stage: the preset passes 256 colours, dithering and zlib level 6
    want = E.quantize(E.normalized(src, False), alpha=False)
    assert got == want["file"]


def test_quality_too_low_falls_back_to_a_lossless_file():
    data = _jpeg_input()
    src, _ = _source_rgba(data)
    got, enc = _encode(data, {"pngquant": {"minimum_quality": 100}})
    assert _color_type(got) == 2 and enc["preferred_mime_type"] == "image/png" and enc["preferred_extension"] == "png"
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got))), src[..., :3])
    rgba = E.photo_rgba(96, 64, seed=5, alpha=True)
    canvas = pack_raw_bgra(np.ascontiguousarray(E.bgra_rows(rgba)), 96, 64, alpha_meaningful=True)
    got, _ = _encode(canvas, {"pngquant": {"minimum_quality": 100}})
    assert _color_type(got) == 6
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got))), rgba)


def test_a_200_colour_canvas_decodes_exactly():
    rgba = E.colour_frame(80, 60, 200, seed=8, alpha=True)
    canvas = pack_raw_bgra(np.ascontiguousarray(E.bgra_rows(rgba)), 80, 60, alpha_meaningful=True)
    got, _ = _encode(canvas, {"pngquant": {}})
    assert _color_type(got) == 3
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got)).convert("RGBA")), E.normalized(rgba))
    deflated, _ = _encode(canvas, {"pngquant": {"maximum_deflate": True}})
    a, b = dict(E.chunks(got))[b"IDAT"], dict(E.chunks(deflated))[b"IDAT"]
    assert a[2:] == b[2:] and a[:2] != b[:2], "maximum_deflate changes the FLEVEL bits only"


@pytest.mark.parametrize("opts", [{"speed": 2.5}, {"quality": 256}, {"minimum_quality": -1}, {"speed": "fast"}, {"maximum_deflate": 1}],
                         ids=lambda o: json.dumps(o))
def test_malformed_options_are_invalid_json(opts):
    with Context() as c:
        c.add_input_buffer(0, _jpeg_input())
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": {"pngquant": opts}}}]}})
        assert status != 200 and "InvalidJson" in r["message"]
