"""The device GIF coder on an MI355X (csrc/gif_encode.hip through imageflow_amd.codecs.gif_encoder and, with the context's
switch on, the "gif" preset of `encode`): palettes, index planes and whole files equal the CPU emulation's
(tests/gif_encode_emulate.cpp, the same core header) byte for byte, on the smallest frames at which the kernels can go
wrong; a batch on a side stream gives every frame the bytes it gets alone; and the jobs write files that Pillow and this
library's own GIF decoder read back to the emulation's pixels.  There is no tolerance anywhere."""
import io

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import gif_encoder as GIF  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import gif_encode_emu as G  # noqa: E402
from tests import gif_gen  # noqa: E402
from tests import png_decode_oracle as PO  # noqa: E402
from tests import png_quantize_emu as Q  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = G.cases()


def bitmap(frames, w, h, alpha=True):
    frames = np.ascontiguousarray(frames)
    return Bitmap.from_numpy(frames, w, h, frames.shape[-1], DEV, alpha_meaningful=alpha)


def device(rgba_frames, alpha, stride=None, **kw):
    """The device's answer for a batch of RGBA frames of one size: (files, status, palettes, indices)."""
    h, w, _ = rgba_frames[0].shape
    rows = np.stack([Q.bgra_rows(f, stride) for f in rgba_frames])
    stage = GIF.GifEncodeStage(w, h, len(rgba_frames), DEV)
    return stage.encode(bitmap(rows, w, h, alpha), taps=True, **kw)


def assert_equals_emulation(rgba, alpha, got, stride=None, **kw):
    files, status, palettes, indices = got
    want = G.encode(rgba, alpha=alpha, stride=stride, **kw)
    assert status[0] == want["status"] == 0
    assert np.array_equal(palettes[0], want["palette"]), "palette and count"
    assert np.array_equal(indices[0], want["indices"]), "index plane"
    assert files[0] == want["file"], "the complete file"
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_emulation(name):
    rgba, alpha = CASES[name]
    assert_equals_emulation(rgba, alpha, device([rgba], alpha))


@pytest.mark.parametrize("residue", [0, 1, 254])
def test_data_lengths_at_the_sub_block_boundaries(residue):
    rgba = G.modulo_frames()[residue]
    want = assert_equals_emulation(rgba, False, device([rgba], False))
    assert want["data_bytes"] % 255 == residue


def test_a_stride_with_padding_and_the_head_fields():
    rgba, alpha = CASES["photo_alpha_70x50"]
    stride = 4 * 70 + 24
    assert_equals_emulation(rgba, alpha, device([rgba], alpha, stride=stride), stride=stride)
    assert_equals_emulation(rgba, alpha, device([rgba], alpha, repeat=3, delay=7, needs_user_input=True), repeat=3, delay=7, user_input=True)


def test_a_batch_of_8_on_a_side_stream_gives_every_frame_the_bytes_it_gets_alone():
    w, h = 150, 130                                                       # two segments each
    frames = [Q.photo_rgba(w, h, seed=7, alpha=True), G.noise_frame(w, h, 256, seed=5), Q.colour_frame(w, h, 200, seed=2), np.zeros((h, w, 4), np.uint8),
              Q.photo_rgba(w, h, seed=12, alpha=True), G.noise_frame(w, h, 2, seed=6), Q.colour_frame(w, h, 257, seed=3), Q.photo_rgba(w, h, seed=13)]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        files, status, palettes, indices = device(frames, True)
    side.synchronize()
    assert status == [0] * 8
    for i, f in enumerate(frames):
        one = device([f], True)
        assert one[0][0] == files[i] and np.array_equal(one[3][0], indices[i]) and np.array_equal(one[2][0], palettes[i]), i
    assert_equals_emulation(frames[0], True, ([files[0]], [status[0]], [palettes[0]], [indices[0]]))
    assert_equals_emulation(frames[1], True, ([files[1]], [status[1]], [palettes[1]], [indices[1]]))


def test_the_host_buffer_form_and_a_pitch_below_the_file():
    rgba, _ = CASES["photo_17x40"]
    stride = 4 * 17 + 8
    want = G.encode(rgba, alpha=False)
    assert GIF.encode_gif_host(Q.bgra_rows(rgba, stride), 17, 40, stride, False) == want["file"]
    flat = np.full((40, 17, 4), (9, 8, 7, 255), np.uint8)                   # a file far below the photo's
    three = [flat, rgba, flat[:, :, [2, 1, 0, 3]].copy()]
    alone = [G.encode(f, alpha=False)["file"] for f in three]
    pitch = 1000
    assert len(alone[0]) < pitch < len(alone[1])
    stage = GIF.GifEncodeStage(17, 40, 3, DEV)
    files, status = stage.encode(bitmap(np.stack([Q.bgra_rows(f) for f in three]), 17, 40, False), file_pitch=pitch)
    assert status == [0, GIF.GIF_FILE_OVERFLOW, 0] and files[1] is None
    assert files[0] == alone[0] and files[2] == alone[2], "the neighbours' files are unchanged"


# ---- jobs (csrc/abi_shim.cpp), with the context's switch on ---------------------------------------------------------------------------

def run(msg, inputs, outputs, gif=True, expect=200):
    with Context() as c:
        assert c.set_gif_encoder(gif) is True
        for io_id, data in inputs.items():
            c.add_input_buffer(io_id, data)
        for io_id in outputs:
            c.add_output_buffer(io_id)
        status, r = c.send_json("v1/execute", msg)
        assert status == expect, (status, r)
        if expect != 200:
            return c.error_code(), r
        return {o: bytes(c.get_output_buffer(o)) for o in outputs}, r


def steps(*nodes):
    return {"framewise": {"steps": list(nodes)}}


GIF_OUT = {"encode": {"io_id": 1, "preset": "gif"}}


def rgba_of_raw(raw):
    rows, w, h, alpha = unpack_raw_bgra(raw)
    return np.ascontiguousarray(rows[:, :4 * w].reshape(h, w, 4)[..., [2, 1, 0, 3]]), alpha


def sources():
    with_alpha = Q.photo_rgba(90, 60, seed=21, alpha=True)
    jpeg = io.BytesIO()
    Image.fromarray(Q.photo_rgba(101, 67, seed=22)[..., :3].copy(), "RGB").save(jpeg, "JPEG", quality=85)
    png = io.BytesIO()
    Image.fromarray(Q.photo_rgba(64, 50, seed=23, alpha=True), "RGBA").save(png, "PNG")
    opaque = Q.photo_rgba(40, 30, seed=24)
    opaque[..., 3] = 3                                                     # bgr_32: the alpha bytes mean nothing
    return {"raw": pack_raw_bgra(Q.bgra_rows(with_alpha, 4 * 90), 90, 60, alpha_meaningful=True), "jpeg": jpeg.getvalue(), "png": png.getvalue(),
            "bgr_32": pack_raw_bgra(Q.bgra_rows(opaque, 4 * 40), 40, 30, alpha_meaningful=False)}


@pytest.mark.parametrize("source", ["raw", "jpeg", "png", "bgr_32"])
def test_steps_decode_then_encode_gif(source):
    data = sources()[source]
    job = steps({"decode": {"io_id": 0}}, GIF_OUT)
    outs, r = run(job, {0: data}, [1])
    tap, _ = run(job, {0: data}, [1], gif=False)
    assert tap[1][:7] == b"IFBGRA1", "off, the preset stays the raw container"
    rgba, alpha = rgba_of_raw(tap[1])
    want = G.encode(rgba, alpha=alpha)
    assert outs[1] == want["file"], "the job's file is the emulation's of the job's frame"
    entry = r["data"]["job_result"]["encodes"][0]
    assert (entry["preferred_mime_type"], entry["preferred_extension"], entry["w"], entry["h"]) == ("image/gif", "gif", rgba.shape[1], rgba.shape[0])
    pixels = G.decoded(want)
    got, _, info = G.pillow_rgba(outs[1])
    assert np.array_equal(got, pixels) and "loop" not in info
    if source == "bgr_32":
        assert want["n_trans"] == 0 and (pixels[..., 3] == 255).all(), "a bgr_32 frame is coded without a transparent entry"
    if source in ("raw", "png"):
        assert want["n_trans"] == 1
    # this project's own decoder, on a context with the switch off
    back, r2 = run(steps({"decode": {"io_id": 0}}, GIF_OUT), {0: outs[1]}, [1], gif=False)
    again, alpha2 = rgba_of_raw(back[1])
    assert alpha2 and np.array_equal(again, pixels)
    assert r2["data"]["job_result"]["decodes"][0]["preferred_mime_type"] == "image/gif"


def test_a_graph_with_a_second_encode_leaves_the_shared_frame_alone():
    data = sources()["raw"]
    job = {"framewise": {"graph": {
        "nodes": {"0": {"decode": {"io_id": 0}}, "1": GIF_OUT, "2": {"encode": {"io_id": 2, "preset": {"libpng": {}}}}},
        "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 0, "to": 2, "kind": "input"}]}}}
    outs, r = run(job, {0: data}, [1, 2])
    rgba, alpha = rgba_of_raw(data)
    want = G.encode(rgba, alpha=True)
    assert outs[1] == want["file"]
    png, info = PO.decode(outs[2])
    assert np.array_equal(png[..., [2, 1, 0, 3]], rgba), "the PNG holds the frame as it was decoded: semi-transparent pixels and all"
    kinds = {e["io_id"]: e["preferred_mime_type"] for e in r["data"]["job_result"]["encodes"]}
    assert kinds == {1: "image/gif", 2: "image/png"}


def test_a_gif_source_hands_its_loop_count_delay_and_user_input_flag_to_the_file():
    idx = gif_gen.runs(30, 20, 16, seed=3)
    pal = gif_gen.palette_of(16, seed=4)
    netscape = b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + (5).to_bytes(2, "little") + b"\x00"
    frames = [gif_gen.frame(idx, 30, 20, m=4, delay=7), gif_gen.frame(idx[::-1], 30, 20, m=4, delay=23, dispose=1)]
    marked = frames[1].replace(b"\x21\xF9\x04\x04", b"\x21\xF9\x04\x06", 1)        # the user-input flag
    assert marked != frames[1]
    src = gif_gen.gif(30, 20, [frames[0], marked], palette=pal, extensions=netscape)
    for select, delay, user in ((None, 7, 0), (1, 23, 2)):
        dec = {"decode": {"io_id": 0}} if select is None else {"decode": {"io_id": 0, "commands": [{"select_frame": select}]}}
        outs, _ = run(steps(dec, GIF_OUT), {0: src}, [1])
        got, _, info = G.pillow_rgba(outs[1])
        assert info["loop"] == 5 and info["duration"] == delay * 10
        at = outs[1].index(b"\x21\xf9\x04")
        assert outs[1][at + 3] & 2 == user
        want = pal[idx if select is None else idx[::-1]]
        assert np.array_equal(got[..., :3], want) and (got[..., 3] == 255).all()
    # a GIF without the block: the reference's decoder answers Infinite (codecs/gif/mod.rs:167-170)
    outs, _ = run(steps({"decode": {"io_id": 0}}, GIF_OUT), {0: gif_gen.gif(30, 20, [frames[0]], palette=pal)}, [1])
    assert G.pillow_rgba(outs[1])[2]["loop"] == 0


def test_a_canvas_wider_than_65535_is_an_invalid_argument():
    job = steps({"create_canvas": {"w": 70000, "h": 1, "format": "bgra_32", "color": "transparent"}}, GIF_OUT)
    job["security"] = {"max_frame_size": {"w": 100000, "h": 100000, "megapixels": 100}}
    code, r = run(job, {}, [1], expect=400)
    assert code == 2 and "InvalidArgument" in r["message"] and "65535" in r["message"]
