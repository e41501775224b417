"""The `mozjpeg` encoder preset through the shim on the GPU (codecs/mozjpeg.rs:37-59): matte -> raw forward stage -> trellis
stage -> the device entropy coder with optimised tables and the progressive scan script.  The file's bytes are the host
writer's over the CPU emulation's planes (tests/jpeg_trellis_emulate.cpp) for the same flattened frame."""
import io

import numpy as np
import pytest
from PIL import Image

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra
from imageflow_amd.codecs.mozjpeg import write_jpeg
from oracle import oracle as O
from tests import jpeg_trellis_emu as E
from tests import util as U

pytestmark = pytest.mark.gpu


def run(c, message):
    status, r = c.send_json("v1/execute", message)
    assert status == 200 and r["success"], r
    return r


def rows_of(frame):
    h, w = frame.shape[:2]
    rows = np.zeros((h, U.stride_for(w)), np.uint8)
    rows[:, :4 * w] = frame.reshape(h, 4 * w)
    return rows


def expected_file(frame, quality):
    """frame: the flattened pixels, uint8 [h][w][4]"""
    h, w = frame.shape[:2]
    r = E.emulate(frame, E.quality_tables(quality))
    return write_jpeg(r["coef"], w, h, *E.S420, quality, progressive=True, optimize_coding=True)


def steps(preset):
    return {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": preset}}]}}


def graph(preset):
    return {"framewise": {"graph": {"nodes": {"0": {"decode": {"io_id": 0}}, "1": {"encode": {"io_id": 1, "preset": preset}}},
                                    "edges": [{"from": 0, "to": 1, "kind": "input"}]}}}


def is_progressive_jpeg(data, w, h):
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    assert b"\xff\xc2" in data[:700] and b"\xff\xc0" not in data[:700]      # SOF2, no baseline frame header
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (w, h) and im.format == "JPEG"
    return np.asarray(im.convert("RGB"))


@pytest.mark.parametrize("job", [steps, graph], ids=["steps", "graph"])
@pytest.mark.parametrize("size,params,quality", [((203, 131), {"quality": 80}, 80), ((17, 9), {}, 75), ((64, 48), {"quality": 200, "progressive": False}, 100)],
                         ids=["203x131_q80", "17x9_default", "64x48_q200"])
def test_decode_then_encode_mozjpeg(job, size, params, quality):
    w, h = size
    frame = E.frame("photo", w, h)
    with Context() as c:
        c.add_input_buffer(0, pack_raw_bgra(rows_of(frame), w, h, alpha_meaningful=False))
        c.add_output_buffer(1)
        r = run(c, job({"mozjpeg": params}))
        got = bytes(c.get_output_buffer(1))
        assert c.L.ifhip_shim_device_coded_files(c.p) == 1          # without ifhip_shim_context_set_device_jpeg_options
    enc = r["data"]["job_result"]["encodes"][0]
    assert (enc["preferred_mime_type"], enc["preferred_extension"], enc["w"], enc["h"]) == ("image/jpeg", "jpg", w, h)
    is_progressive_jpeg(got, w, h)
    assert got == expected_file(frame, quality)


@pytest.mark.parametrize("matte_json,matte32", [(None, 0xFFFFFFFF), ({"srgb": {"hex": "336699FF"}}, 0xFF336699)], ids=["white", "336699"])
def test_a_translucent_canvas_is_flattened_on_the_matte(matte_json, matte32):
    w, h = 40, 24
    params = {"quality": 85}
    if matte_json:
        params["matte"] = matte_json
    with Context() as c:
        c.add_output_buffer(1)
        run(c, {"framewise": {"steps": [{"create_canvas": {"w": w, "h": h, "format": "bgra_32", "color": {"srgb": {"hex": "FF000080"}}}},
                                        {"encode": {"io_id": 1, "preset": {"mozjpeg": params}}}]}})
        got = bytes(c.get_output_buffer(1))
    canvas = np.zeros((h, U.stride_for(w)), np.uint8)
    canvas[:, :4 * w] = np.tile(np.array([0, 0, 255, 0x80], np.uint8), (h, w))
    O.apply_matte(canvas, w, h, canvas.shape[1], matte32, True)
    flat = np.ascontiguousarray(canvas[:, :4 * w].reshape(h, w, 4))
    assert got == expected_file(flat, 85)
    rgb = is_progressive_jpeg(got, w, h)
    assert np.abs(rgb.astype(np.int32) - flat[..., 2::-1].astype(np.int32)).max() <= 3      # (one flat colour: the blend, not black)


def test_the_other_presets_of_the_same_job_are_what_they_were():
    """libjpeg_turbo beside mozjpeg: byte for byte libjpeg-turbo's file, as before; "gif" still gets the raw container"""
    w, h = 97, 61
    frame = E.frame("photo", w, h)
    rows = rows_of(frame)
    with Context() as c:
        c.add_input_buffer(0, pack_raw_bgra(rows, w, h, alpha_meaningful=False))
        for io_id in (1, 2, 3):
            c.add_output_buffer(io_id)
        run(c, {"framewise": {"graph": {
            "nodes": {"0": {"decode": {"io_id": 0}}, "1": {"encode": {"io_id": 1, "preset": {"mozjpeg": {"quality": 85}}}},
                      "2": {"encode": {"io_id": 2, "preset": {"libjpeg_turbo": {"quality": 85}}}}, "3": {"encode": {"io_id": 3, "preset": "gif"}}},
            "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 0, "to": 2, "kind": "input"}, {"from": 0, "to": 3, "kind": "input"}]}}})
        moz, classic, raw = (bytes(c.get_output_buffer(i)) for i in (1, 2, 3))
        assert c.L.ifhip_shim_device_coded_files(c.p) == 2
    assert moz == expected_file(frame, 85)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[..., 2::-1])).save(buf, "JPEG", quality=85, subsampling="4:2:0", optimize=False)
    assert classic == buf.getvalue()
    got_rows, gw, gh, _ = unpack_raw_bgra(raw)
    assert (gw, gh) == (w, h) and np.array_equal(got_rows[:, :4 * w], rows[:, :4 * w])


@pytest.mark.parametrize("quality", [300, 1.5])
def test_a_quality_that_is_no_u8_is_invalid_json(quality):
    with Context() as c:
        c.add_input_buffer(0, pack_raw_bgra(rows_of(E.frame("photo", 17, 9)), 17, 9, alpha_meaningful=False))
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", steps({"mozjpeg": {"quality": quality}}))
        assert status == 400 and "InvalidJson" in r["message"], r
        assert c.get_output_buffer(1) == b""
