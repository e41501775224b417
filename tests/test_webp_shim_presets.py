"""The shim's handling of the WebP presets without a device: which coder `encode` hands a preset to
(ifhip_encode_preset_coder is the function `encode` itself dispatches on), that a `"webplossless"` job gets as far as
needing the device and never writes the raw container, and that the querystring's format=webp stays refused."""
import ctypes as C
import json

import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd.abi import Context  # noqa: E402

RAW, JPEG, PNG, PNGQUANT, WEBP_LOSSLESS = 0, 1, 2, 3, 4       # include/imageflow_hip.h IFHIP_ENCODE_CODER_*


def coder(preset):
    L = _native.lib()
    L.ifhip_encode_preset_coder.argtypes = [C.c_char_p, C.c_size_t]
    L.ifhip_encode_preset_coder.restype = C.c_int
    text = json.dumps(preset).encode()
    return L.ifhip_encode_preset_coder(text, len(text))


def test_the_string_preset_webplossless_reaches_the_webp_coder():
    assert coder("webplossless") == WEBP_LOSSLESS


@pytest.mark.parametrize("preset", ["webplossy", {"webplossy": {"quality": 80.0}}, {"webplossy": {}}, {"webplossless": {}}, "WebPLossless", "webp",
                                    "gif", {"lodepng": {"maximum_deflate": False}}, None, ["webplossless"]])
def test_every_other_webp_form_keeps_the_raw_container(preset):
    assert coder(preset) == RAW


def test_the_other_coders_are_chosen_as_before():
    assert coder({"libjpeg_turbo": {"quality": 85}}) == JPEG
    assert coder({"libpng": {}}) == PNG and coder({"pngquant": {"quality": 80}}) == PNGQUANT
    L = _native.lib()
    L.ifhip_encode_preset_coder.argtypes = [C.c_char_p, C.c_size_t]
    assert L.ifhip_encode_preset_coder(b"{\"libpng\": ", 11) == -1 and L.ifhip_encode_preset_coder(None, 0) == -1


def test_a_webplossless_job_needs_the_device_and_writes_no_container():
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_webp_encode.py runs the job")
    with Context() as c:
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": [
            {"create_canvas": {"w": 8, "h": 8, "format": "bgra_32", "color": "transparent"}}, {"encode": {"io_id": 1, "preset": "webplossless"}}]}})
        assert status == 500 and r["success"] is False and "Gpu" in r["message"], r
        assert c.get_output_buffer(1) == b""


def test_querystring_format_webp_stays_refused():
    for fmt in ("webp", "png"):
        with Context() as c:
            c.add_input_buffer(0, b"\xff\xd8\xff" + bytes(64))
            c.add_output_buffer(1)
            status, r = c.send_json("v1/execute", {"framewise": {"steps": [
                {"command_string": {"kind": "ir4", "value": "width=100&format=" + fmt, "decode": 0, "encode": 1}}]}})
            assert status == 400 and "ActionNotSupported" in r["message"] and "format=" + fmt in r["message"], r
