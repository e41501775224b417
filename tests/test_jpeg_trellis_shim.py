"""The shim's handling of the `mozjpeg` preset without a device: which coder `encode` hands it to (ifhip_encode_preset_coder
is the function `encode` itself dispatches on), that every other preset goes where it went, the preset's quality (an
Option<u8>), and that a job gets as far as needing the device and never writes the raw container."""
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context  # noqa: E402
from tests.test_webp_shim_presets import JPEG, PNG, PNGQUANT, RAW, WEBP_LOSSLESS, coder  # noqa: E402

MOZJPEG = 5                                                     # include/imageflow_hip.h IFHIP_ENCODE_CODER_MOZJPEG


@pytest.mark.parametrize("preset", [{"mozjpeg": {}}, {"mozjpeg": {"quality": 90, "progressive": False}}])
def test_the_mozjpeg_preset_reaches_its_coder(preset):
    assert coder(preset) == MOZJPEG


def test_every_other_preset_goes_where_it_went():
    assert coder("webplossless") == WEBP_LOSSLESS
    for preset in ["webplossy", {"webplossy": {"quality": 80.0}}, {"webplossy": {}}, {"webplossless": {}}, "WebPLossless", "webp", "gif",
                   {"lodepng": {"maximum_deflate": False}}, None, ["webplossless"], "mozjpeg", ["mozjpeg"]]:
        assert coder(preset) == RAW, preset
    assert coder({"libjpeg_turbo": {"quality": 85}}) == JPEG
    assert coder({"libpng": {}}) == PNG and coder({"pngquant": {"quality": 80}}) == PNGQUANT


def job(preset):
    return {"framewise": {"steps": [{"create_canvas": {"w": 8, "h": 8, "format": "bgra_32", "color": "transparent"}},
                                    {"encode": {"io_id": 1, "preset": preset}}]}}


@pytest.mark.parametrize("quality", [300, 1.5, -1])
def test_quality_is_an_option_u8(quality):
    with Context() as c:
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", job({"mozjpeg": {"quality": quality}}))
        assert status == 400 and r["success"] is False and "InvalidJson" in r["message"] and "mozjpeg.quality" in r["message"], r
        assert c.get_output_buffer(1) == b""


def test_a_mozjpeg_job_needs_the_device_and_writes_no_container():
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_mozjpeg_preset.py runs the job")
    with Context() as c:
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", job({"mozjpeg": {"quality": 80}}))
        assert status == 500 and r["success"] is False and "Gpu" in r["message"], r
        assert c.get_output_buffer(1) == b""
