"""Colour management in the ABI shim without a device: the context switch exists, v1/tell_decoder takes the new command, and a
job that would convert gets as far as needing the device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context  # noqa: E402
from tests import png_decode_oracle as O  # noqa: E402
from tests.test_jpeg_headers import P3_XYZ, make_icc  # noqa: E402


def p3_png():
    import zlib
    s = O.random_samples(np.random.default_rng(4), 9, 5, 6, 8, smooth=True)
    return O.write_png(s, 6, 8, ancillary=O.chunk(b"iCCP", b"Display P3\0\0" + zlib.compress(make_icc(xyz=P3_XYZ))))


def test_the_context_switch_exists_and_answers_true():
    with Context() as c:
        assert c.set_color_management(True) is True
        assert c.set_color_management(False) is True
        assert not c.has_error()
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "ifhip_shim_context_set_color_management(struct imageflow_context *context, int on)" in open(os.path.join(root, "include", "imageflow_abi_subset.h")).read()


def test_tell_decoder_accepts_the_commands():
    with Context() as c:
        c.add_input_buffer(0, p3_png())
        for command in ("convert_color_profile", "ignore_color_profile_errors", "discard_color_profile"):
            status, r = c.send_json("v1/tell_decoder", {"io_id": 0, "command": command})
            assert status == 200 and r["success"] is True, (command, r)
        status, r = c.send_json("v1/tell_decoder", {"io_id": 0, "command": "convert_colour_profile"})       # not a command
        assert status == 400 and "unknown decoder command" in r["message"]


@pytest.mark.parametrize("how", ["switch", "command", "tell"])
def test_a_job_that_would_convert_needs_the_device(how):
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_color_management_jobs.py runs the job")
    with Context() as c:
        c.add_input_buffer(0, p3_png())
        c.add_output_buffer(1)
        if how == "switch":
            assert c.set_color_management(True)
        if how == "tell":
            assert c.send_json("v1/tell_decoder", {"io_id": 0, "command": "convert_color_profile"})[0] == 200
        decode = {"io_id": 0, "commands": ["convert_color_profile"]} if how == "command" else {"io_id": 0}
        status, r = c.send_json("v1/execute", {"framewise": {"steps": [{"decode": decode}, {"encode": {"io_id": 1, "preset": "gif"}}]}})
        assert status == 500 and r["success"] is False and "Gpu" in r["message"], r


def test_without_the_switch_the_refusal_stands_and_names_it():
    with Context() as c:
        c.add_input_buffer(0, p3_png())
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": "gif"}}]}})
        assert status == 400 and c.error_code() == 8, r
        for word in ("ICC profile", "discard_color_profile", "ifhip_shim_context_set_color_management", "convert_color_profile"):
            assert word in r["message"], (word, r["message"])
