"""The C ABI of the device lossy WebP coder without a GPU: the header of its own declares the ifhip_webp_lossy_enc_* entries (and
says why it is apart), the bindings and the library carry them; every refused argument is refused in the words the other
file coders use, before the device check; the shim's switch is off by default, where the `webplossy` preset stays the raw
container -- with it on and no GPU a job answers a Gpu error and writes nothing, and the forms the reference's struct variant
does not deserialise are InvalidJson; the kernels stay out of scratch memory and hold what DESIGN 4.19 states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd import build as B  # noqa: E402
from imageflow_amd.abi import Context, pack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import webp_lossy_encoder as ENC  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from tests import test_encode_handoff as EH  # noqa: E402
from tests.test_kernel_resources import resource_usage, _int  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ifhip_webp_lossy_enc_stage_create", "ifhip_webp_lossy_enc_stage_destroy", "ifhip_webp_lossy_enc_stage_max_file_bytes",
           "ifhip_webp_lossy_encode_batch_device", "ifhip_webp_lossy_encode"]
KERNELS = {"vp8e_convert_kernel": 256, "vp8e_code_kernel": 512, "vp8e_count_kernel": 256, "vp8e_decide_kernel": 64, "vp8e_streams_kernel": 64,
           "vp8e_layout_kernel": 256}
INVALID = int(ErrorKind.InvalidArgument)
NO_GPU = (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
W, H, STRIDE = EH.W, EH.H, EH.STRIDE


def test_header_bindings_and_library_agree():
    main = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "imageflow_hip_webp_lossy_enc.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop_webp_lossy_enc.rs")).read()
    shim = open(os.path.join(ROOT, "include", "imageflow_abi_subset.h")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert name + "(" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S), name       # the main header's stream table is left alone
        assert re.search(r"IFHIP_API [^;]*\b%s\(" % name, extra), name
        assert re.search(r"\bpub fn %s\(" % name, bindings), name
        assert getattr(L, name) is not None
    assert re.search(r"IFHIP_API [^;]*\bifhip_webp_lossy_encode_batch_device\([^;]*float quality[^;]*void\* hip_stream\)", extra)
    assert "quality: f32" in bindings and "hip_stream: *mut c_void" in bindings
    assert '#include "imageflow_hip.h"' in extra and "stream" in extra.split("#ifndef")[0]
    for name in os.listdir(os.path.join(ROOT, "include")):
        assert not re.search(r'#include\s*"imageflow_hip_webp_lossy_enc\.h"', open(os.path.join(ROOT, "include", name)).read()), name      # included by nothing
    assert re.search(r"#define IFHIP_VP8_ENC_FILE_OVERFLOW 1\b", extra) and ENC.VP8_ENC_FILE_OVERFLOW == 1
    assert "kVp8eFileOverflow = 1;" in open(os.path.join(B.CSRC, "vp8_encode_core.hpp")).read()
    assert "ifhip_shim_context_set_webp_lossy_encoder" in shim and L.ifhip_shim_context_set_webp_lossy_encoder is not None
    for cite in ("WebPEncodeBGRA", "WebPEncodeBGR", "codecs/webp.rs"):
        assert cite in extra, cite


class Lossy:
    """the shape tests/test_encode_handoff.py's refusals() asks of a coder; the coder's own first refusal is its file_pitch"""
    own_text = b"InvalidArgument: file_pitch below 32 bytes"

    def __init__(self):
        self.L = ENC._bind()
        self.destroy_fn = self.L.ifhip_webp_lossy_enc_stage_destroy

    def stage(self, max_images=1):
        h = C.c_void_p()
        assert self.L.ifhip_webp_lossy_enc_stage_create(C.byref(h), W, H, 1, max_images) == 0      # (geometry only: the scratch comes with the first batch)
        return h

    def batch(self, stage, images=EH.P_IN, image_bytes=H * STRIDE, stride=STRIDE, n=1, files=EH.P_OUT, lengths=EH.P_LEN, own=False):
        pitch = 16 if own else (self.L.ifhip_webp_lossy_enc_stage_max_file_bytes(stage) + 15) // 16 * 16 if stage else 1 << 20
        rc = self.L.ifhip_webp_lossy_encode_batch_device(stage, images, image_bytes, stride, n, 75.0, files, pitch, lengths, None, None)
        return rc, self.L.ifhip_last_error_message()

    def host(self, bitmap=True, w=W, h=H, stride=STRIDE, length=True, status=None):
        frame, out, n = (C.c_uint8 * (H * STRIDE))(), (C.c_uint8 * 16)(), C.c_size_t(0)
        rc = self.L.ifhip_webp_lossy_encode(frame if bitmap else None, w, h, stride, 1, 75.0, out, 16, C.byref(n) if length else None)
        return rc, self.L.ifhip_last_error_message()


def test_every_refused_argument_is_refused_in_the_words_of_the_other_coders():
    """the made-up device pointers never reach a kernel: every call here fails a check on the host"""
    mine, theirs = EH.refusals(Lossy()), EH.refusals(EH.Coder("webp"))
    assert sorted(mine) == sorted(theirs)
    for case, ((rc, message), want) in mine.items():
        assert rc == INVALID, (case, rc)
        assert message == want and message == theirs[case][0][1], (case, message)


def test_stage_arguments_the_bound_and_the_coders_own_checks():
    c = Lossy()
    L, h = c.L, C.c_void_p()
    for args, words in (((0, 5, 1, 1), b"InvalidArgument: Bitmap dimensions cannot be zero"), ((5, 0, 1, 1), b"InvalidArgument: Bitmap dimensions cannot be zero"),
                        ((16384, 5, 1, 1), b"InvalidArgument: a WebP frame is at most 16383 x 16383 (14 bits each), not 16384 x 5"),
                        ((5, 16384, 0, 1), b"InvalidArgument: a WebP frame is at most 16383 x 16383 (14 bits each), not 5 x 16384"),
                        ((5, 5, 1, 0), b"InvalidArgument: 1..65535 images per stage"), ((5, 5, 1, 65536), b"InvalidArgument: 1..65535 images per stage")):
        assert L.ifhip_webp_lossy_enc_stage_create(C.byref(h), *args) == INVALID and L.ifhip_last_error_message() == words, args
        assert not h.value
    assert L.ifhip_webp_lossy_enc_stage_create(None, 5, 5, 1, 1) == INVALID and L.ifhip_last_error_message() == b"InvalidArgument: null stage out-pointer"
    assert L.ifhip_webp_lossy_enc_stage_create(C.byref(h), 16383, 16383, 1, 1) == 0     # geometry only: the scratch comes with the first batch
    L.ifhip_webp_lossy_enc_stage_destroy(h)
    assert L.ifhip_webp_lossy_enc_stage_max_file_bytes(None) == 0
    from tests import vp8_encode_emu as E
    for w, hh, alpha in ((800, 450, 0), (800, 450, 1), (17, 33, 1), (1, 1, 0)):
        assert L.ifhip_webp_lossy_enc_stage_create(C.byref(h), w, hh, alpha, 2) == 0
        assert L.ifhip_webp_lossy_enc_stage_max_file_bytes(h) == int(E.emulator().vp8e_emu_max_file_bytes(w, hh, alpha))
        L.ifhip_webp_lossy_enc_stage_destroy(h)
    s = c.stage()
    assert c.batch(s, n=0, images=None, files=None, lengths=None, own=True)[0] == 0, "an empty batch is answered before its pointers are looked at"
    assert c.batch(s, own=True) == (INVALID, c.own_text)
    nan = L.ifhip_webp_lossy_encode_batch_device(s, EH.P_IN, H * STRIDE, STRIDE, 1, float("nan"), EH.P_OUT, 1 << 20, EH.P_LEN, None, None)
    assert nan == INVALID and L.ifhip_last_error_message() == b"InvalidArgument: quality is not a number"
    if not torch.cuda.is_available():                                  # (with a GPU the made-up pointers must not reach a kernel)
        assert c.batch(s)[0] in NO_GPU, "a well-formed call reaches the device check"
        assert c.host()[0] in NO_GPU
    c.destroy_fn(s)


# ---- the shim's switch -------------------------------------------------------------------------------------------------------------------

def _job(preset, form="steps"):
    if form == "steps":
        return {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": preset}}]}}
    return {"framewise": {"graph": {"nodes": {"0": {"decode": {"io_id": 0}}, "1": {"encode": {"io_id": 1, "preset": preset}}},
                                    "edges": [{"from": 0, "to": 1, "kind": "input"}]}}}


def _send(preset, on, form="steps"):
    rows = np.zeros((8, 64), np.uint8)
    with Context() as c:
        if on is not None:
            assert c.set_webp_lossy_encoder(on)
        c.add_input_buffer(0, pack_raw_bgra(rows, 16, 8, alpha_meaningful=False))
        c.add_output_buffer(1)
        status, _ = c.send_json("v1/execute", _job(preset, form))
        message = c.error_message()[0] if status != 200 else ""
        return status, c.error_code(), message, bytes(c.get_output_buffer(1)) if status == 200 else b""


def test_the_switch_is_off_by_default_and_the_dispatch_function_is_unchanged():
    L = _native.lib()
    L.ifhip_encode_preset_coder.argtypes = [C.c_char_p, C.c_size_t]
    for text in (b'{"webplossy": {"quality": 80.0}}', b'"webplossy"', b'{"webplossy": {}}'):
        assert L.ifhip_encode_preset_coder(text, len(text)) == 0        # IFHIP_ENCODE_CODER_RAW, as pinned
    if torch.cuda.is_available():
        pytest.skip("the jobs below are the GPU suite's (tests/test_gpu_webp_lossy_encode.py)")
    for on in (None, False):                                           # off: the job is what it was -- without a device its frame cannot even go up
        status, code, message, _ = _send({"webplossy": {"quality": 80.0}}, on)
        assert status != 200 and "InvalidJson" not in message
        status, code, message, _ = _send("webplossy", on)              # the forms that the switch refuses are not looked at
        assert "InvalidJson" not in message
    assert _send({"webplossy": {}}, False)[2] == _send("gif", None)[2], "off: a webplossy preset of any form runs into what the raw tap runs into"


@pytest.mark.parametrize("form", ["steps", "graph"])
def test_with_the_switch_on_the_forms_that_do_not_deserialise_are_invalid_json_before_any_node_runs(form):
    for preset in ("webplossy", {"webplossy": {}}, {"webplossy": {"quality": "80"}}, {"webplossy": {"quality": None}}, {"webplossy": 80}):
        status, code, message, out = _send(preset, True, form)
        assert status == 400 and code == 3, (preset, status, code, message)    # InvalidJson: no node ran, so no device was asked for
        assert message.startswith("InvalidJson: encode.preset.webplossy.quality is a number") and out == b""


def test_with_the_switch_on_and_no_gpu_a_job_answers_a_gpu_error_and_writes_nothing():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    status, code, message, out = _send({"webplossy": {"quality": 80.0}}, True)
    assert status != 200 and out == b"" and "Gpu" in message, (status, code, message)


def test_the_kernels_use_no_scratch_and_hold_what_the_design_table_states():
    rows = resource_usage(os.path.join(B.CSRC, "vp8_encode.hip"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert sorted(rows) == sorted(KERNELS)
    for name, lanes in KERNELS.items():
        r = rows[name]
        assert _int(r, "ScratchSize [bytes/lane]") == 0, (name, r)
        assert _int(r, "LDS Size [bytes/block]") <= 64 * 1024, (name, r)
        assert _int(r, "VGPRs") <= 512 // max(1, lanes // 256), (name, r)
        m = re.search(r"\| `%s` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|" % name, design)      # lanes, VGPRs, LDS bytes, scratch
        assert m, name
        assert [int(g) for g in m.groups()] == [lanes, _int(r, "VGPRs"), _int(r, "LDS Size [bytes/block]"), 0], (name, m.groups(), r)
