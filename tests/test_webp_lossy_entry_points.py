"""The C ABI of the device lossy WebP decoder without a GPU: the headers and the bindings declare ifhip_webp_lossy_decode (in
imageflow_hip.h, with the IFHIP_VP8_DEC_* words) and ifhip_webp_lossy_decode_batch_device (in imageflow_hip_webp_lossy.h, and
why there), and the library exports them; both refuse bad arguments in the words every file decoder uses, before the device
check; what the host stage finds needs no device; the kernels stay out of scratch memory and hold what DESIGN 4.18 states;
the lossless entry points still answer a lossy file in their old words; and the shim's switch is off by default."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd import build as B  # noqa: E402
from imageflow_amd.abi import Context  # noqa: E402
from imageflow_amd.codecs import webp_decoder, webp_lossy_decoder as D  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from tests import webp_decode_fixtures as LX  # noqa: E402
from tests import webp_lossy_fixtures as X  # noqa: E402
from tests.test_decode_handoff import refusals  # noqa: E402
from tests.test_kernel_resources import resource_usage, _int  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = int(ErrorKind.InvalidArgument)
KERNELS = {"vp8_residual_kernel": 256, "vp8_predict_kernel": 1024, "vp8_loop_filter_kernel": 1024, "vp8_alpha_kernel": 64, "vp8_to_bgra_kernel": 256}
WORDS = ("CONTAINER", "NOT_LOSSY", "FRAME_HEADER", "PARTITIONS", "END_OF_MODES", "END_OF_TOKENS", "ALPHA_HEADER", "ALPHA_STREAM")


def test_headers_bindings_and_library_agree():
    main = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    extra = open(os.path.join(ROOT, "include", "imageflow_hip_webp_lossy.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop.rs")).read()
    shim = open(os.path.join(ROOT, "include", "imageflow_abi_subset.h")).read()
    L = _native.lib()
    assert re.search(r"IFHIP_API [^;]*\bifhip_webp_lossy_decode\(", main) and re.search(r"\bfn ifhip_webp_lossy_decode\(", bindings)
    # the batch entry takes a stream: it lives in the header of its own until the stream-order table of the main header gains its row
    assert "ifhip_webp_lossy_decode_batch_device(" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert re.search(r"IFHIP_API [^;]*\bifhip_webp_lossy_decode_batch_device\([^;]*void\* hip_stream\)", extra)
    assert '#include "imageflow_hip.h"' in extra and "stream" in extra.split("#ifndef")[0]
    for name in os.listdir(os.path.join(ROOT, "include")):
        assert not re.search(r'#include\s*"imageflow_hip_webp_lossy\.h"', open(os.path.join(ROOT, "include", name)).read()), name      # included by nothing
    for name in ("ifhip_webp_lossy_decode", "ifhip_webp_lossy_decode_batch_device", "ifhip_shim_context_set_webp_lossy_decoder"):
        assert getattr(L, name) is not None
    assert "ifhip_shim_context_set_webp_lossy_decoder" in shim
    for value, word in enumerate(WORDS, 1):
        assert re.search(r"#define IFHIP_VP8_DEC_%s %d\b" % (word, value), main), word
        assert D.STATUS[value] == word.lower()
        assert getattr(X, word) == value
    core = open(os.path.join(B.CSRC, "vp8_decode_core.hpp")).read()
    for value, word in enumerate(("Container", "NotLossy", "FrameHeader", "Partitions", "EndOfModes", "EndOfTokens", "AlphaHeader", "AlphaStream"), 1):
        assert re.search(r"kVp8Dec%s = %d," % (word, value), core), word


class Lossy:
    """the shape tests/test_decode_handoff.py's refusals() asks of a decoder"""
    def __init__(self):
        self.L = D._bind()
        self.file = X.good_files()["size_33x21"]
        self.w, self.h = 33, 21

    def call_batch(self, frame_bytes, stride, frame=0x7F0000000000, files=True, file=True, n=1):
        buf = np.frombuffer(self.file, np.uint8)
        ptrs, lens = (C.c_void_p * 1)(buf.ctypes.data if file else None), (C.c_size_t * 1)(buf.size)
        frames, fb, st = (C.c_void_p * 1)(frame), (C.c_size_t * 1)(frame_bytes), (C.c_uint32 * 1)(stride)
        rc = self.L.ifhip_webp_lossy_decode_batch_device(ptrs if files else None, lens, n, frames, fb, st, 0x7F0000200000, None)
        return rc, self.L.ifhip_last_error_message()

    def call_host(self, stride, capacity, bitmap=True, file=True):
        buf = np.frombuffer(self.file, np.uint8)
        out, st = np.zeros(self.h * (4 * self.w + 16), np.uint8), C.c_uint32(0)
        rc = self.L.ifhip_webp_lossy_decode(buf.ctypes.data if file else None, buf.size, out.ctypes.data if bitmap else None, stride, capacity, C.byref(st))
        return rc, self.L.ifhip_last_error_message()


def test_every_refused_argument_is_refused_in_the_words_of_the_other_decoders():
    """the made-up device pointers never reach a kernel: every call here fails a check on the host"""
    for case, ((rc, message), want) in refusals(Lossy()).items():
        assert rc == INVALID, (case, rc)
        assert message == want, (case, message)


def test_argument_checks_and_the_host_stage_come_before_the_device_check():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the made-up pointers below must not reach a kernel")
    d = Lossy()
    stride = 4 * d.w + 8
    assert d.call_batch(d.h * stride, stride, n=0)[0] == 0
    assert d.call_batch(d.h * stride, stride)[0] in (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
    assert d.call_host(stride, d.h * stride)[0] in (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
    big, st = np.zeros(1 << 16, np.uint8), C.c_uint32(0)
    for name, (data, _, word) in X.damaged_files().items():            # what the host stage finds needs no device
        if name == "alph_stream_truncated":                               # (found by the device's VP8L reader)
            continue
        buf = np.frombuffer(data, np.uint8)
        assert d.L.ifhip_webp_lossy_decode(buf.ctypes.data, buf.size, big.ctypes.data, 4 * 56, big.size, C.byref(st)) == INVALID, name
        assert b"ImageMalformed" in d.L.ifhip_last_error_message(), name
        assert st.value == (0 if word == X.CONTAINER else word), name
    buf = np.frombuffer(LX.good_files()["w17"], np.uint8)
    assert d.L.ifhip_webp_lossy_decode(buf.ctypes.data, buf.size, big.ctypes.data, 4 * 17, big.size, C.byref(st)) == int(ErrorKind.MethodNotImplemented)
    assert b"not a lossy WebP" in d.L.ifhip_last_error_message()


def test_the_kernels_use_no_scratch_and_hold_what_the_design_table_states():
    rows = resource_usage(os.path.join(B.CSRC, "vp8_decode.hip"))
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


def test_the_lossless_entry_points_still_answer_a_lossy_file_in_their_old_words():
    L = webp_decoder._bind()
    out, st = np.zeros(1 << 16, np.uint8), C.c_uint32(0)
    for name, words in (("size_33x21", b"a lossy WebP (VP8)"), ("rgba_56x40", b"a lossy WebP (VP8 + ALPH)")):
        buf = np.frombuffer(X.good_files()[name], np.uint8)
        assert L.ifhip_webp_decode(buf.ctypes.data, buf.size, out.ctypes.data, 4 * 56, out.size, C.byref(st)) == int(ErrorKind.MethodNotImplemented)
        message = L.ifhip_last_error_message()
        assert message.startswith(b"ImageTypeNotSupported: " + words) and b"the lossy VP8 decoder is not built, only lossless VP8L files are read" in message
        info = webp_decoder.webp_info(X.good_files()[name])
        assert (info["lossless"], info["animated"], info["has_alpha"]) == (False, False, name == "rgba_56x40")


def test_the_shims_switch_is_off_by_default_and_get_image_info_follows_it():
    data = X.good_files()["rgba_56x40"]
    with Context() as c:
        c.add_input_buffer(0, data)
        status, _ = c.send_json("v1/get_image_info", {"io_id": 0})
        assert status == 400 and c.error_code() == 5 and "lossy" in c.error_message()[0]
    with Context() as c:
        assert c.set_webp_lossy_decoder(True)
        c.add_input_buffer(0, data)
        status, r = c.send_json("v1/get_image_info", {"io_id": 0})
        assert status == 200 and r["data"]["image_info"]["frame_decodes_into"] == "bgra_32" and r["data"]["image_info"]["image_width"] == 56
        assert c.set_webp_lossy_decoder(False)
        status, _ = c.send_json("v1/get_scaled_image_info", {"io_id": 0})
        assert status == 400 and c.error_code() == 5
