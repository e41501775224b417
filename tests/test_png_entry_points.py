"""The C ABI of the device PNG coder without a GPU: the header declares the four ifhip_png_* entries (plus the stage's
max_file_bytes) and the library exports them; the frame checks of ifhip_png_encode_batch_device come before the device
check; the new kernels stay out of scratch memory and inside a workgroup's LDS."""
import ctypes as C
import os
import re

import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd import build as B  # noqa: E402
from imageflow_amd.codecs import libpng_encoder as PNG  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from tests.test_kernel_resources import resource_usage, _int  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ifhip_png_enc_stage_create", "ifhip_png_enc_stage_destroy", "ifhip_png_enc_stage_max_file_bytes",
           "ifhip_png_encode_batch_device", "ifhip_png_encode"]
W, H = 37, 23
STRIDE = 4 * W + 8
INVALID = int(ErrorKind.InvalidArgument)


def test_header_declares_and_library_exports_the_png_entries():
    header = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop.rs")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert re.search(r"IFHIP_API [^;]*\b%s\(" % name, header), name
        assert re.search(r"\bfn %s\(" % name, bindings), name
        assert getattr(L, name) is not None
    for cite in ("imageflow_types/src/lib.rs:751-755", "codecs/auto.rs:241-268", "codecs/libpng_encoder.rs:43-72,134-160", "codec_png_wrapper.c:349-430"):
        assert cite in header, cite


def test_stage_arguments():
    L = PNG._bind()
    h = C.c_void_p()
    assert L.ifhip_png_enc_stage_create(C.byref(h), 0, 5, PNG.PNG_RGB, 1) == INVALID
    assert L.ifhip_png_enc_stage_create(C.byref(h), 5, 5, 3, 1) == INVALID            # palette: not a colour type of this coder
    assert L.ifhip_png_enc_stage_create(C.byref(h), 5, 5, PNG.PNG_RGBA, 0) == INVALID
    assert L.ifhip_png_enc_stage_create(C.byref(h), 40000, 40000, PNG.PNG_RGBA, 1) == INVALID
    assert L.ifhip_png_enc_stage_create(C.byref(h), 800, 450, PNG.PNG_RGB, 2) == 0
    n = 450 * (1 + 3 * 800)
    assert L.ifhip_png_enc_stage_max_file_bytes(h) == n + 5 * -(-n // 32768) + 6 + 8 + 25 + 16 + 13 + 44 + 12 + 12
    L.ifhip_png_enc_stage_destroy(h)
    assert L.ifhip_png_enc_stage_max_file_bytes(None) == 0


def test_frame_checks_come_before_the_device_check():
    """Without a GPU: a bad stride and a short image_bytes are argument errors, a well-formed call reaches the device check.
    (The pointers are made up, so this must never run where a kernel could be launched.)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present: the made-up pointers below must not reach a kernel")
    L = PNG._bind()
    h = C.c_void_p()
    assert L.ifhip_png_enc_stage_create(C.byref(h), W, H, PNG.PNG_RGBA, 1) == 0       # geometry only: the scratch comes with the first batch
    p_in, p_out, p_len = 0x7F0000000000, 0x7F0000100000, 0x7F0000200000              # 16-byte aligned, never dereferenced
    pitch = L.ifhip_png_enc_stage_max_file_bytes(h)

    def call(image_bytes, stride, ptr=p_in, level=6):
        return L.ifhip_png_encode_batch_device(h, ptr, image_bytes, stride, 1, level, p_out, pitch, p_len, None, None)
    assert call(H * STRIDE, 4 * W - 4) == INVALID
    assert call(H * STRIDE, STRIDE + 2) == INVALID
    assert call((H - 1) * STRIDE + 4 * W - 4, STRIDE) == INVALID
    assert call(H * STRIDE, STRIDE, ptr=p_in + 2) == INVALID
    assert call(H * STRIDE, STRIDE, level=10) == INVALID
    assert call(H * STRIDE, STRIDE) in (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
    L.ifhip_png_enc_stage_destroy(h)
    out, n = (C.c_uint8 * 16)(), C.c_size_t(0)
    frame = (C.c_uint8 * (H * STRIDE))()
    assert L.ifhip_png_encode(frame, W, H, 4 * W - 4, PNG.PNG_RGB, 6, out, 16, C.byref(n)) == INVALID
    assert L.ifhip_png_encode(frame, W, H, STRIDE, PNG.PNG_RGB, 6, out, 16, C.byref(n)) in (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))


def test_png_kernels_use_no_scratch_and_fit_a_workgroups_lds():
    rows = resource_usage(os.path.join(B.CSRC, "png_encode.hip"))                      # filter and finish
    rows.update(resource_usage(os.path.join(B.CSRC, "png_deflate.hip")))              # the deflate back end's four
    lanes = {"png_filter_kernel": 256, "png_match_kernel": 1024, "png_codes_kernel": 64, "png_layout_kernel": 1024, "png_emit_kernel": 512,
             "png_finish_kernel": 1024}
    for name, n in lanes.items():
        r = rows[name]
        assert _int(r, "ScratchSize [bytes/lane]") == 0, (name, r)
        assert _int(r, "LDS Size [bytes/block]") <= 160 * 1024, (name, r)
        assert _int(r, "VGPRs") <= 512 // max(1, n // 256), (name, r)
    assert _int(rows["png_match_kernel"], "LDS Size [bytes/block]") <= 112 * 1024       # DESIGN 4.9's budget
