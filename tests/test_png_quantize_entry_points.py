"""The C ABI of the device palette coder without a GPU: the header declares the ifhip_png_quant* entries, the bindings and
the library carry them; stage and batch arguments are checked, the frame checks before the device is asked for; the new
kernels stay out of scratch memory and inside a workgroup's LDS; the truecolour stage still refuses colour type 3."""
import ctypes as C
import os
import re

import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd import build as B  # noqa: E402
from imageflow_amd.codecs import libpng_encoder as PNG  # noqa: E402
from imageflow_amd.codecs import pngquant as Q  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from tests.test_kernel_resources import resource_usage, _int  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ifhip_png_quant_stage_create", "ifhip_png_quant_stage_destroy", "ifhip_png_quant_stage_max_file_bytes",
           "ifhip_png_quantize_batch_device", "ifhip_png_quantize"]
W, H = 37, 23
STRIDE = 4 * W + 8
INVALID = int(ErrorKind.InvalidArgument)
NO_GPU = (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))


def test_header_bindings_and_library_agree_on_the_new_names():
    header = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop.rs")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert re.search(r"IFHIP_API [^;]*\b%s\(" % name, header), name
        assert re.search(r"\bfn %s\(" % name, bindings), name
        assert getattr(L, name) is not None
    for cite in ("imageflow_types/src/lib.rs:756-761", "codecs/pngquant.rs", "lode.rs:162-195"):
        assert cite in header, cite
    assert re.search(r"#define IFHIP_PNG_QUALITY_TOO_LOW 2\b", header) and re.search(r"#define IFHIP_PNG_FILE_OVERFLOW 1\b", header)
    assert Q.PNG_QUALITY_TOO_LOW == 2 and Q.PNG_FILE_OVERFLOW == PNG.PNG_FILE_OVERFLOW


def test_stage_arguments():
    L = Q._bind()
    h = C.c_void_p()
    assert L.ifhip_png_quant_stage_create(None, 5, 5, 1) == INVALID
    assert L.ifhip_png_quant_stage_create(C.byref(h), 0, 5, 1) == INVALID
    assert L.ifhip_png_quant_stage_create(C.byref(h), 5, 0, 1) == INVALID
    assert L.ifhip_png_quant_stage_create(C.byref(h), 5, 5, 0) == INVALID
    assert L.ifhip_png_quant_stage_create(C.byref(h), 5, 5, 65536) == INVALID
    assert L.ifhip_png_quant_stage_create(C.byref(h), 20000, 20000, 1) == INVALID      # more than 2^28 pixels
    assert L.ifhip_png_quant_stage_create(C.byref(h), 16385, 1024, 1) == INVALID       # the last lane's error row would not fit LDS
    assert L.ifhip_png_quant_stage_create(C.byref(h), 16385, 1023, 1) == 0
    L.ifhip_png_quant_stage_destroy(h)
    assert L.ifhip_png_quant_stage_create(C.byref(h), 800, 450, 2) == 0
    n = 450 * (1 + 800)
    # every block stored, the zlib header and Adler-32; signature, IHDR, a full PLTE and tRNS, IDAT's 12 bytes, IEND
    assert L.ifhip_png_quant_stage_max_file_bytes(h) == n + 5 * -(-n // 32768) + 6 + 8 + 25 + (12 + 768) + (12 + 256) + 12 + 12
    L.ifhip_png_quant_stage_destroy(h)
    assert L.ifhip_png_quant_stage_max_file_bytes(None) == 0


def test_the_truecolour_stage_still_refuses_colour_type_3():
    L = PNG._bind()
    h = C.c_void_p()
    assert L.ifhip_png_enc_stage_create(C.byref(h), 5, 5, 3, 1) == INVALID


def test_argument_and_frame_checks_come_before_the_device_check():
    """Without a GPU: bad arguments and frames are argument errors, a well-formed call reaches the device check.  (The
    pointers are made up, so this must never run where a kernel could be launched.)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present: the made-up pointers below must not reach a kernel")
    L = Q._bind()
    h = C.c_void_p()
    assert L.ifhip_png_quant_stage_create(C.byref(h), W, H, 1) == 0                   # geometry only: the scratch comes with the first batch
    p_in, p_out, p_len = 0x7F0000000000, 0x7F0000100000, 0x7F0000200000              # 16-byte aligned, never dereferenced
    pitch = L.ifhip_png_quant_stage_max_file_bytes(h)

    def call(image_bytes=H * STRIDE, stride=STRIDE, ptr=p_in, n=1, max_colors=256, dither=1, level=6, out=p_out, file_pitch=pitch, mse=None):
        return L.ifhip_png_quantize_batch_device(h, ptr, image_bytes, stride, 1, n, -1, -1, -1, max_colors, dither, level, out, file_pitch, p_len, None,
                                                 None, None, mse, None)
    assert call(stride=4 * W - 4) == INVALID
    assert call(stride=STRIDE + 2) == INVALID
    assert call(image_bytes=(H - 1) * STRIDE + 4 * W - 4) == INVALID
    assert call(ptr=p_in + 2) == INVALID
    assert call(n=2) == INVALID                                                       # more than the stage holds
    assert call(max_colors=1) == INVALID and call(max_colors=257) == INVALID
    assert call(dither=2) == INVALID
    assert call(level=10) == INVALID
    assert call(out=None) == INVALID
    assert call(file_pitch=1000) == INVALID
    assert call(mse=0x7F0000300004) == INVALID
    assert call(n=0) == 0
    assert call() in NO_GPU
    assert call(max_colors=2, dither=0) in NO_GPU
    L.ifhip_png_quant_stage_destroy(h)
    out, n, status = (C.c_uint8 * 16)(), C.c_size_t(0), C.c_uint32(0)
    frame = (C.c_uint8 * (H * STRIDE))()
    assert L.ifhip_png_quantize(frame, W, H, 4 * W - 4, 1, -1, -1, -1, out, 16, C.byref(n), C.byref(status)) == INVALID
    assert L.ifhip_png_quantize(frame, W, H, STRIDE, 1, -1, -1, -1, out, 16, None, None) == INVALID
    assert L.ifhip_png_quantize(frame, W, H, STRIDE, 1, -1, -1, -1, out, 16, C.byref(n), C.byref(status)) in NO_GPU


def test_quantize_kernels_use_no_scratch_and_fit_a_workgroups_lds():
    rows = resource_usage(os.path.join(B.CSRC, "png_quantize.hip"))
    lanes = {"pngq_histogram_kernel": 256, "pngq_palette_kernel": 1024, "pngq_remap_kernel": 1024, "pngq_finish_kernel": 256}
    for name, n in lanes.items():
        r = rows[name]
        assert _int(r, "ScratchSize [bytes/lane]") == 0, (name, r)
        assert _int(r, "LDS Size [bytes/block]") <= 160 * 1024, (name, r)
        assert _int(r, "VGPRs") <= 512 // max(1, n // 256), (name, r)
    # the kernels of the shared deflate keep their names: the palette coder launches them, it does not fork them
    shared = resource_usage(os.path.join(B.CSRC, "png_deflate.hip"))
    for name in ("png_match_kernel", "png_codes_kernel", "png_layout_kernel", "png_emit_kernel"):
        assert name in shared and not any(name in k for k in rows), name
