"""The C ABI of the device GIF coder without a GPU: the header declares the ifhip_gif_enc* entries, the bindings and the
library carry them; stage and batch arguments are checked, the frame checks before the device is asked for; the new kernels
stay out of scratch memory and hold the LDS of the DESIGN table; the context switch of the job interface exists and answers."""
import ctypes as C
import os
import re

import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd import build as B  # noqa: E402
from imageflow_amd.abi import Context  # noqa: E402
from imageflow_amd.codecs import gif_encoder as GIF  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from tests.test_kernel_resources import resource_usage, _int  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ifhip_gif_enc_stage_create", "ifhip_gif_enc_stage_destroy", "ifhip_gif_enc_stage_max_file_bytes", "ifhip_gif_encode_batch_device",
           "ifhip_gif_encode"]
W, H = 37, 23
STRIDE = 4 * W + 8
INVALID = int(ErrorKind.InvalidArgument)
NO_GPU = (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
KERNELS = {"gif_remap_kernel": 256, "gif_lzw_kernel": 64, "gif_enc_scan_kernel": 256, "gif_gather_kernel": 256, "gif_finish_kernel": 256}


def test_header_bindings_and_library_agree_on_the_new_names():
    header = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop.rs")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert re.search(r"IFHIP_API [^;]*\b%s\(" % name, header), name
        assert re.search(r"\bfn %s\(" % name, bindings), name
        assert getattr(L, name) is not None
    assert "codecs/gif/mod.rs:385-592" in header
    assert re.search(r"#define IFHIP_GIF_FILE_OVERFLOW 1\b", header) and re.search(r"#define IFHIP_GIF_ENC_SEGMENT_PIXELS (\d+)\b", header)
    assert int(re.search(r"#define IFHIP_GIF_ENC_SEGMENT_PIXELS (\d+)\b", header).group(1)) == GIF.SEGMENT_PIXELS
    assert GIF.GIF_FILE_OVERFLOW == 1


def test_stage_arguments_and_the_bound_by_arithmetic():
    L = GIF._bind()
    h = C.c_void_p()
    assert L.ifhip_gif_enc_stage_create(None, 5, 5, 1) == INVALID
    assert L.ifhip_gif_enc_stage_create(C.byref(h), 0, 5, 1) == INVALID
    assert L.ifhip_gif_enc_stage_create(C.byref(h), 5, 0, 1) == INVALID
    assert L.ifhip_gif_enc_stage_create(C.byref(h), 5, 5, 0) == INVALID
    assert L.ifhip_gif_enc_stage_create(C.byref(h), 5, 5, 65536) == INVALID
    assert L.ifhip_gif_enc_stage_create(C.byref(h), 65536, 1, 1) == INVALID            # size_16()
    message = _native.lib().ifhip_last_error_message().decode()
    assert message.startswith("InvalidArgument") and "65535" in message
    assert L.ifhip_gif_enc_stage_create(C.byref(h), 1, 70000, 1) == INVALID
    assert L.ifhip_gif_enc_stage_create(C.byref(h), 20000, 20000, 1) == INVALID        # more than 2^28 pixels
    assert L.ifhip_gif_enc_stage_create(C.byref(h), 65535, 2, 1) == 0
    L.ifhip_gif_enc_stage_destroy(h)
    for w, ht in ((1, 1), (800, 450), (3840, 2160)):
        assert L.ifhip_gif_enc_stage_create(C.byref(h), w, ht, 2) == 0
        n = w * ht
        codes = n + n // (4094 - 256) + 2 * -(-n // GIF.SEGMENT_PIXELS)     # a code per pixel, a clear per full table, two per segment
        data = -(-codes * 12 // 8)
        # signature, screen, NETSCAPE2.0, graphic control extension, image descriptor, 256 entries, minimum code size; a
        # length byte per 255 data bytes; the terminator and ';'
        assert L.ifhip_gif_enc_stage_max_file_bytes(h) == (6 + 7 + 19 + 8 + 10 + 768 + 1) + data + -(-data // 255) + 2
        L.ifhip_gif_enc_stage_destroy(h)
    assert L.ifhip_gif_enc_stage_max_file_bytes(None) == 0


def test_argument_and_frame_checks_come_before_the_device_check():
    """Without a GPU: bad arguments and frames are argument errors, a well-formed call reaches the device check.  (The
    pointers are made up, so this must never run where a kernel could be launched.)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present: the made-up pointers below must not reach a kernel")
    L = GIF._bind()
    h = C.c_void_p()
    assert L.ifhip_gif_enc_stage_create(C.byref(h), W, H, 1) == 0                     # geometry only: the scratch comes with the first batch
    p_in, p_out, p_len = 0x7F0000000000, 0x7F0000100000, 0x7F0000200000              # 16-byte aligned, never dereferenced
    pitch = L.ifhip_gif_enc_stage_max_file_bytes(h)

    def call(image_bytes=H * STRIDE, stride=STRIDE, ptr=p_in, n=1, repeat=-1, delay=0, out=p_out, file_pitch=pitch, lengths=p_len, stage=h):
        return L.ifhip_gif_encode_batch_device(stage, ptr, image_bytes, stride, 1, n, repeat, delay, 0, out, file_pitch, lengths, None, None, None, None)
    assert call(stage=None) == INVALID
    assert call(ptr=None) == INVALID
    assert call(stride=4 * W - 4) == INVALID
    assert call(stride=STRIDE + 2) == INVALID
    assert call(image_bytes=(H - 1) * STRIDE + 4 * W - 4) == INVALID                  # a short frame
    assert call(ptr=p_in + 2) == INVALID
    assert call(n=2) == INVALID                                                       # more than the stage holds
    assert call(repeat=-2) == INVALID and call(repeat=65536) == INVALID
    assert call(delay=65536) == INVALID
    assert call(out=None) == INVALID and call(lengths=None) == INVALID
    assert call(file_pitch=800) == INVALID
    assert call(n=0) == 0
    assert call() in NO_GPU
    assert call(repeat=0, delay=65535) in NO_GPU
    L.ifhip_gif_enc_stage_destroy(h)
    out, n = (C.c_uint8 * 16)(), C.c_size_t(0)
    frame = (C.c_uint8 * (H * STRIDE))()
    assert L.ifhip_gif_encode(frame, W, H, 4 * W - 4, 1, -1, 0, 0, out, 16, C.byref(n)) == INVALID
    assert L.ifhip_gif_encode(None, W, H, STRIDE, 1, -1, 0, 0, out, 16, C.byref(n)) == INVALID
    assert L.ifhip_gif_encode(frame, W, H, STRIDE, 1, -1, 0, 0, out, 16, None) == INVALID
    assert L.ifhip_gif_encode(frame, 65536, 1, 4 * 65536, 1, -1, 0, 0, out, 16, C.byref(n)) == INVALID
    assert L.ifhip_gif_encode(frame, W, H, STRIDE, 1, -1, 0, 0, out, 16, C.byref(n)) in NO_GPU


def test_gif_encode_kernels_use_no_scratch_and_hold_the_lds_of_the_design_table():
    rows = resource_usage(os.path.join(B.CSRC, "gif_encode.hip"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.16" in design
    for name, lanes in KERNELS.items():
        r = rows[name]
        assert _int(r, "ScratchSize [bytes/lane]") == 0, (name, r)
        assert _int(r, "VGPRs") <= 512 // max(1, lanes // 256), (name, r)
        m = re.search(r"\| `%s` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|" % name, design)      # lanes, VGPRs, LDS bytes, scratch
        assert m, name
        assert int(m.group(1)) == lanes and int(m.group(3)) == _int(r, "LDS Size [bytes/block]") and int(m.group(4)) == 0, (name, m.groups(), r)
    assert _int(rows["gif_lzw_kernel"], "LDS Size [bytes/block]") == 4 * 8192           # the hash table: four segments share a CU's 160 KiB
    assert 4 * _int(rows["gif_lzw_kernel"], "LDS Size [bytes/block]") <= 160 * 1024
    assert _int(rows["gif_remap_kernel"], "LDS Size [bytes/block]") == 16 * 256          # the palette, premultiplied
    # the quantiser's kernels keep their names in png_quantize.hip: the GIF coder launches them, it does not fork them
    assert not any(k.startswith("pngq_") for k in rows)


def test_the_context_switch_exists_and_answers():
    header = open(os.path.join(ROOT, "include", "imageflow_abi_subset.h")).read()
    assert "ifhip_shim_context_set_gif_encoder(struct imageflow_context *context, int on)" in header
    with Context() as c:
        assert c.set_gif_encoder(True) is True
        assert c.set_gif_encoder(False) is True
