"""The stage flags of the device lossless-WebP coder without a GPU: the header, the bindings and the library carry
ifhip_webp_enc_stage_create_flags and IFHIP_WEBP_ENC_COLOR_INDEXING; an unknown bit is an argument error before any device is
asked for; the flag leaves the stage's bound alone; the kernels of csrc/webp_encode_indexed.hip stay out of scratch memory
and inside a workgroup's LDS; the shim's setter refuses what the coder does not know."""
import ctypes as C
import os
import re

import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd import build as B  # noqa: E402
from imageflow_amd.abi import Context  # noqa: E402
from imageflow_amd.codecs import webp_encoder as WEBP  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from tests.test_kernel_resources import resource_usage, _int  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = int(ErrorKind.InvalidArgument)


def test_header_bindings_and_library_carry_the_entry_and_the_flag():
    header = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop.rs")).read()
    assert re.search(r"IFHIP_API int ifhip_webp_enc_stage_create_flags\([^;]*uint32_t max_images,\s*uint32_t flags\);", header)
    assert re.search(r"\bpub fn ifhip_webp_enc_stage_create_flags\([^;]*max_images: u32, flags: u32\) -> c_int;", bindings)
    assert re.search(r"^#define IFHIP_WEBP_ENC_COLOR_INDEXING 1u$", header, flags=re.M)
    assert re.search(r"^pub const IFHIP_WEBP_ENC_COLOR_INDEXING: u32 = 1;", bindings, flags=re.M)
    assert WEBP.WEBP_ENC_COLOR_INDEXING == 1
    assert _native.lib().ifhip_webp_enc_stage_create_flags is not None
    shim = open(os.path.join(ROOT, "include", "imageflow_abi_subset.h")).read()
    assert re.search(r"IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_webp_lossless_flags\(struct imageflow_context \*context, uint32_t flags\);", shim)


def test_flags_are_checked_before_any_device_and_leave_the_bound_alone():
    L = WEBP._bind()
    h, plain = C.c_void_p(), C.c_void_p()
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert L.ifhip_webp_enc_stage_create_flags(C.byref(h), 37, 23, 1, 1, flags) == INVALID, flags
        assert L.ifhip_last_error_message().startswith(b"InvalidArgument: unknown WebP stage flags") and not h.value
    assert L.ifhip_webp_enc_stage_create_flags(C.byref(h), 0, 23, 1, 1, 1) == INVALID              # the geometry's checks are the plain entry's
    assert L.ifhip_webp_enc_stage_create_flags(C.byref(h), 37, 16385, 1, 1, 1) == INVALID
    assert L.ifhip_webp_enc_stage_create_flags(None, 37, 23, 1, 1, 1) == INVALID
    for w, hh, alpha, n in ((37, 23, 1, 1), (800, 450, 0, 32), (16384, 16384, 1, 1), (1, 1, 1, 1)):
        assert L.ifhip_webp_enc_stage_create(C.byref(plain), w, hh, alpha, n) == 0
        for flags in (0, 1):                                              # geometry only: the scratch comes with the first batch
            assert L.ifhip_webp_enc_stage_create_flags(C.byref(h), w, hh, alpha, n, flags) == 0 and h.value
            assert L.ifhip_webp_enc_stage_max_file_bytes(h) == L.ifhip_webp_enc_stage_max_file_bytes(plain) > 0
            L.ifhip_webp_enc_stage_destroy(h)
        L.ifhip_webp_enc_stage_destroy(plain)


def test_a_flagged_stage_checks_its_frames_before_the_device():
    """(The pointers are made up, so this must never run where a kernel could be launched.)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present: the made-up pointers below must not reach a kernel")
    L = WEBP._bind()
    h = C.c_void_p()
    w, hh, stride = 37, 23, 4 * 37 + 8
    assert L.ifhip_webp_enc_stage_create_flags(C.byref(h), w, hh, 1, 1, 1) == 0
    pitch = L.ifhip_webp_enc_stage_max_file_bytes(h)
    p_in, p_out, p_len = 0x7F0000000000, 0x7F0000100000, 0x7F0000200000
    assert L.ifhip_webp_encode_batch_device(h, p_in, hh * stride, 4 * w - 4, 1, p_out, pitch, p_len, None, None) == INVALID
    assert L.ifhip_webp_encode_batch_device(h, p_in, hh * stride, stride, 2, p_out, pitch, p_len, None, None) == INVALID
    assert L.ifhip_webp_encode_batch_device(h, p_in, hh * stride, stride, 1, p_out, pitch, p_len, None, None) in (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
    L.ifhip_webp_enc_stage_destroy(h)


def test_indexing_kernels_use_no_scratch_and_fit_a_workgroups_lds():
    rows = resource_usage(os.path.join(B.CSRC, "webp_encode_indexed.hip"))
    lanes = {"webp_ix_count_kernel": 256, "webp_ix_palette_kernel": 1024, "webp_ix_bundle_kernel": 256, "webp_ix_parse_kernel": 1024,
             "webp_ix_codes_kernel": 256, "webp_ix_layout_kernel": 1024, "webp_ix_emit_kernel": 1024}
    for name, n in lanes.items():
        r = rows[name]
        print(name, r)
        assert _int(r, "ScratchSize [bytes/lane]") == 0, (name, r)
        assert _int(r, "LDS Size [bytes/block]") <= 160 * 1024, (name, r)
        assert _int(r, "VGPRs") <= 512 // max(1, n // 256), (name, r)
    assert _int(rows["webp_ix_parse_kernel"], "LDS Size [bytes/block]") <= 80 * 1024    # as the plain parse: two workgroups per CU
    assert _int(rows["webp_ix_emit_kernel"], "LDS Size [bytes/block]") <= 40 * 1024


def test_the_shims_setter_takes_the_coders_flags_only():
    with Context() as c:
        assert c.L.ifhip_shim_context_set_webp_lossless_flags(c.p, 0) is True
        assert c.L.ifhip_shim_context_set_webp_lossless_flags(c.p, 1) is True
        for flags in (2, 3, 0x80000000):
            assert c.L.ifhip_shim_context_set_webp_lossless_flags(c.p, flags) is False, flags
        assert c.set_webp_lossless_flags(color_indexing=True) is True and c.set_webp_lossless_flags() is True
