"""The colour conversion kernel on an MI355X (csrc/color_profile.hip through imageflow_amd.codecs.color_profile) against its CPU
emulation (tests/color_profile_emulate.cpp: the same arithmetic header, plans and tables), byte for byte: every shape at
which the kernel takes another path, row padding and the gap between the frames of a batch left as they were, alpha carried
over.  And without a device: the argument checks, which come before the device is touched."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.codecs import color_profile as CP  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import color_profile_emulation as E  # noqa: E402
from tests.test_jpeg_headers import P3_XYZ, make_icc  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0xA5
INVALID = int(ErrorKind.InvalidArgument)
THREE_TRCS = [("gamma", 563 / 256), ("para", 3, [2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045]), ("curv", [int(round((k / 16) ** 1.8 * 65535)) for k in range(17)])]


def plans():
    """name -> (the native plan, the emulation's plan of the same source): one tone curve for all channels, one per channel,
    and gAMA + cHRM"""
    if not hasattr(plans, "made"):
        made = {}
        for name, icc in (("p3", make_icc(xyz=P3_XYZ)), ("adobe-three-trcs", E.icc_profile(E.ADOBE_XYZ, THREE_TRCS, version=2))):
            made[name] = (CP.plan_from_icc(icc), E.plan_from_icc(icc)[1])
        g = (0.5, (0.3127, 0.3290, 0.64, 0.33, 0.21, 0.71, 0.15, 0.06))
        made["gama-chrm"] = (CP.plan_from_gamma_primaries(*g), E.plan_from_gamma_primaries(*g)[1])
        made["identity"] = (CP.plan_from_gamma_primaries(0.45455, E.SRGB_CHRM), E.plan_from_gamma_primaries(0.45455, E.SRGB_CHRM)[1])
        plans.made = made
    return plans.made


def run_batch(n, w, h, stride, image_bytes, plan_name, seed):
    """n frames of seeded random bytes (alpha included) at the given stride and pitch, everything else SENTINEL; the device's
    result and the emulation's"""
    rng = np.random.default_rng(seed)
    host = np.full((n, image_bytes), SENTINEL, np.uint8)
    for i in range(n):
        rows = host[i, :h * stride].reshape(h, stride) if image_bytes >= h * stride else None
        assert rows is not None
        rows[:, :4 * w] = rng.integers(0, 256, (h, 4 * w), dtype=np.uint8)
    native, emulated = plans()[plan_name]
    want = host.copy()
    for i in range(n):
        want[i, :h * stride] = E.transform(host[i, :h * stride].reshape(h, stride), w, emulated).ravel()
    data = torch.from_numpy(host.copy()).to(DEV)
    b = Bitmap(data, w, h, stride)
    CP.transform_to_srgb(b, native)
    torch.cuda.synchronize()
    return host, data.cpu().numpy(), want


SHAPES = [(1, 1), (3, 1), (5, 2), (67, 3), (257, 3), (1024, 2), (1030, 70)]      # vector tails; rows across lanes and workgroups


@pytest.mark.gpu
@pytest.mark.parametrize("plan_name", ["p3", "adobe-three-trcs", "gama-chrm"])
@pytest.mark.parametrize("w, h", SHAPES)
def test_device_equals_the_emulation_byte_for_byte(w, h, plan_name):
    stride = (4 * w + 63) // 64 * 64                                               # Bitmap::create_u8's rows: the 16-byte path
    host, got, want = run_batch(1, w, h, stride, h * stride, plan_name, seed=w * 131 + h)
    assert np.array_equal(got, want)
    rows, before = got[0].reshape(h, stride), host[0].reshape(h, stride)
    assert np.array_equal(rows[:, 3:4 * w:4], before[:, 3:4 * w:4])               # alpha as it was
    assert (rows[:, 4 * w:] == SENTINEL).all()
    if w * h > 16:
        assert not np.array_equal(rows[:, :4 * w], before[:, :4 * w])             # and the colours did move


@pytest.mark.gpu
def test_row_padding_keeps_its_bytes_at_a_stride_that_is_no_multiple_of_16():
    w, h = 64, 5
    stride = 4 * w + 12                                                            # the dword path
    host, got, want = run_batch(1, w, h, stride, h * stride, "p3", seed=5)
    assert np.array_equal(got, want)
    assert (got[0].reshape(h, stride)[:, 4 * w:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("gap", [64, 36])
def test_a_batch_leaves_the_gap_between_its_frames_alone(gap):
    n, w, h = 3, 33, 7
    stride = 192                                                                   # get_stride(33)
    image_bytes = h * stride + gap                                                 # gap 36: the frames are no longer 16-byte aligned
    host, got, want = run_batch(n, w, h, stride, image_bytes, "adobe-three-trcs", seed=9)
    assert np.array_equal(got, want)
    assert (got[:, h * stride:] == SENTINEL).all()
    assert not np.array_equal(got[1], got[2])


@pytest.mark.gpu
def test_the_identity_plan_changes_no_byte():
    host, got, want = run_batch(2, 259, 9, 1088, 9 * 1088, "identity", seed=3)
    assert np.array_equal(got, host) and np.array_equal(want, host)
    # every byte value in every channel
    ramp = np.repeat(np.arange(256, dtype=np.uint8), 4).reshape(1, -1).copy()
    assert np.array_equal(CP.transform_to_srgb_host(ramp.copy(), 256, plans()["identity"][0]), ramp)


@pytest.mark.gpu
def test_the_host_form_stages_one_bitmap():
    w, h, stride = 37, 6, 4 * 37 + 8
    rng = np.random.default_rng(21)
    rows = np.full((h, stride), SENTINEL, np.uint8)
    rows[:, :4 * w] = rng.integers(0, 256, (h, 4 * w), dtype=np.uint8)
    want = E.transform(rows, w, plans()["p3"][1])
    got = CP.transform_to_srgb_host(rows.copy(), w, plans()["p3"][0])
    assert np.array_equal(got, want) and (got[:-1, 4 * w:] == SENTINEL).all()


def test_argument_checks_come_before_the_device_is_touched():
    """Bad arguments are argument errors with or without a GPU (the made-up pointers are never dereferenced: no kernel is
    launched for them); without one, a well-formed call gets as far as the device check."""
    L = CP._bind()
    plan = plans()["p3"][0]
    W, H, STRIDE = 37, 23, 4 * 37 + 12
    p = 0x7F0000000000

    def call(ptr=p, image_bytes=H * STRIDE, n=1, w=W, h=H, stride=STRIDE, plan_ref=C.byref(plan)):
        return L.ifhip_color_transform_batch_device(ptr, image_bytes, n, w, h, stride, plan_ref, None)
    assert call(ptr=None) == INVALID                                               # a null frame
    assert call(plan_ref=None) == INVALID
    assert call(stride=4 * W - 4) == INVALID                                       # stride < 4 w
    assert call(stride=STRIDE + 2) == INVALID                                      # a misaligned stride
    assert call(ptr=p + 2) == INVALID
    assert call(w=0) == INVALID and call(h=0) == INVALID                           # zero sizes
    assert call(image_bytes=(H - 1) * STRIDE + 4 * W - 4) == INVALID               # the last row does not fit
    assert call(n=65536) == INVALID
    assert call(n=0, ptr=None) == 0                                                # an empty batch is no work
    frame = (C.c_uint8 * (H * STRIDE))()
    assert L.ifhip_color_transform(frame, W, H, 4 * W - 4, C.byref(plan)) == INVALID
    assert L.ifhip_color_transform(None, W, H, STRIDE, C.byref(plan)) == INVALID
    assert L.ifhip_color_transform(frame, 0, H, STRIDE, C.byref(plan)) == INVALID
    if not torch.cuda.is_available():
        unavailable = (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
        assert call() in unavailable
        assert L.ifhip_color_transform(frame, W, H, STRIDE, C.byref(plan)) in unavailable
