"""GPU parity of the mozjpeg preset's trellis stage (csrc/jpeg_trellis.hip behind the raw form of csrc/jpeg_forward.hip): the
planes it leaves in HBM equal the CPU emulation's (tests/jpeg_trellis_emulate.cpp, which defines the coder) byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

from imageflow_amd import _native
from imageflow_amd.codecs import mozjpeg as M
from imageflow_amd.graphics.bitmaps import Bitmap, get_stride
from tests import jpeg_trellis_emu as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, SENTINEL = 256, 0x5A5A
INVALID = 1                     # include/imageflow_hip.h IFHIP_INVALID_ARGUMENT
# 257 crosses the forward kernel's 256-pixel tile; 17 x 9 has 12 blocks and 40 x 24 has 36: neither fills its last 16-block workgroup
SIZES = [(1, 1), (17, 9), (33, 31), (257, 17), (40, 24)]


def upload(frames):
    """frames: list of uint8 [h][w][4] of one size -> Bitmap with the library's stride"""
    h, w = frames[0].shape[:2]
    stride = get_stride(w)
    host = np.zeros((len(frames), h, stride), np.uint8)
    for i, f in enumerate(frames):
        host[i, :, :w * 4] = f.reshape(h, w * 4)
    return Bitmap.from_numpy(host, w, h, stride, DEV)


def tables(n, quality):
    return torch.from_numpy(np.stack([E.quality_tables(quality)] * n).view(np.int16)).to(DEV)


def guarded(n, blocks_w, blocks_h):
    """three output planes, each with a guard region behind it"""
    flats, planes = [], []
    for c in range(3):
        size = n * blocks_h[c] * blocks_w[c] * 64
        flat = torch.full((size + GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
        flats.append(flat)
        planes.append(flat[:size].view(n, blocks_h[c], blocks_w[c], 64))
    return flats, planes


def guards_intact(flats):
    return all(bool((f[-GUARD:] == SENTINEL).all()) for f in flats)


def run(frames, quality, lambda_scale=M.TRELLIS_LAMBDA_ONE, sampling=E.S420):
    bmp = upload(frames)
    n = len(frames)
    fwd = M.JpegForwardStage(bmp.w, bmp.h, sampling[0], sampling[1], n, DEV)
    raw_flats, raw = guarded(n, fwd.blocks_w, fwd.blocks_h)
    fwd.write_frames(bmp, None, coef=raw, raw=True)
    stage = M.JpegTrellisStage(bmp.w, bmp.h, sampling[0], sampling[1], n, DEV)
    flats, coef = guarded(n, fwd.blocks_w, fwd.blocks_h)
    stage.quantize(raw, tables(n, quality), lambda_scale, coef=coef)
    torch.cuda.synchronize()
    assert guards_intact(raw_flats) and guards_intact(flats)
    return [r.cpu().numpy() for r in raw], [c.cpu().numpy() for c in coef]


@pytest.mark.parametrize("kind", E.FRAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_planes_equal_the_emulation(size, kind):
    w, h = size
    for quality in (1, 75, 100):
        want = E.reference(kind, w, h, quality)
        raw, coef = run([E.frame(kind, w, h)], quality)
        for c in range(3):
            assert np.array_equal(raw[c][0], want["raw"][c]), (quality, c)
            assert np.array_equal(coef[c][0], want["coef"][c]), (quality, c)


def test_444_and_a_heavier_lambda():
    want = E.emulate(E.frame("photo", 33, 31), E.quality_tables(75), E.S444, 4096)
    _, coef = run([E.frame("photo", 33, 31)], 75, 4096, E.S444)
    for c in range(3):
        assert np.array_equal(coef[c][0], want["coef"][c]), c


def test_batch_of_three_different_frames():
    w, h = 40, 24
    _, coef = run([E.frame(k, w, h) for k in E.FRAMES], 75)
    for i, kind in enumerate(E.FRAMES):
        want = E.reference(kind, w, h, 75)
        for c in range(3):
            assert np.array_equal(coef[c][i], want["coef"][c]), (kind, c)


@pytest.mark.parametrize("size", [(17, 9), (257, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lambda_zero_equals_the_forward_stage(size):
    w, h = size
    frames = [E.frame("photo", w, h), E.frame("noise", w, h)]
    _, coef = run(frames, 75, lambda_scale=0)
    bmp = upload(frames)
    fwd = M.JpegForwardStage(w, h, *E.S420, 2, DEV)
    plain = fwd.write_frames(bmp, tables(2, 75))
    for c in range(3):
        assert np.array_equal(coef[c], plain[c].cpu().numpy()), c


def test_host_buffer_drop_in():
    want = E.reference("photo", 33, 31, 75)
    coef = M.jpeg_trellis_host(want["raw"], 33, 31, *E.S420, E.quality_tables(75))
    for c in range(3):
        assert np.array_equal(coef[c], want["coef"][c]), c


def test_bad_arguments_are_refused_before_any_launch():
    w, h = 33, 31
    bmp = upload([E.frame("photo", w, h)])
    fwd = M.JpegForwardStage(w, h, *E.S420, 1, DEV)
    flats, raw = guarded(1, fwd.blocks_w, fwd.blocks_h)
    L = M._bind()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = [p.data_ptr() for p in raw]
    # a frame that does not fit its image_bytes; a null plane
    assert L.ifhip_jpeg_forward_raw_batch_device(fwd._h, bmp.data.data_ptr(), (h - 1) * bmp.stride, bmp.stride, 1, *ptrs, stream) == INVALID
    assert L.ifhip_jpeg_forward_raw_batch_device(fwd._h, bmp.data.data_ptr(), bmp.image_bytes, bmp.stride, 1, ptrs[0], None, ptrs[2], stream) == INVALID
    stage = M.JpegTrellisStage(w, h, *E.S420, 1, DEV)
    qt = tables(1, 75)
    out_flats, coef = guarded(1, fwd.blocks_w, fwd.blocks_h)
    outs = [p.data_ptr() for p in coef]
    one = M.TRELLIS_LAMBDA_ONE
    assert L.ifhip_jpeg_trellis_batch_device(stage._h, ptrs[0], None, ptrs[2], qt.data_ptr(), one, 1, *outs, stream) == INVALID
    assert L.ifhip_jpeg_trellis_batch_device(stage._h, *ptrs, qt.data_ptr(), one, 1, outs[0], outs[1], None, stream) == INVALID
    assert L.ifhip_jpeg_trellis_batch_device(stage._h, *ptrs, None, one, 1, *outs, stream) == INVALID
    assert L.ifhip_jpeg_trellis_batch_device(stage._h, *ptrs, qt.data_ptr(), 65536, 1, *outs, stream) == INVALID
    assert L.ifhip_jpeg_trellis_batch_device(stage._h, *ptrs, qt.data_ptr(), one, 2, *outs, stream) == INVALID      # over the stage's capacity
    assert L.ifhip_jpeg_trellis_batch_device(stage._h, ptrs[0] + 2, ptrs[1], ptrs[2], qt.data_ptr(), one, 1, *outs, stream) == INVALID
    torch.cuda.synchronize()
    assert all(bool((f == SENTINEL).all()) for f in flats + out_flats)           # nothing was launched
    assert b"InvalidArgument" in _native.lib().ifhip_last_error_message()
