"""The host code around the kernel launches of the C entry points (csrc/hip_entry.hpp):
  * every synchronous host-buffer drop-in that no other test calls gives the bytes of its _batch_device form on one frame
    (odd sizes, a padded stride that is not a multiple of 16), side outputs included;
  * an image_bytes shorter than one frame, (h-1)*stride + 4*w, is refused with IFHIP_INVALID_ARGUMENT by every entry that
    checks a batch of BGRA frames -- on the GPU through real tensors, and without a GPU before the device check."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from imageflow_amd.graphics import bitmap_ops as G  # noqa: E402
from imageflow_amd.graphics import rounded_corners as RC  # noqa: E402
from imageflow_amd.graphics import white_balance as WB  # noqa: E402
from imageflow_amd.graphics import whitespace as WS  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402

DEV = "cuda:0"
W, H = 37, 23
STRIDE = 4 * W + 8                      # 156: 4-byte aligned, not a multiple of 16
INVALID = int(ErrorKind.InvalidArgument)


def _frame(w=W, h=H, stride=STRIDE, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, stride), dtype=np.uint8)


def _device(a, w=W, h=H, stride=STRIDE, **kw):
    return Bitmap.from_numpy(a.copy()[None], w, h, stride, DEV, **kw)


def _short(w, h, stride):
    return (h - 1) * stride + 4 * w - 4


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- drop-ins against the device form ----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_color_matrix_and_flip_dropins_equal_the_device_form():
    L = G._bind()
    a = _frame(seed=1)
    m = np.random.default_rng(2).normal(0, 1.5, (5, 5)).astype(np.float32)
    host = a.copy()
    _native.check(L.ifhip_apply_color_matrix(host.ctypes.data, W, H, STRIDE, m.ctypes.data))
    b = _device(a)
    G.window_bgra32_apply_color_matrix(b, m)
    assert np.array_equal(host, b.to_numpy()[0])
    for dropin, device in ((L.ifhip_flip_vertical, G.flow_bitmap_bgra_flip_vertical_safe),
                           (L.ifhip_flip_horizontal, G.flow_bitmap_bgra_flip_horizontal_safe)):
        host = a.copy()
        _native.check(dropin(host.ctypes.data, W, H, STRIDE))
        b = _device(a)
        device(b)
        assert np.array_equal(host, b.to_numpy()[0])
        assert not np.array_equal(host, a)


@pytest.mark.gpu
def test_fill_rect_dropin_equals_the_device_form():
    a = _frame(seed=3)
    host = a.copy()
    _native.check(G._bind().ifhip_fill_rect(host.ctypes.data, W, H, STRIDE, 0, 3, 2, 30, 21, 0x80402010))
    b = _device(a)
    G.fill_rectangle(b, 0x80402010, 3, 2, 30, 21)
    assert np.array_equal(host, b.to_numpy()[0])


@pytest.mark.gpu
@pytest.mark.parametrize("in_alpha,canvas_alpha", [(1, 0), (0, 1), (0, 0)])
def test_copy_rect_dropin_equals_the_device_form(in_alpha, canvas_alpha):
    cw, ch, cs = 29, 31, 4 * 29 + 8
    a, c = _frame(seed=4), _frame(cw, ch, cs, seed=5)
    hi, hc, flag = a.copy(), c.copy(), C.c_int(canvas_alpha)
    _native.check(G._bind().ifhip_copy_rect(hi.ctypes.data, W, H, STRIDE, in_alpha, hc.ctypes.data, cw, ch, cs, C.byref(flag),
                                            5, 3, 2, 4, 21, 17))
    bi = _device(a, alpha_meaningful=bool(in_alpha))
    bc = _device(c, cw, ch, cs, alpha_meaningful=bool(canvas_alpha))
    G.copy_rectangle(bi, bc, 5, 3, 2, 4, 21, 17)
    assert np.array_equal(hc, bc.to_numpy()[0])
    assert np.array_equal(hi, bi.to_numpy()[0])                  # the input's alpha is normalised the same way
    assert bool(flag.value) == bc.alpha_meaningful


@pytest.mark.gpu
def test_transpose_dropin_equals_the_device_form_and_keeps_the_canvas_padding():
    ts = 4 * H + 8
    a, t = _frame(seed=6), _frame(H, W, ts, seed=7)
    host = t.copy()
    _native.check(G._bind().ifhip_transpose(a.ctypes.data, W, H, STRIDE, host.ctypes.data, H, W, ts))
    bt = _device(t, H, W, ts)
    G.bitmap_window_transpose(_device(a), bt)
    assert np.array_equal(host, bt.to_numpy()[0])
    assert np.array_equal(host[:, 4 * H:], t[:, 4 * H:])
    assert np.array_equal(host[:, :4 * H].reshape(W, H, 4), a[:, :4 * W].reshape(H, W, 4).transpose(1, 0, 2))


@pytest.mark.gpu
def test_detect_content_dropin_equals_the_device_form():
    a = np.full((H, STRIDE), 255, np.uint8)
    a[6:15, 4 * 9:4 * 28] = np.random.default_rng(8).integers(0, 256, size=(9, 4 * 19), dtype=np.uint8)
    host, rect = a.copy(), np.zeros(4, np.uint32)
    _native.check(WS._bind().ifhip_detect_content(host.ctypes.data, W, H, STRIDE, 0, 80, rect.ctypes.data_as(C.POINTER(C.c_uint32))))
    assert [tuple(int(v) for v in rect)] == WS.detect_content(_device(a), 80)
    assert tuple(int(v) for v in rect) != (0, 0, W, H)
    assert np.array_equal(host, a)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,radii", [("pixels", [9.5]), ("circle", [0.0]), ("percentage_custom", [10.0, 40.0, 0.0, 75.0])])
def test_round_corners_dropin_equals_the_device_form(mode, radii):
    a = _frame(seed=9)
    r = (radii * 4)[:4]
    host = a.copy()
    _native.check(RC._bind().ifhip_round_corners(host.ctypes.data, W, H, STRIDE, RC.MODES[mode], (C.c_float * 4)(*r), 0x80FF8040))
    b = _device(a)
    RC.clear_around_rounded_corners(b, mode, r, 0x80FF8040)
    assert np.array_equal(host, b.to_numpy()[0])
    assert not np.array_equal(host, a)


@pytest.mark.gpu
def test_white_balance_dropin_equals_the_device_form_with_its_histograms():
    a = _frame(seed=10)
    a[:, :4 * W] //= 2
    host, hist = a.copy(), np.zeros(768, np.uint64)
    _native.check(WB._bind().ifhip_white_balance(host.ctypes.data, W, H, STRIDE, 0.006, hist.ctypes.data))
    b = _device(a)
    dh = torch.zeros(768, dtype=torch.int64, device=DEV)
    WB.white_balance_srgb(b, 0.006, dh)
    assert np.array_equal(host, b.to_numpy()[0])
    assert np.array_equal(hist, dh.cpu().numpy().view(np.uint64))
    assert int(hist.sum()) == 3 * W * H
    no_hist = a.copy()
    _native.check(WB._bind().ifhip_white_balance(no_hist.ctypes.data, W, H, STRIDE, 0.006, None))
    assert np.array_equal(no_hist, host)


# ---- image_bytes shorter than one frame -------------------------------------------------------------------------------

def _bitmap_calls(p_in, p_out, image_bytes, stride, stream=None):
    """The eight batch entries that take one BGRA frame geometry (W x H, `stride`) on the pointers given; the transpose
    and copy_rect canvases get a correct frame of their own, so that only the checked frame is short."""
    L = G._bind()
    m = np.eye(5, dtype=np.float32)
    flag = C.c_int(0)
    ts = 4 * H
    return {
        "color_matrix": lambda: L.ifhip_apply_color_matrix_batch_device(p_in, image_bytes, 1, W, H, stride, m.ctypes.data, stream),
        "fill_rect": lambda: L.ifhip_fill_rect_batch_device(p_in, image_bytes, 1, W, H, stride, 0, 0, 0, W, H, 0xFF000000, stream),
        "normalize_alpha": lambda: L.ifhip_normalize_unused_alpha_batch_device(p_in, image_bytes, 1, W, H, stride, 0, stream),
        "flip_v": lambda: L.ifhip_flip_vertical_batch_device(p_in, image_bytes, 1, W, H, stride, stream),
        "flip_h": lambda: L.ifhip_flip_horizontal_batch_device(p_in, image_bytes, 1, W, H, stride, stream),
        "copy_rect": lambda: L.ifhip_copy_rect_batch_device(p_in, image_bytes, W, H, stride, 0, p_out, H * STRIDE, W, H, STRIDE,
                                                            C.byref(flag), 0, 0, 0, 0, W, H, 1, stream),
        "transpose": lambda: L.ifhip_transpose_batch_device(p_in, image_bytes, W, H, stride, p_out, W * ts, H, W, ts, 1, stream),
        "apply_matte": lambda: _native.lib().ifhip_apply_matte_batch_device(p_in, image_bytes, 1, W, H, stride, 1, 0xFF204080, stream),
    }


@pytest.mark.gpu
def test_short_image_bytes_is_refused_on_the_device():
    frame = torch.zeros(H * STRIDE, dtype=torch.uint8, device=DEV)          # holds the whole frame: nothing could run past it
    other = torch.zeros(H * STRIDE, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        for name, call in _bitmap_calls(frame.data_ptr(), other.data_ptr(), _short(W, H, STRIDE), STRIDE, _stream()).items():
            assert call() == INVALID, name
        for name, call in _bitmap_calls(frame.data_ptr(), other.data_ptr(), _short(W, H, STRIDE) + 4, STRIDE, _stream()).items():
            assert call() == 0, name                                      # exactly one frame is enough
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_short_image_bytes_is_refused_by_the_jpeg_stages():
    from imageflow_amd.codecs.mozjpeg import JpegForwardStage
    from imageflow_amd.codecs.mozjpeg_decoder import JpegPixelStage
    frame = torch.zeros(H * STRIDE, dtype=torch.uint8, device=DEV)
    qt = torch.ones((1, 3, 64), dtype=torch.int16, device=DEV)
    fwd = JpegForwardStage(W, H, [2, 1, 1], [2, 1, 1], 1, DEV)
    coef = [torch.zeros((1, fwd.blocks_h[c], fwd.blocks_w[c], 64), dtype=torch.int16, device=DEV) for c in range(3)]
    with torch.cuda.device(DEV):
        assert _forward(fwd, frame, _short(W, H, STRIDE), qt, coef) == INVALID
        assert _forward(fwd, frame, _short(W, H, STRIDE) + 4, qt, coef) == 0
        torch.cuda.synchronize()
    inv = JpegPixelStage(W, H, 3, [2, 1, 1], [2, 1, 1], 1, DEV)
    assert (inv.out_w, inv.out_h) == (W, H)
    with torch.cuda.device(DEV):
        assert _idct(inv, coef, qt, frame, _short(W, H, STRIDE)) == INVALID
        assert _idct(inv, coef, qt, frame, _short(W, H, STRIDE) + 4) == 0
        torch.cuda.synchronize()


def _forward(stage, frame, image_bytes, qt, coef):
    from imageflow_amd.codecs import mozjpeg
    return mozjpeg._bind().ifhip_jpeg_forward_batch_device(stage._h, frame.data_ptr(), image_bytes, STRIDE, qt.data_ptr(), 1,
                                                           coef[0].data_ptr(), coef[1].data_ptr(), coef[2].data_ptr(), _stream())


def _idct(stage, coef, qt, frame, image_bytes):
    from imageflow_amd.codecs import mozjpeg_decoder
    return mozjpeg_decoder._bind().ifhip_jpeg_idct_color_batch_device(stage._h, coef[0].data_ptr(), coef[1].data_ptr(),
                                                                      coef[2].data_ptr(), qt.data_ptr(), 1, frame.data_ptr(),
                                                                      image_bytes, STRIDE, _stream())


def test_frame_checks_come_before_the_device_check():
    """Without a GPU: a bad stride and a short image_bytes are argument errors, a well-formed call reaches the device check.
    (The pointers are made up, so this must never run where a kernel could be launched.)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present: the made-up pointers below must not reach a kernel")
    p_in, p_out = 0x7F0000000000, 0x7F0000100000                    # 16-byte aligned, never dereferenced
    for name, call in _bitmap_calls(p_in, p_out, H * STRIDE, 4 * W - 4).items():
        assert call() == INVALID, name
    for name, call in _bitmap_calls(p_in, p_out, _short(W, H, STRIDE), STRIDE).items():
        assert call() == INVALID, name
    for name, call in _bitmap_calls(p_in, p_out, H * STRIDE, STRIDE).items():
        assert call() in (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError)), name


def test_set_thread_stream_is_bound_and_accepts_none():
    """_native.set_thread_stream exists, takes None (the null stream) and a raw handle, and needs no device: it only notes
    the stream for this thread's later create calls."""
    assert _native.set_thread_stream(None) is None
    _native.set_thread_stream(0)
    _native.set_thread_stream(None)
