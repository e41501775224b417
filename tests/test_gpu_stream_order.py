"""Stream order of the device entry points, proven with late inputs (the harness: tests/stream_order.py).

Every `*_device` entry point takes a hip_stream and promises to run in that stream's order.  Each row of ROWS hands one
entry point buffers that hold a decoy until the caller's stream S -- delayed on purpose -- delivers the real contents, and
compares what the call left, in S's order, with the same independent reference the entry point's own parity test uses.  A
launch on the null stream, a copy on the thread stream instead of the caller's, or a wait for the wrong stream gives the
right bytes in every other test of the suite and wrong bytes here."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd import _native  # noqa: E402
from imageflow_amd.graphics import bitmap_ops as G  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap, BitmapCompositing  # noqa: E402
from imageflow_amd.graphics.blend import apply_matte  # noqa: E402
from imageflow_amd.graphics.color import WorkingFloatspace  # noqa: E402
from imageflow_amd.graphics.rounded_corners import clear_around_rounded_corners  # noqa: E402
from imageflow_amd.graphics.scaling import ResamplePlan, ScaleAndRenderParams, scale_and_render  # noqa: E402
from imageflow_amd.graphics.weights import Filter  # noqa: E402
from imageflow_amd.graphics.white_balance import white_balance_srgb  # noqa: E402
from imageflow_amd.graphics.whitespace import detect_content_into  # noqa: E402
from imageflow_amd.flow.nodes import color as CN  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import rounded_corners_oracle as RC  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import util as U  # noqa: E402
from tests import white_balance_oracle as WB  # noqa: E402
from tests import whitespace_oracle as WS  # noqa: E402

DEV = "cuda:0"
GUARD = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def streams():
    """(S, W), chosen once: a pair of torch streams that run side by side under this process's hardware queues."""
    try:
        return SO.choose_streams(DEV)
    except SO.StreamOrderError as e:
        pytest.fail(str(e))


def _bytes(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def gbuf(name, real, decoy, expected=None, dtype=torch.uint8, guard=256, mask=None):
    """A device buffer with a guard region behind it, as one harness buffer: `real` / `decoy` / `expected` are host arrays of
    the same size; the guard bytes belong to all three, so a store behind the data fails the comparison.  mask: the data
    bytes that are compared (default: all; the guard always is).  -> (Buf, the data as a flat tensor of `dtype`)."""
    r = _bytes(real)
    tail = np.full(guard, GUARD, np.uint8)
    t = torch.empty(r.size + guard, dtype=torch.uint8, device=DEV)
    d = _bytes(decoy)
    assert d.size == r.size, name
    b = SO.Buf(name, t, np.concatenate([r, tail]), np.concatenate([d, tail]),
               None if expected is None else np.concatenate([_bytes(expected), tail]),
               mask=None if mask is None else np.concatenate([np.asarray(mask, bool).reshape(-1), np.ones(guard, bool)]))
    return b, t[:r.size].view(dtype)


def row_mask(n, h, stride, w):
    """the pixel bytes of n frames of h rows: for outputs whose row padding the entry point leaves unspecified"""
    m = np.zeros((n, h, stride), bool)
    m[:, :, :4 * w] = True
    return m


def noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ---- rows ----------------------------------------------------------------------------------------------------------------
# A row builder returns (buffers, call): `call` enqueues the entry point on the CURRENT stream and does nothing else.
ROWS = {}


def row(name, *entry_points, waits=False):
    """waits: the call waits on the host for what is queued on its stream (the exceptions the header lists); every other row
    must return with the window open."""
    def deco(fn):
        ROWS[name] = (entry_points, fn, waits)
        return fn
    return deco


def _maker(fx, make):
    """an object of the library as a function: made once, or -- fx["create_in_call"] -- by every call, on the thread's stream"""
    if fx.get("create_in_call"):
        keep = fx.setdefault("keep", [])                             # (alive until the test ends: a destroy waits for the device)

        def fresh():
            keep.append(make())
            return keep[-1]
        return fresh
    made = make()
    return lambda: made


_PLANS = {}


def _resample(iw, ih, ow, oh, force, fx=None):
    fx = fx or {}
    n, alpha, compose, matte = 3, True, BitmapCompositing.BlendWithMatte, 0x80FF2010
    space = WorkingFloatspace.LinearRGB
    real = U.random_frames(n, iw, ih, seed0=4100 + 10 * fx.get("variant", 0), alpha=True)
    decoy = U.random_frames(n, iw, ih, seed0=4200, alpha=True)
    cst = U.stride_for(ow)
    canvas0 = noise(7, (n, oh, cst))
    exp = canvas0.copy()
    exp_f32 = U.oracle_render(real, iw, ih, exp, ow, oh, 0, 0, ow, oh, filter_id=int(Filter.Robidoux), working_space=int(space),
                              compositing=int(compose), matte_bgra=matte, alpha_meaningful=alpha, want_f32=True)
    bi, ti = gbuf("source frames", real, decoy)
    bc, tc = gbuf("canvas", canvas0, noise(8, canvas0.shape), exp)
    f0 = np.full(exp_f32.shape, 12345.0, np.float32)
    bf, tf = gbuf("f32 dump", f0, np.full(exp_f32.shape, -1.0, np.float32), exp_f32, dtype=torch.float32)
    inp = Bitmap(ti.view(n, -1), iw, ih, real.shape[2], alpha)
    can = Bitmap(tc.view(n, -1), ow, oh, cst, False, compose, matte)
    f32 = tf.view(n, oh, ow, 4)
    info = ScaleAndRenderParams(0, 0, ow, oh, 0.0, Filter.Robidoux, space)

    def make():                                                      # a plan may be shared by any number of launches: one per shape
        if (iw, ih, ow, oh) not in _PLANS or fx.get("create_in_call"):
            _PLANS[(iw, ih, ow, oh)] = ResamplePlan(iw, ih, ow, oh, Filter.Robidoux, 0.0)
        return _PLANS[(iw, ih, ow, oh)]
    plan = _maker(fx, make)
    if force == 0:
        assert plan().kernel_kind(alpha) == 0

    def call():
        scale_and_render(inp, can, info, f32_out=f32, force_kernel=force, plan=plan())
    return [bi, bc, bf], call


@row("scale_and_render fused 101x67->33x21", "ifhip_scale_and_render_batch_device")
def _(fx):
    return _resample(101, 67, 33, 21, 0)


@row("scale_and_render generic pair 101x67->33x21", "ifhip_scale_and_render_batch_device")
def _(fx):
    return _resample(101, 67, 33, 21, 1, fx)


@row("scale_and_render banded 37x23->111x70", "ifhip_scale_and_render_batch_device")
def _(fx):
    return _resample(37, 23, 111, 70, 2)


@row("scale_and_render banded strips of 16 100x100->300x300", "ifhip_scale_and_render_batch_device")
def _(fx):
    fx["debug_switch"]("banded_strip", "16")
    return _resample(100, 100, 300, 300, 2)


@row("time_scale_and_render 101x67->33x21, two launches", "ifhip_time_scale_and_render_batch_device", waits=True)
def _(fx):
    """bench.py's kernel-duration probe: the launches between two events on the caller's stream, which it then waits for"""
    from imageflow_amd.graphics.scaling import time_scale_and_render
    iw, ih, ow, oh, n = 101, 67, 33, 21, 2
    real, decoy = U.random_frames(n, iw, ih, seed0=4300, alpha=False), U.random_frames(n, iw, ih, seed0=4400, alpha=False)
    cst = U.stride_for(ow)
    canvas0 = noise(9, (n, oh, cst))
    exp = canvas0.copy()
    U.oracle_render(real, iw, ih, exp, ow, oh, 0, 0, ow, oh)        # Robidoux, linear light, ReplaceSelf: a second launch changes nothing
    bi, ti = gbuf("source frames", real, decoy)
    bc, tc = gbuf("canvas", canvas0, noise(10, canvas0.shape), exp)
    inp, can = Bitmap(ti.view(n, -1), iw, ih, real.shape[2]), Bitmap(tc.view(n, -1), ow, oh, cst)
    info = ScaleAndRenderParams(0, 0, ow, oh)
    plan = ResamplePlan(iw, ih, ow, oh, Filter.Robidoux, 0.0)

    def call():
        assert time_scale_and_render(inp, can, info, 2, plan=plan) > 0.0
    return [bi, bc], call


BW, BH, BN = 37, 29, 2


def _frames_pad(seed, w=BW, h=BH, n=BN, pad=4):
    stride = O.stride_for_width(w) + pad
    return noise(seed, (n, h, stride)), stride


def _in_place(name, op, ofn, alpha=False, w=BW, h=BH):
    real, s = _frames_pad(11, w, h)
    decoy, _ = _frames_pad(12, w, h)
    exp = real.copy()
    for k in range(real.shape[0]):
        ofn(exp[k], w, h, s)
    b, t = gbuf(name, real, decoy, exp)
    bm = Bitmap(t.view(real.shape[0], -1), w, h, s, alpha)
    return [b], lambda: op(bm)


@row("apply_matte 37x29", "ifhip_apply_matte_batch_device")
def _(fx):
    def ofn(f, w, h, s):
        O.apply_matte(f, w, h, s, 0xFF336699)

    def op(bm):
        bm.alpha_meaningful = True
        apply_matte(bm, 0xFF336699)
    return _in_place("frames", op, ofn, alpha=True)


@row("apply_color_matrix 37x29", "ifhip_apply_color_matrix_batch_device")
def _(fx):
    m = CN.sepia()
    return _in_place("frames", lambda bm: G.window_bgra32_apply_color_matrix(bm, m), lambda f, w, h, s: O.apply_color_matrix(f, w, h, s, m))


@row("flip_vertical 37x29", "ifhip_flip_vertical_batch_device")
def _(fx):
    return _in_place("frames", G.flow_bitmap_bgra_flip_vertical_safe, O.flip_vertical)


@row("flip_horizontal 37x29", "ifhip_flip_horizontal_batch_device")
def _(fx):
    return _in_place("frames", G.flow_bitmap_bgra_flip_horizontal_safe, O.flip_horizontal)


@row("fill_rect 37x29", "ifhip_fill_rect_batch_device")
def _(fx):
    return _in_place("frames", lambda bm: G.fill_rectangle(bm, 0x80FF7F01, 4, 2, 30, 19),
                     lambda f, w, h, s: O.fill_rect(f, w, h, s, False, 4, 2, 30, 19, 0x80FF7F01))


@row("normalize_unused_alpha 37x29", "ifhip_normalize_unused_alpha_batch_device")
def _(fx):
    def ofn(f, w, h, s):
        f[:, 3:4 * w:4] = 255                                       # bitmaps.rs:1570-1576: alpha of every pixel to 255
    return _in_place("frames", G.normalize_unused_alpha, ofn, alpha=False)


@row("copy_rect 37x29 -> 50x40", "ifhip_copy_rect_batch_device")
def _(fx):
    real, s = _frames_pad(21)
    decoy, _ = _frames_pad(22)
    c0, cs = _frames_pad(23, 50, 40)
    exp = c0.copy()
    for k in range(BN):
        rc, _am = O.copy_rect(real[k].copy(), BW, BH, s, True, exp[k], 50, 40, cs, False, 1, 0, 3, 2, 33, 27)
        assert rc == 0
    bi, ti = gbuf("source frames", real, decoy)
    bc, tc = gbuf("canvas", c0, noise(24, c0.shape), exp)
    ib = Bitmap(ti.view(BN, -1), BW, BH, s, True)
    cb = Bitmap(tc.view(BN, -1), 50, 40, cs, False)
    def call():
        cb.alpha_meaningful, cb.compose = False, BitmapCompositing.ReplaceSelf       # (the wrapper keeps the reference's bookkeeping)
        G.copy_rectangle(ib, cb, 1, 0, 3, 2, 33, 27)
    return [bi, bc], call


@row("transpose 37x29", "ifhip_transpose_batch_device")
def _(fx):
    real, s = _frames_pad(31)
    decoy, _ = _frames_pad(32)
    t0, ts = _frames_pad(33, BH, BW)
    exp = t0.copy()
    for k in range(BN):
        assert O.transpose(real[k], BW, BH, s, exp[k], BH, BW, ts) == 0
    bi, ti = gbuf("source frames", real, decoy)
    bt, tt = gbuf("transposed", t0, noise(34, t0.shape), exp)
    fb = Bitmap(ti.view(BN, -1), BW, BH, s)
    tb = Bitmap(tt.view(BN, -1), BH, BW, ts)
    return [bi, bt], lambda: G.bitmap_window_transpose(fb, tb)


FW, FH, FN = 67, 33, 2


def _finishing_frames(seed, kinds, pad=12):
    """[n][h][stride] with garbage in the row padding, and the pixel views [n][h][w][4] the restatements take"""
    rng = np.random.default_rng(seed)
    stride = 4 * FW + pad
    host = rng.integers(0, 256, (FN, FH, stride), dtype=np.uint8)
    for i, kind in enumerate(kinds):
        f = rng.integers(0, 256, (FH, FW, 4), dtype=np.uint8)
        if kind == "narrow":
            f[..., :3] = 60 + f[..., :3] // 3
        elif kind == "box":
            f[:] = 255
            x1, x2 = sorted(rng.integers(0, FW, 2))
            y1, y2 = sorted(rng.integers(0, FH, 2))
            f[y1:y2 + 1, x1:x2 + 1] = rng.integers(0, 256, (y2 - y1 + 1, x2 - x1 + 1, 4), dtype=np.uint8)
        host[i, :, :4 * FW] = f.reshape(FH, 4 * FW)
    return host, stride


def _pixels(host):
    return [np.ascontiguousarray(host[i, :, :4 * FW]).reshape(FH, FW, 4) for i in range(host.shape[0])]


def _with_pixels(host, frames):
    out = host.copy()
    for i, f in enumerate(frames):
        out[i, :, :4 * FW] = f.reshape(FH, 4 * FW)
    return out


@row("white_balance 67x33 with histograms", "ifhip_white_balance_batch_device")
def _(fx):
    real, stride = _finishing_frames(41, ["narrow", "random"])
    decoy, _ = _finishing_frames(42, ["random", "narrow"])
    exp = _with_pixels(real, [WB.white_balance(f.copy(), None) for f in _pixels(real)])
    hist = np.stack([WB.histograms(f).astype(np.int64) for f in _pixels(real)])
    b, t = gbuf("frames", real, decoy, exp)
    h0 = np.full(FN * 768, -7, np.int64)
    bh, th = gbuf("histograms", h0, np.full(FN * 768, -9, np.int64), hist, dtype=torch.int64)
    bm = Bitmap(t.view(FN, -1), FW, FH, stride)
    return [b, bh], lambda: white_balance_srgb(bm, None, th)


@row("white_balance 67x33 with scratch histograms", "ifhip_white_balance_batch_device")
def _(fx):
    real, stride = _finishing_frames(43 + 100 * fx.get("variant", 0), ["narrow", "random"])
    decoy, _ = _finishing_frames(44, ["random", "narrow"])
    exp = _with_pixels(real, [WB.white_balance(f.copy(), 0.02) for f in _pixels(real)])
    b, t = gbuf("frames", real, decoy, exp)
    bm = Bitmap(t.view(FN, -1), FW, FH, stride)
    return [b], lambda: white_balance_srgb(bm, 0.02)


@row("round_corners 67x33", "ifhip_round_corners_batch_device")
def _(fx):
    real, stride = _finishing_frames(45, ["random", "random"])
    decoy, _ = _finishing_frames(46, ["random", "random"])
    radii = [3.7, 20.0, 0.25, 9.0]
    exp = _with_pixels(real, [RC.clear_around_rounded_corners(f.copy(), "pixels_custom", radii, 0x80102030) for f in _pixels(real)])
    b, t = gbuf("frames", real, decoy, exp)
    bm = Bitmap(t.view(FN, -1), FW, FH, stride)
    return [b], lambda: clear_around_rounded_corners(bm, "pixels_custom", radii, 0x80102030)


@row("detect_content 67x33", "ifhip_detect_content_batch_device")
def _(fx):
    real, stride = _finishing_frames(47 + 100 * fx.get("variant", 0), ["box", "box"])
    decoy, _ = _finishing_frames(48, ["box", "box"])
    want = np.array([WS.detect_content(f, False, 20) for f in _pixels(real)], np.int64).astype(np.uint32)
    other = np.array([WS.detect_content(f, False, 20) for f in _pixels(decoy)], np.int64).astype(np.uint32)
    assert not np.array_equal(want, other), "the decoy frames must have other content rectangles"
    b, t = gbuf("frames", real, decoy)
    r0 = np.full(4 * FN, GUARD, np.uint32)
    br, tr = gbuf("rectangles", r0, np.full(4 * FN, 0x5A, np.uint32), want, dtype=torch.int32)
    bm = Bitmap(t.view(FN, -1), FW, FH, stride, False)
    rects = tr.view(FN, 4)
    return [b, br], lambda: detect_content_into(bm, 20, rects)


@row("color_transform 67x33 P3", "ifhip_color_transform_batch_device")
def _(fx):
    from imageflow_amd.codecs import color_profile as CP
    from tests import color_profile_emulation as CE
    from tests.test_gpu_color_profile import plans
    native, emulated = plans()["p3"]
    real, stride = _finishing_frames(49, ["random", "random"])
    decoy, _ = _finishing_frames(50, ["random", "random"])
    exp = np.stack([CE.transform(real[i].copy(), FW, emulated) for i in range(FN)])
    b, t = gbuf("frames", real, decoy, exp)
    bm = Bitmap(t.view(FN, -1), FW, FH, stride)
    return [b], lambda: CP.transform_to_srgb(bm, native)


# ---- JPEG: pixel stage, block scalers, decode + resample, entropy decode ---------------------------------------------------
JW, JH, JN = 40, 24, 2
S420 = ((2, 1, 1), (2, 1, 1))


def _jpeg_cases(seed, w=JW, h=JH):
    from tests.test_gpu_jpeg import _random_case
    rng = np.random.default_rng(seed)
    return [_random_case(rng, w, h, S420[0], S420[1], 3, 200) for _ in range(JN)]


def _coefficient_buffers(js_real, js_decoy):
    """the three coefficient planes and the tables of a batch, late: -> (buffers, planes as tensors [n, bh, bw, 64], tables)"""
    bufs, planes = [], []
    for c in range(3):
        real = np.stack([j["coef"][c] for j in js_real])
        b, t = gbuf("coefficients %d" % c, real, np.stack([j["coef"][c] for j in js_decoy]), dtype=torch.int16)
        bufs.append(b)
        planes.append(t.view(real.shape))
    bq, tq = gbuf("quantisation tables", np.stack([j["qt"] for j in js_real]).astype(np.uint16),
                  np.stack([j["qt"] for j in js_decoy]).astype(np.uint16), dtype=torch.int16)
    return bufs + [bq], planes, tq.view(len(js_real), 3, 64)


def _pixel_stage(fx, scale_num=8, w=JW, h=JH):
    from imageflow_amd.codecs.mozjpeg_decoder import JpegPixelStage
    return _maker(fx, lambda: JpegPixelStage(w, h, 3, S420[0], S420[1], JN, DEV, scale_num=scale_num))


@row("jpeg_idct_color 4:2:0 40x24", "ifhip_jpeg_idct_color_batch_device")
def _(fx):
    js = _jpeg_cases(61 + fx.get("variant", 0))
    bufs, planes, qt = _coefficient_buffers(js, _jpeg_cases(62))
    stride = U.stride_for(JW)
    exp = noise(63, (JN, JH, stride))
    for k, j in enumerate(js):
        exp[k, :, :4 * JW] = O.jpeg_idct_color(j)[:, :4 * JW]
    bo, to = gbuf("decoded frames", noise(63, exp.shape), noise(64, exp.shape), exp, mask=row_mask(JN, JH, stride, JW))
    out = Bitmap(to.view(JN, -1), JW, JH, stride)
    stage = _pixel_stage(fx)
    return bufs + [bo], lambda: stage().read_frames(planes, qt, out) and None


def _decode_resample(fx, scale_num, tw, th, want_fused, w=JW, h=JH):
    js = _jpeg_cases(65 + scale_num + fx.get("variant", 0), w, h)
    bufs, planes, qt = _coefficient_buffers(js, _jpeg_cases(66, w, h))
    ow, oh = (w * scale_num + 7) // 8, (h * scale_num + 7) // 8
    cst = U.stride_for(tw)
    canvas0 = noise(67, (JN, th, cst))
    exp = canvas0.copy()
    for k, j in enumerate(js):
        dec = O.jpeg_idct_color_scaled(j, scale_num, 0)
        U.oracle_render(dec[None], ow, oh, exp[k:k + 1], tw, th, 0, 0, tw, th)
    bc, tc = gbuf("canvas", canvas0, noise(68, canvas0.shape), exp, mask=row_mask(JN, th, cst, tw))
    can = Bitmap(tc.view(JN, -1), tw, th, cst)
    info = ScaleAndRenderParams(0, 0, tw, th)
    stage = _pixel_stage(fx, scale_num, w, h)
    plan = _maker(fx, lambda: ResamplePlan(ow, oh, tw, th, Filter.Robidoux, 0.0))

    def call():
        fused = stage().read_frames_into(planes, qt, can, info, plan=plan())
        assert fused == want_fused, "the call took its %s form" % ("one-call" if fused else "two-step")
    return bufs + [bc], call


@row("jpeg_decode_resample two-step 40x24 -> 20x12", "ifhip_jpeg_decode_resample_batch_device")
def _(fx):
    return _decode_resample(fx, 8, 20, 12, False)


# The one-call form reads the component planes in the fused kernel's per-pixel form, which no 40 x 24 frame reaches
# (ifhip_describe_launch says so on the host); 160 x 96 at 4/8 -> 40 x 24 is the smallest 4:2:0 shape found that does.
@row("jpeg_decode_resample one call 160x96 at 4/8 -> 40x24", "ifhip_jpeg_decode_resample_batch_device")
def _(fx):
    return _decode_resample(fx, 4, 40, 24, True, 160, 96)


@row("scale_spatial_plane 6x4 blocks", "ifhip_scale_spatial_plane_device")
def _(fx):
    import ctypes as C
    from imageflow_amd.codecs import block_scalers as BS
    bw, bh, n, srgb = 6, 4, 4, 1                                     # the luma plane of a 4:2:0 40 x 24 frame, MCU padded
    real, decoy = noise(71, (8 * bh, 8 * bw)), noise(72, (8 * bh, 8 * bw))
    blocks = real.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    exp = O.scale_spatial_blocks(blocks, n, srgb).reshape(bh, bw, n, n).transpose(0, 2, 1, 3).reshape(bh * n, bw * n)
    bi, ti = gbuf("plane", real, decoy)
    bo, to = gbuf("scaled plane", noise(73, exp.shape), noise(74, exp.shape), exp)
    L = BS._bind()

    def call():
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        _native.check(L.ifhip_scale_spatial_plane_device(ti.data_ptr(), 8 * bw, bw, bh, n, srgb, to.data_ptr(), n * bw, st))
    return [bi, bo], call


def _entropy_files(seed):
    import io
    from PIL import Image
    from tests.test_jpeg_device_coder import photo
    out = []
    for k, kw in enumerate(({}, {"restart_marker_blocks": 3})):
        buf = io.BytesIO()
        Image.fromarray(photo(64, 48, seed + k)).save(buf, "JPEG", quality=85, subsampling="4:2:0", **kw)
        out.append(buf.getvalue())
    return out


def _entropy_outputs(files):
    js = [O.jpeg_read_coefficients(f) for f in files]
    bufs, planes = [], []
    for c in range(3):
        exp = np.stack([j["coef"][c] for j in js])
        b, t = gbuf("coefficients %d" % c, np.full(exp.shape, 0x5A5A, np.int16), np.full(exp.shape, 0x1111, np.int16), exp, dtype=torch.int16)
        bufs.append(b)
        planes.append(t.view(exp.shape))
    return bufs, planes


@row("jpeg_entropy_decode two 64x48 files, one with restart intervals", "ifhip_jpeg_entropy_decode_device", waits=True)
def _(fx):
    from imageflow_amd.codecs import mozjpeg_decoder as D
    files = _entropy_files(81)
    assert [D.get_image_info(f)["restart_interval"] for f in files] == [0, 3]
    bufs, planes = _entropy_outputs(files)
    ent = _maker(fx, lambda: D.JpegEntropyBatch(files, DEV))
    return bufs, lambda: ent().read_coefficients(planes) and None


@row("jpeg_prepared_upload on the caller's stream, then the batch", "ifhip_jpeg_prepared_upload", "ifhip_jpeg_entropy_decode_device", waits=True)
def _(fx):
    from imageflow_amd.codecs import mozjpeg_decoder as D
    files = _entropy_files(83)
    bufs, planes = _entropy_outputs(files)

    alive = []

    def call():
        alive.append(D.JpegEntropyBatch(files, DEV, prepared=True, upload_stream=torch.cuda.current_stream(DEV)))
        alive[-1].read_coefficients(planes)
    return bufs, call


# ---- JPEG: forward stage, trellis, the device entropy coder, the file gather -------------------------------------------------
def _trellis_frames(w, h, kinds):
    from imageflow_amd.graphics.bitmaps import get_stride
    from tests import jpeg_trellis_emu as E
    stride = get_stride(w)
    host = np.zeros((len(kinds), h, stride), np.uint8)
    for i, k in enumerate(kinds):
        host[i, :, :4 * w] = E.frame(k, w, h).reshape(h, 4 * w)
    return host, stride


def _plane_outputs(expected, fill):
    bufs, planes = [], []
    for c in range(3):
        b, t = gbuf("planes %d" % c, np.full(expected[c].shape, fill, np.int16), np.full(expected[c].shape, 0x1111, np.int16), expected[c],
                    dtype=torch.int16)
        bufs.append(b)
        planes.append(t.view(expected[c].shape))
    return bufs, planes


def _tables(quality, n):
    from imageflow_amd.codecs import mozjpeg as MJ
    return np.stack([MJ.quant_tables_for_quality(quality)] * n)


def _forward(fx, w, h, raw):
    from imageflow_amd.codecs import mozjpeg as MJ
    from tests import jpeg_trellis_emu as E
    kinds = ("photo", "noise")
    real, stride = _trellis_frames(w, h, kinds)
    decoy, _ = _trellis_frames(w, h, ("noise", "flat"))
    qt = _tables(75, 2)
    if raw:
        exp = [np.stack([E.reference(k, w, h, 75)["raw"][c] for k in kinds]) for c in range(3)]
    else:
        per = [O.jpeg_forward(real[i], w, h, stride, list(S420[0]), list(S420[1]), qt[i]) for i in range(2)]
        exp = [np.stack([p[c] for p in per]) for c in range(3)]
    bi, ti = gbuf("frames", real, decoy)
    bq, tq = gbuf("quantisation tables", qt, _tables(50, 2), dtype=torch.int16)
    bufs, planes = _plane_outputs(exp, 0x5A5A)
    bm = Bitmap(ti.view(2, -1), w, h, stride)
    stage = _maker(fx, lambda: MJ.JpegForwardStage(w, h, S420[0], S420[1], 2, DEV))
    return [bi, bq] + bufs, lambda: stage().write_frames(bm, tq, coef=planes, raw=raw) and None


def _trellis(fx, w, h):
    from imageflow_amd.codecs import mozjpeg as MJ
    from tests import jpeg_trellis_emu as E
    kinds, others = ("photo", "noise"), ("noise", "flat")
    ins, raws = [], []
    for c in range(3):
        real = np.stack([E.reference(k, w, h, 75)["raw"][c] for k in kinds])
        b, t = gbuf("raw planes %d" % c, real, np.stack([E.reference(k, w, h, 75)["raw"][c] for k in others]), dtype=torch.int16)
        ins.append(b)
        raws.append(t.view(real.shape))
    bq, tq = gbuf("quantisation tables", _tables(75, 2), _tables(50, 2), dtype=torch.int16)
    exp = [np.stack([E.reference(k, w, h, 75)["coef"][c] for k in kinds]) for c in range(3)]
    bufs, planes = _plane_outputs(exp, 0x5A5A)
    stage = MJ.JpegTrellisStage(w, h, S420[0], S420[1], 2, DEV)
    return ins + [bq] + bufs, lambda: stage.quantize(raws, tq, coef=planes) and None


def file_outputs(expected_files, pitch, whole=False):
    """files [n, pitch], lengths [n] and status [n] of a coder, pre-filled late; the bytes behind a file's length are compared
    only where the entry point promises them (whole: zeros)"""
    n = len(expected_files)
    exp = np.full((n, pitch), 0x5C, np.uint8) if not whole else np.zeros((n, pitch), np.uint8)
    mask = np.zeros((n, pitch), bool)
    for i, f in enumerate(expected_files):
        assert len(f) <= pitch
        exp[i, :len(f)] = np.frombuffer(f, np.uint8)
        mask[i, :len(f)] = True
    bf, tf = gbuf("files", np.full((n, pitch), 0x5C, np.uint8), np.full((n, pitch), 0x3C, np.uint8), exp, mask=None if whole else mask)
    bl, tl = gbuf("lengths", np.full(n, -7, np.int32), np.full(n, -8, np.int32), np.array([len(f) for f in expected_files], np.int32), dtype=torch.int32)
    bs, ts = gbuf("status", np.full(n, -9, np.int32), np.full(n, -10, np.int32), np.zeros(n, np.int32), dtype=torch.int32)
    return [bf, bl, bs], tf.view(n, pitch), tl, ts


def _jpeg_twins(w, h, seeds, quality):
    from tests.test_jpeg_device_coder import photo
    from tests.test_jpeg_device_coder_progressive import twin
    imgs = [photo(w, h, s) for s in seeds]
    return imgs, [twin(img, quality, "4:2:0") for img in imgs]


def _jpeg_encode(fx, w, h, flags):
    import ctypes as C
    from imageflow_amd.codecs import mozjpeg as MJ
    from tests.test_jpeg_device_coder_progressive import FLAGS, save
    q = 85
    imgs, js = _jpeg_twins(w, h, (91, 92), q)
    _, other = _jpeg_twins(w, h, (93, 94), q)
    ins, planes = [], []
    for c in range(3):
        real = np.stack([np.ascontiguousarray(j["coef"][c], np.int16) for j in js])
        b, t = gbuf("coefficients %d" % c, real, np.stack([np.ascontiguousarray(j["coef"][c], np.int16) for j in other]), dtype=torch.int16)
        ins.append(b)
        planes.append(t)
    want = [save(img, q, "4:2:0", **(FLAGS[flags] if flags else {"optimize": False})) for img in imgs]
    j0 = js[0]
    stage = _maker(fx, lambda: MJ.JpegEntropyStage(w, h, j0["hs"], j0["vs"], j0["bw"], j0["bh"], 2, DEV))
    pitch = (stage().max_file_bytes_for(bool(flags & 2), bool(flags & 1)) + 15) // 16 * 16
    outs, files, lengths, status = file_outputs(want, pitch)
    L = MJ._bind()

    def call():
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        head = (stage()._h, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), q)     # (_maker keeps a fresh stage alive)
        tail = (2, files.data_ptr(), pitch, lengths.data_ptr(), status.data_ptr(), st)
        if flags:
            _native.check(L.ifhip_jpeg_encode_flags_batch_device(*head, flags, *tail))
        else:
            _native.check(L.ifhip_jpeg_encode_batch_device(*head, *tail))
    return ins + outs, call


def _pack_files(fx, w, h):
    from imageflow_amd.codecs import mozjpeg as MJ
    from tests.test_jpeg_device_coder_progressive import save
    from tests.test_jpeg_device_coder import photo
    real = [save(photo(w, h, s), 85, "4:2:0", optimize=False) for s in (95, 96, 97)]
    decoy = [save(photo(w, h, s), 60, "4:2:0", optimize=False) for s in (98, 99, 100)]
    n = 3
    pitch = (max(len(f) for f in real + decoy) + 15) // 16 * 16 + 16

    def slots(files):
        a = np.zeros((n, pitch), np.uint8)
        for i, f in enumerate(files):
            a[i, :len(f)] = np.frombuffer(f, np.uint8)
        return a, np.array([len(f) for f in files], np.int32)
    (rf, rl), (df, dl) = slots(real), slots(decoy)
    bf, tf = gbuf("files", rf, df)
    bl, tl = gbuf("lengths", rl, dl, dtype=torch.int32)
    offsets, exp, mask, at = np.zeros(n + 1, np.int64), np.full(n * pitch, 0x5C, np.uint8), np.zeros(n * pitch, bool), 0
    for i, f in enumerate(real):                                    # the header's rule: every start rounded up to 16 bytes
        offsets[i] = at
        exp[at:at + len(f)] = np.frombuffer(f, np.uint8)
        mask[at:at + len(f)] = True
        at = (at + len(f) + 15) // 16 * 16
    offsets[n] = at
    bo, to = gbuf("packed", np.full(n * pitch, 0x5C, np.uint8), np.full(n * pitch, 0x3C, np.uint8), exp, mask=mask)
    bx, tx = gbuf("offsets", np.full(n + 1, -7, np.int64), np.full(n + 1, -8, np.int64), offsets, dtype=torch.int64)
    files = tf.view(n, pitch)

    def call():
        got_out, got_offsets = MJ.pack_files_device(files, tl, out=to)
        assert got_out is to
        tx.copy_(got_offsets, non_blocking=True)                    # (the wrapper makes the offsets on the current stream)
    return [bf, bl, bo, bx], call


for _w, _h in ((33, 31), (257, 17)):
    _size = "%dx%d" % (_w, _h)
    row("jpeg_forward " + _size, "ifhip_jpeg_forward_batch_device")(lambda fx, w=_w, h=_h: _forward(fx, w, h, False))
    row("jpeg_forward_raw " + _size, "ifhip_jpeg_forward_raw_batch_device")(lambda fx, w=_w, h=_h: _forward(fx, w, h, True))
    row("jpeg_trellis " + _size, "ifhip_jpeg_trellis_batch_device")(lambda fx, w=_w, h=_h: _trellis(fx, w, h))
    row("jpeg_encode baseline " + _size, "ifhip_jpeg_encode_batch_device")(lambda fx, w=_w, h=_h: _jpeg_encode(fx, w, h, 0))
    for _flags, _what in ((1, "optimised tables"), (2, "progressive"), (3, "progressive, optimised tables")):
        row("jpeg_encode_flags %s %s" % (_what, _size), "ifhip_jpeg_encode_flags_batch_device")(
            lambda fx, w=_w, h=_h, f=_flags: _jpeg_encode(fx, w, h, f))
    row("pack_files " + _size, "ifhip_pack_files_device")(lambda fx, w=_w, h=_h: _pack_files(fx, w, h))


# ---- the file coders: PNG, palette PNG, lossless WebP, GIF -------------------------------------------------------------------
def _file_coder(fx, name, w, h):
    from tests import png_quantize_emu as Q
    from tests import test_encode_handoff as EH
    stride = 4 * w + 8
    rgba = EH.frames_of(w, h) if (w, h) != (129, 128) else EH.frames_of(w, h)[:1]
    other = [Q.photo_rgba(w, h, seed=77, alpha=True), np.random.default_rng(78).integers(0, 256, (h, w, 4), dtype=np.uint8)][:len(rgba)]
    n = len(rgba)
    bi, ti = gbuf("frames", np.stack([Q.bgra_rows(f, stride) for f in rgba]), np.stack([Q.bgra_rows(f, stride) for f in other]))
    want = [EH.emulated(name, f, stride) for f in rgba]
    stage = EH.new_stage(name, w, h, n)
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    outs, files, lengths, status = file_outputs(want, pitch, whole=name == "webp")
    L = EH.Coder(name).L
    frames, fb = ti.data_ptr(), h * stride
    out = (files.data_ptr(), pitch, lengths.data_ptr(), status.data_ptr())
    args = {"png": (L.ifhip_png_encode_batch_device, stage._h, frames, fb, stride, n, 6, *out),
            "pngquant": (L.ifhip_png_quantize_batch_device, stage._h, frames, fb, stride, 1, n, -1, -1, -1, 256, 1, 6, *out, None, None, None),
            "webp": (L.ifhip_webp_encode_batch_device, stage._h, frames, fb, stride, n, *out),
            "gif": (L.ifhip_gif_encode_batch_device, stage._h, frames, fb, stride, 1, n, -1, 0, 0, *out, None, None)}[name]
    return [bi] + outs, lambda: stage._on_stream(*args)


row("png_encode 33x31", "ifhip_png_encode_batch_device")(lambda fx: _file_coder(fx, "png", 33, 31))
row("png_quantize 33x31", "ifhip_png_quantize_batch_device")(lambda fx: _file_coder(fx, "pngquant", 33, 31))
row("webp_encode 33x31", "ifhip_webp_encode_batch_device")(lambda fx: _file_coder(fx, "webp", 33, 31))
row("gif_encode 33x31", "ifhip_gif_encode_batch_device")(lambda fx: _file_coder(fx, "gif", 33, 31))
row("gif_encode 129x128, a second LZW segment", "ifhip_gif_encode_batch_device")(lambda fx: _file_coder(fx, "gif", 129, 128))


@row("gif_encode_animation 33x31, two frames", "ifhip_gif_encode_animation_device", waits=True)
def _(fx):
    import ctypes as C
    from imageflow_amd.codecs import gif_encoder
    from tests import gif_animation_emu as A
    from tests import png_quantize_emu as Q
    w, h, n, delays, user, repeat = 33, 31, 2, [5, 7], [False, True], 0
    rgba, other = A.photo_frames(w, h, n, True), A.photo_frames(w, h, n, True, seed=9)
    want = A.assemble(rgba, True, delays, user, repeat)[0]
    bi, ti = gbuf("frames", np.stack([Q.bgra_rows(f) for f in rgba]), np.stack([Q.bgra_rows(f) for f in other]))
    stage = gif_encoder.GifEncodeStage(w, h, n, DEV)
    capacity = (stage.max_animation_bytes(n) + 3) // 4 * 4
    exp, mask = np.full(capacity, 0x5C, np.uint8), np.zeros(capacity, bool)
    exp[:len(want)] = np.frombuffer(want, np.uint8)
    mask[:len(want)] = True
    bf, tf = gbuf("file", np.full(capacity, 0x5C, np.uint8), np.full(capacity, 0x3C, np.uint8), exp, mask=mask)
    bl, tl = gbuf("length", np.full(1, -7, np.int32), np.full(1, -8, np.int32), np.array([len(want)], np.int32), dtype=torch.int32)
    bs, ts = gbuf("status", np.full(1, -9, np.int32), np.full(1, -10, np.int32), np.zeros(1, np.int32), dtype=torch.int32)
    d, u = (C.c_uint32 * n)(*delays), (C.c_uint8 * n)(*[int(v) for v in user])
    fn = gif_encoder._bind().ifhip_gif_encode_animation_device
    return [bi, bf, bl, bs], lambda: stage._on_stream(fn, stage._h, ti.data_ptr(), h * 4 * w, 4 * w, 1, n, repeat, d, u, tf.data_ptr(), capacity,
                                                      tl.data_ptr(), ts.data_ptr())


# ---- the file decoders: two good files around a damaged one; the 0xA5 pre-fill of the frames arrives late ----------------------
def _decoder_files(name, variant=0):
    """-> [(file, the oracle's BGRA [h, w, 4] or None for the damaged one, its status word)] and the front end's batch call"""
    from imageflow_amd.codecs import gif_decoder, libpng_decoder, webp_decoder
    if name == "png":
        import zlib
        from tests import png_decode_oracle as PO
        from tests.test_decode_handoff import png_file
        good = [png_file(2, 8, 37 + variant, 23), png_file(6, 8, 7, 5 + variant)]
        stream = PO.filtered_stream(np.zeros((70, 5, 3), np.uint32), 2, 8, 0)
        stream = stream[:16 * 66] + b"\x05" + stream[16 * 66 + 1:]                            # row 66's filter byte: "bad adaptive filter value"
        bad = (PO.write_png(np.zeros((70, 5, 3), np.uint32), 2, 8, z=zlib.compress(stream)), None, 10)
        return [(good[0], PO.decode(good[0])[0], 0), bad, (good[1], PO.decode(good[1])[0], 0)], libpng_decoder._bind().ifhip_png_decode_batch_device, libpng_decoder.png_info
    if name == "webp":
        from tests import webp_decode_fixtures as WX
        names = ("w17", "1x1") if not variant else ("1x1", "w17")
        data, status = WX.damaged_files(library=True)["truncated_40"]
        return ([(WX.good_files()[names[0]], WX.expected_bgra(names[0])[0], 0), (data, None, status),
                 (WX.good_files()[names[1]], WX.expected_bgra(names[1])[0], 0)], webp_decoder._bind().ifhip_webp_decode_batch_device, webp_decoder.webp_info)
    from tests import gif_fixtures as GX
    names = ("m4_noise", "size_1x1") if not variant else ("size_1x1", "m4_noise")
    data, _, status = GX.damaged_files()["too_little_cut"]
    return ([(GX.good_files()[names[0]][0], GX.expected(names[0]), 0), (data, None, status),
             (GX.good_files()[names[1]][0], GX.expected(names[1]), 0)], gif_decoder._bind().ifhip_gif_decode_batch_device, gif_decoder.gif_info)


def _file_decoder(fx, name):
    from imageflow_amd.graphics.bitmaps import get_stride
    import ctypes as C
    cases, batch_fn, info_of = _decoder_files(name, fx.get("variant", 0))
    bufs, frames = [], []
    for i, (data, want, status) in enumerate(cases):
        info = info_of(data)
        w, h = info["width"], info["height"]
        stride = get_stride(w) + 16
        exp = np.full((h, stride), 0xA5, np.uint8)
        if want is not None:
            assert want.shape == (h, w, 4), (name, i)
            exp[:, :4 * w] = want.reshape(h, 4 * w)
        b, t = gbuf("frame of file %d" % i, np.full((h, stride), 0xA5, np.uint8), np.full((h, stride), 0x3C, np.uint8), exp)
        bufs.append(b)
        frames.append(Bitmap(t.view(1, -1), w, h, stride, alpha_meaningful=True))
    files, words = [c[0] for c in cases], [c[2] for c in cases]
    assert words[1] != 0
    n = len(files)
    bs, ts = gbuf("status", np.full(n, -9, np.int32), np.full(n, -10, np.int32), np.array(words, np.int32), dtype=torch.int32)
    keep = [np.frombuffer(f, np.uint8) for f in files]
    ptrs, lens = (C.c_void_p * n)(*[k.ctypes.data for k in keep]), (C.c_size_t * n)(*[k.size for k in keep])
    d_frames = (C.c_void_p * n)(*[f.data.data_ptr() for f in frames])
    frame_bytes = (C.c_size_t * n)(*[f.data.shape[1] for f in frames])
    strides = (C.c_uint32 * n)(*[f.stride for f in frames])
    lead = (None,) if name == "gif" else ()                          # GIF's frame_index array: frame 0 of every file

    def call():
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        _native.check(batch_fn(ptrs, lens, n, *lead, d_frames, frame_bytes, strides, ts.data_ptr(), st))
    call.keep = keep
    return bufs + [bs], call


row("png_decode two files around a damaged one", "ifhip_png_decode_batch_device", waits=True)(lambda fx: _file_decoder(fx, "png"))
row("webp_decode two files around a damaged one", "ifhip_webp_decode_batch_device", waits=True)(lambda fx: _file_decoder(fx, "webp"))
row("gif_decode two files around a damaged one", "ifhip_gif_decode_batch_device", waits=True)(lambda fx: _file_decoder(fx, "gif"))


def _gif_screens(fx, damaged):
    import ctypes as C
    from imageflow_amd.codecs import gif_decoder
    from imageflow_amd.graphics.bitmaps import get_stride
    from tests import gif_fixtures as GX
    if damaged:
        data, _, word = GX.damaged_files()["second_frame_damaged"]
        n, wants = 2, None
    else:
        data, word = GX.rgb_animation(), 0
        wants = [GX.expected("rgb_animation_frame%d" % k) for k in range(3)]
        n = len(wants)
    info = gif_decoder.gif_info(data)
    w, h = info["width"], info["height"]
    stride = get_stride(w) + 16
    exp = np.full((n, h, stride), 0xA5, np.uint8)
    if wants:
        for k, want in enumerate(wants):
            exp[k, :, :4 * w] = want.reshape(h, 4 * w)
    b, t = gbuf("screens", np.full(exp.shape, 0xA5, np.uint8), np.full(exp.shape, 0x3C, np.uint8), exp)
    bs, ts = gbuf("status", np.full(1, -9, np.int32), np.full(1, -10, np.int32), np.array([word], np.int32), dtype=torch.int32)
    buf = np.frombuffer(data, np.uint8)
    fn = gif_decoder._bind().ifhip_gif_decode_frames_device

    def call():
        written = C.c_uint32(77)
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        _native.check(fn(buf.ctypes.data, buf.size, t.data_ptr(), h * stride, stride, n, ts.data_ptr(), C.byref(written), st))
        assert written.value == (0 if damaged else n)
    return [b, bs], call


row("gif_decode_frames three screens", "ifhip_gif_decode_frames_device", waits=True)(lambda fx: _gif_screens(fx, False))
row("gif_decode_frames a damaged second frame", "ifhip_gif_decode_frames_device", waits=True)(lambda fx: _gif_screens(fx, True))


# ---- the tests -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROWS))
def test_entry_point_follows_a_late_stream(name, streams, debug_switch):
    S, W = streams
    bufs, call = ROWS[name][1]({"debug_switch": debug_switch})
    entry = SO.check_late(name, bufs, call, S, W)
    print("stream-order", entry)
    assert entry["checks"] == "a b c"
    assert entry["blocking"] == ROWS[name][2], "the call %s" % ("returned with the window open: the header lists it among those that wait"
                                                                if ROWS[name][2] else "waited on the host for its stream")


# Every row whose scratch comes from the block cache FOR its stream and goes back behind it (devmem.cpp cached_malloc_for_stream,
# cached_free_after) in a call that returns with its stream still held up.  The three file decoders and the GIF animation coder
# release a block behind their stream too (decode_handoff.hpp StagedBlock), but they wait for the stream before their first
# launch: on return the stream is drained, the block's event completes within microseconds, and whether the next caller finds
# it parked or free is a matter of the clock that no counter can pin.
CACHED_SCRATCH_ROWS = ["scale_and_render generic pair 101x67->33x21", "white_balance 67x33 with scratch histograms", "detect_content 67x33",
                       "jpeg_decode_resample two-step 40x24 -> 20x12"]


@pytest.mark.parametrize("name", CACHED_SCRATCH_ROWS)
def test_scratch_released_behind_a_late_stream_is_not_handed_to_another_stream(name, streams, debug_switch):
    """The cache's counters while S is held up: the scratch of a call on S is parked behind S; the same call on W gets none of
    it (it allocates from the driver); the next call on S gets it at once.  The scratch of these calls is written before it is
    read, so a block handed over too early would not change their pixels: the counters are the proof, the pixels of both
    calls are compared besides.  A resample plan is shared between the two streams (the header calls it shareable); stages
    are one per stream.  No device-wide wait may be what keeps the streams apart."""
    import gc
    S, W = streams
    bufs_a, call_a = ROWS[name][1]({"debug_switch": debug_switch, "variant": 0})
    bufs_b, call_b = ROWS[name][1]({"debug_switch": debug_switch, "variant": 1})
    gc.collect()                                                    # (objects of earlier tests free their blocks now, not inside the window)
    before = _native.cache_stats()
    print("stream-order", SO.check_two_streams(name, bufs_a, call_a, bufs_b, call_b, S, W, _native.cache_stats, _native.trim_cache))
    after = _native.cache_stats()
    assert after["device_wide_syncs"] == before["device_wide_syncs"], (before, after)


# Objects of the library that upload or clear on the thread's stream when they are created.
# row -> the call waits on the host for S with the thread's stream (set to S, left at the null stream): a plan uploads its
# tables when it is created, a pixel stage uploads nothing, an encode stage's first call sends its marker segments behind a
# wait for the caller's stream, the entropy decode synchronises its stream.
THREAD_STREAM_ROWS = {"scale_and_render generic pair 101x67->33x21": (True, False), "jpeg_idct_color 4:2:0 40x24": (False, False),
                      "jpeg_encode baseline 33x31": (True, True),
                      "jpeg_entropy_decode two 64x48 files, one with restart intervals": (True, True)}


@pytest.mark.parametrize("thread_stream", ["S", "the null stream"])
@pytest.mark.parametrize("name", THREAD_STREAM_ROWS)
def test_objects_created_inside_the_window_are_ready_for_the_callers_stream(name, thread_stream, streams, debug_switch):
    """A resample plan, a JPEG pixel stage, an encode stage and an entropy handle, created by the call itself while S is held
    up and used on S at once: with ifhip_set_thread_stream(S), as a host with one job per thread does it, and with the thread
    stream left at the null stream."""
    S, W = streams
    fx = {"debug_switch": debug_switch, "create_in_call": True}
    bufs, call = ROWS[name][1](fx)
    call_ms = SO.plain_run(name, bufs, call)
    try:
        if thread_stream == "S":
            _native.set_thread_stream(S)
        entry = SO.check_late("%s, created in the call on %s" % (name, thread_stream), bufs, call, S, W, call_ms=call_ms)
    finally:
        _native.set_thread_stream(None)
        torch.cuda.synchronize()
        fx.get("keep", []).clear()
    print("stream-order", entry)
    assert entry["checks"] == "a b c"
    assert entry["blocking"] == THREAD_STREAM_ROWS[name][0 if thread_stream == "S" else 1]


def _stand_in_buffers():
    real, decoy = noise(1, 4096), noise(2, 4096)
    bi, ti = gbuf("input", real, decoy)
    bo, to = gbuf("output", noise(3, 4096), noise(4, 4096), real)
    return [bi, bo], ti, to


def test_the_harness_reports_a_call_that_leaves_the_stream(streams):
    """A stand-in 'library call' made of torch ops that copies on W without waiting for S: it reads the decoy."""
    S, W = streams
    bufs, ti, to = _stand_in_buffers()

    def right_stream():
        to.copy_(ti, non_blocking=True)
    good = SO.check_late("stand-in: copy on the caller's stream", bufs, right_stream, S, W)
    assert good["checks"] == "a b c" and not good["blocking"] and good["witnesses"] == 3

    def wrong_stream():
        with torch.cuda.stream(W):
            to.copy_(ti, non_blocking=True)
    SO.plain_run("stand-in: copy on W", bufs, wrong_stream)                   # right bytes when nothing is late
    with pytest.raises(SO.StreamOrderError, match="wrong only when late"):
        SO.check_late("stand-in: copy on W", bufs, wrong_stream, S, W, call_ms=0.1)


def test_the_harness_reports_work_that_finishes_behind_the_scribble(streams):
    """A stand-in that copies on S, but behind an event recorded after the scribble: check (b)."""
    S, W = streams
    bufs, ti, to = _stand_in_buffers()

    def deferring():
        def later():
            ev = torch.cuda.Event()
            ev.record(S)
            S.wait_event(ev)
            to.copy_(ti, non_blocking=True)
        return later
    with pytest.raises(SO.StreamOrderError, match="wrong only when late"):
        SO.check_late("stand-in: deferred copy", bufs, deferring, S, W, call_ms=0.1)


def _entry_points_with_a_stream():
    text = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = set()
    for decl in text.split(";"):
        m = re.search(r"\b(ifhip_\w+)\s*\(", decl)
        if m and re.search(r"\bvoid\s*\*\s*hip_stream\b", decl):
            found.add(m.group(1))
    return found


def test_every_entry_point_with_a_stream_has_a_row():
    """include/imageflow_hip.h, comments removed: every declaration with a `void* hip_stream` parameter is named by a row."""
    have = {e for eps, _, _ in ROWS.values() for e in eps}
    header = _entry_points_with_a_stream() - {"ifhip_set_thread_stream"}       # (no call to order: the thread-stream test above)
    assert len(header) >= 30, "the declarations of the header were not found"
    assert have == header, sorted(have ^ header)
