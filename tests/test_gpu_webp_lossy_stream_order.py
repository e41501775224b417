"""Stream order of ifhip_webp_lossy_decode_batch_device, proven with late inputs (the harness: tests/stream_order.py), in the
manner of the `webp_decode` row of tests/test_gpu_stream_order.py -- the proof that table would demand of the entry point,
which is declared in include/imageflow_hip_webp_lossy.h until the table gains its row.

Two good files around a damaged one; the first is a 56 x 40 RGBA file, so the alpha path (the VP8L reader's launches, the
alpha kernel) is in the window, and the damaged one's fault is found on the DEVICE, in its VP8L alpha stream.  The 0xA5
pre-fill of the frames arrives late on the held-up stream S: a kernel that ran ahead of S is overwritten by it, witnesses on
the null stream and on W see the decoy, and the call -- which sends its records ahead and waits for that copy, as the header
says of every file decoder -- is asserted to have waited on the host."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd import _native  # noqa: E402
from imageflow_amd.codecs import webp_lossy_decoder as D  # noqa: E402
from imageflow_amd.graphics.bitmaps import get_stride  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import webp_lossy_fixtures as X  # noqa: E402

DEV = "cuda:0"
GUARD = 0xA5
ROW = "webp_lossy_decode two files around a damaged one"


def gbuf(name, real, decoy, expected, dtype=torch.uint8, guard=256):
    """a device buffer with a guard region behind it as one harness buffer -> (Buf, the data as a flat tensor of `dtype`)"""
    r, d, e = (np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in (real, decoy, expected))
    assert r.size == d.size == e.size, name
    tail = np.full(guard, GUARD, np.uint8)
    t = torch.empty(r.size + guard, dtype=torch.uint8, device=DEV)
    return SO.Buf(name, t, np.concatenate([r, tail]), np.concatenate([d, tail]), np.concatenate([e, tail])), t[:r.size].view(dtype)


def test_the_lossy_decoder_follows_a_late_stream():
    try:
        S, W = SO.choose_streams(DEV)
    except SO.StreamOrderError as e:
        pytest.fail(str(e))
    damaged, _, word = X.damaged_files()["alph_stream_truncated"]
    cases = [(X.good_files()["rgba_56x40"], X.expected_bgra("rgba_56x40"), 0), (damaged, None, word),
             (X.good_files()["size_17x16"], X.expected_bgra("size_17x16"), 0)]
    assert word == X.ALPHA_STREAM and X.parts(cases[0][0])[1] is not None
    bufs, tensors, strides_ = [], [], []
    for i, (data, want, _) in enumerate(cases):
        info = D.webp_info(data)
        w, h = info["width"], info["height"]
        stride = get_stride(w) + 16
        exp = np.full((h, stride), 0xA5, np.uint8)
        if want is not None:
            assert want.shape == (h, w, 4), i
            exp[:, :4 * w] = want.reshape(h, 4 * w)
        b, t = gbuf("frame of file %d" % i, np.full((h, stride), 0xA5, np.uint8), np.full((h, stride), 0x3C, np.uint8), exp)
        bufs.append(b)
        tensors.append(t)
        strides_.append(stride)
    n = len(cases)
    bs, ts = gbuf("status", np.full(n, -9, np.int32), np.full(n, -10, np.int32), np.array([c[2] for c in cases], np.int32), dtype=torch.int32)
    keep = [np.frombuffer(c[0], np.uint8) for c in cases]
    ptrs, lens = (C.c_void_p * n)(*[k.ctypes.data for k in keep]), (C.c_size_t * n)(*[k.size for k in keep])
    d_frames = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    frame_bytes = (C.c_size_t * n)(*[t.numel() for t in tensors])
    strides = (C.c_uint32 * n)(*strides_)
    batch_fn = D._bind().ifhip_webp_lossy_decode_batch_device

    def call():
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        _native.check(batch_fn(ptrs, lens, n, d_frames, frame_bytes, strides, ts.data_ptr(), st))
    try:
        entry = SO.check_late(ROW, bufs + [bs], call, S, W)
    except SO.StreamOrderError as e:
        pytest.fail(str(e))
    print("stream-order", entry)
    assert entry["checks"] == "a b c"
    assert entry["blocking"] is True, "the call returned with the window open: it sends its records ahead and is to wait for that copy"
