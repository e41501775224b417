"""Stream order of ifhip_jpeg_progressive_decode_batch_device, proven with late inputs (the harness: tests/stream_order.py), in
the manner of tests/test_gpu_webp_lossy_stream_order.py -- the proof tests/test_gpu_stream_order.py's table would demand of
the entry point, which is declared in include/imageflow_hip_jpeg_progressive.h until the table gains its row.

Three files of different sizes, samplings and level depths, the middle one damaged inside a scan (its fault is found on the
DEVICE; its planes are undefined and only the guard behind them is compared).  The 0xA5 pre-fill of the planes arrives late on
the held-up stream S: a clear or a level's launch that ran ahead of S is overwritten by it, witnesses on the null stream and
on W see the decoy, and the call -- which sends its records ahead and waits for that copy, as the header says -- is asserted
to have waited on the host."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd import _native  # noqa: E402
from imageflow_amd.codecs import jpeg_progressive_decoder as D  # noqa: E402
from tests import jpeg_prog_fixtures as X  # noqa: E402
from tests import stream_order as SO  # noqa: E402

DEV = "cuda:0"
GUARD = 256
ROW = "jpeg_progressive_decode two files around a damaged one"


def test_the_progressive_decoder_follows_a_late_stream():
    try:
        S, W = SO.choose_streams(DEV)
    except SO.StreamOrderError as e:
        pytest.fail(str(e))
    damaged = X.damaged_files()
    emu = dict(zip(sorted(damaged), X.emulate_batch([damaged[n] for n in sorted(damaged)])))
    bad = [n for n in sorted(damaged) if emu[n][0] == 0 and emu[n][1] != 0][0]
    files = X.accepted_files()
    cases = [("odd_24x24_420", files["odd_24x24_420"], 0), (bad, damaged[bad], emu[bad][1]),
             ("pillow_100x75_444_q90_rst1", files["pillow_100x75_444_q90_rst1"], 0)]
    prepared = [D.PreparedProgressive(c[1]) for c in cases]
    assert prepared[0].n_levels == 4 and prepared[2].n_levels == 3
    bufs, ptrs, sizes = [], [[], [], []], []
    for i, (name, _, word) in enumerate(cases):
        p = prepared[i]
        want = None if word else X.host_planes(name)[1]
        for c in range(3):
            if c >= p.ncomp:
                ptrs[c].append(None)
                sizes.append(0)
                continue
            nbytes = int(np.prod(p.plane_shape(c))) * 2
            t = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
            tail = np.full(GUARD, 0xA5, np.uint8)
            real, decoy = np.full(nbytes + GUARD, 0xA5, np.uint8), np.concatenate([np.full(nbytes, 0x3C, np.uint8), tail])
            if want is None:
                exp, mask = real, np.concatenate([np.zeros(nbytes, bool), np.ones(GUARD, bool)])
            else:
                exp, mask = np.concatenate([np.ascontiguousarray(want[c]).reshape(-1).view(np.uint8), tail]), None
            bufs.append(SO.Buf("plane %d of file %d" % (c, i), t, real, decoy, exp, mask=mask))
            ptrs[c].append(t.data_ptr())
            sizes.append(nbytes)
    n = len(cases)
    ts = torch.empty(n + GUARD // 4, dtype=torch.int32, device=DEV)
    tail = np.full(GUARD // 4, -1515870811, np.int32)                       # 0xA5A5A5A5
    bufs.append(SO.Buf("status", ts, np.concatenate([np.full(n, -9, np.int32), tail]), np.concatenate([np.full(n, -10, np.int32), tail]),
                       np.concatenate([np.array([c[2] for c in cases], np.int32), tail])))
    handles = (C.c_void_p * n)(*[p.handle.value for p in prepared])
    coef = [(C.c_void_p * n)(*ptrs[c]) for c in range(3)]
    plane_bytes = (C.c_size_t * (3 * n))(*sizes)
    batch_fn = D._bind().ifhip_jpeg_progressive_decode_batch_device

    def call():
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        _native.check(batch_fn(handles, n, coef[0], coef[1], coef[2], plane_bytes, ts.data_ptr(), st))
    try:
        entry = SO.check_late(ROW, bufs, call, S, W)
    except SO.StreamOrderError as e:
        pytest.fail(str(e))
    finally:
        # torch hands out its 32 pooled streams per device in turn and choose_streams took 8 of them: take the other 24, so that
        # the stream-order tests that run after this file are handed the very streams they were handed before it existed
        # (which pooled streams share a hardware queue is what their witnesses depend on)
        _ = [torch.cuda.Stream(DEV) for _ in range(24)]
    print("stream-order", entry)
    assert entry["checks"] == "a b c"
    assert entry["blocking"] is True, "the call returned with the window open: it sends its records ahead and is to wait for that copy"
