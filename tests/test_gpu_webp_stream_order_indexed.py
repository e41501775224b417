"""Stream order of ifhip_webp_encode_batch_device on a stage with IFHIP_WEBP_ENC_COLOR_INDEXING, proven with late inputs (the
harness: tests/stream_order.py), in the manner of the `webp_encode` row of tests/test_gpu_stream_order.py: the flagged stage
launches the kernels of csrc/webp_encode_indexed.hip and two more memsets around the plain coder's, and every one of them is
to follow the caller's stream.  (The file sorts behind the tests/test_gpu_webp_lossy_stream_order*.py files on purpose: the
harness draws its streams from torch's pool, and the lossy decoder's proof, which takes the first pair it is given, keeps
the draw it had.)

Three frames of 33 x 31 on one stage: five colours (indexed, two pixels a bundle), a photograph (more than 256 colours: the
count gives up and the file is the plain one), two colours (indexed, eight pixels a bundle).  The frames arrive late on the
held-up stream S over decoys of the same geometry whose kinds are the other way round, and so do the pre-fills of the files,
the lengths and the status words: a launch that ran ahead of S counts, bundles or codes the decoy, or is overwritten.  The call
makes no host round trip -- an image's packed shape stays on the device -- so it must return with the window open."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd.codecs import webp_encoder as WEBP  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import webp_frames as F  # noqa: E402
from tests import webp_indexed_emulation as E  # noqa: E402

DEV = "cuda:0"
GUARD = 0xA5
ROW = "webp_encode with colour indexing 33x31, indexed / plain / indexed"
W, H = 33, 31


def gbuf(name, real, decoy, expected=None, dtype=torch.uint8, guard=256):
    """a device buffer with a guard region behind it as one harness buffer -> (Buf, the data as a flat tensor of `dtype`)"""
    r, d = (np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in (real, decoy))
    assert r.size == d.size, name
    tail = np.full(guard, GUARD, np.uint8)
    e = None if expected is None else np.concatenate([np.ascontiguousarray(expected).reshape(-1).view(np.uint8), tail])
    t = torch.empty(r.size + guard, dtype=torch.uint8, device=DEV)
    return SO.Buf(name, t, np.concatenate([r, tail]), np.concatenate([d, tail]), e), t[:r.size].view(dtype)


def rows_of(bgra, stride):
    h, w, _ = bgra.shape
    out = np.full((h, stride), 0xA5, np.uint8)
    out[:, :4 * w] = bgra.reshape(h, 4 * w)
    return out


def test_the_flagged_stage_follows_a_late_stream():
    stride = 4 * W + 8
    frames = [F.few_colours(W, H, n=5), F.photo(W, H, seed=91), F.few_colours(W, H, n=2, seed=4)]
    decoys = [F.photo(W, H, seed=92), F.few_colours(W, H, n=9, seed=5), F.noise(W, H, 93)]
    emu = [E.encode(f, True, E.COLOR_INDEXING) for f in frames]
    want = [d for d, _ in emu]
    assert [st["indexed"] for _, st in emu] == [1, 0, 1]
    n = len(frames)
    bi, ti = gbuf("frames", np.stack([rows_of(f, stride) for f in frames]), np.stack([rows_of(f, stride) for f in decoys]))
    stage = WEBP.WebpEncodeStage(W, H, True, n, DEV, color_indexing=True)
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    exp = np.zeros((n, pitch), np.uint8)                               # all of a file's pitch is written: zeros behind the file
    for i, f in enumerate(want):
        exp[i, :len(f)] = np.frombuffer(f, np.uint8)
    bf, tf = gbuf("files", np.full((n, pitch), 0x5C, np.uint8), np.full((n, pitch), 0x3C, np.uint8), exp)
    bl, tl = gbuf("lengths", np.full(n, -7, np.int32), np.full(n, -8, np.int32), np.array([len(f) for f in want], np.int32), dtype=torch.int32)
    bs, ts = gbuf("status", np.full(n, -9, np.int32), np.full(n, -10, np.int32), np.zeros(n, np.int32), dtype=torch.int32)
    fn = WEBP._bind().ifhip_webp_encode_batch_device

    def call():
        stage._on_stream(fn, stage._h, ti.data_ptr(), H * stride, stride, n, tf.data_ptr(), pitch, tl.data_ptr(), ts.data_ptr())
    # A run that the harness itself calls "window closed" proves nothing either way (it "never passes unproven"): which torch
    # pool streams a process draws decides whether the witness stream runs beside the held-up one.  Such a run is made again
    # with the next pair of streams, four times at the most; wrong bytes fail at once.
    entry = None
    for attempt in range(4):
        try:
            S, Wd = SO.choose_streams(DEV)
            entry = SO.check_late(ROW, [bi, bf, bl, bs], call, S, Wd)
            break
        except SO.StreamOrderError as e:
            if "window closed" not in str(e) or attempt == 3:
                pytest.fail(str(e))
    print("stream-order", entry)
    assert entry["checks"] == "a b c"
    assert entry["blocking"] is False, "the call waited on the host: it is to be asynchronous on hip_stream, with no round trip"
