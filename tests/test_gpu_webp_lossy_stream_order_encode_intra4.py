"""Stream order of ifhip_webp_lossy_encode_batch_device on a stage with IFHIP_VP8_ENC_INTRA4, proven with late inputs (the harness:
tests/stream_order.py), as tests/test_gpu_webp_lossy_stream_order_encode.py proves it for a stage without flags: the flagged
stage launches vp8e_code4_kernel of csrc/vp8_encode_intra4.hip from another translation unit, and that launch too must be on
hip_stream.  (The file sorts behind that test on purpose: the harness draws its streams from torch's pool.)

Three frames of 33 x 31 in a stage with alpha; the middle one has alpha below 255.  The frames arrive late on the held-up stream
S over decoys of the same geometry, and so do the pre-fills of the files, the lengths and the status words: a launch that ran
ahead of S codes the decoy or is overwritten.  The call makes no host round trip: it must return with the window open."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd.codecs import webp_lossy_encoder as ENC  # noqa: E402
from tests import stream_order as SO  # noqa: E402
from tests import test_gpu_webp_lossy_stream_order_encode as BASE  # noqa: E402
from tests import vp8_encode_intra4_emu as E4  # noqa: E402
from tests import webp_frames as F  # noqa: E402

DEV = "cuda:0"
ROW = "webp_lossy_encode with IFHIP_VP8_ENC_INTRA4 33x31, three frames, one with alpha"
W, H, QUALITY = BASE.W, BASE.H, BASE.QUALITY


def test_the_flagged_lossy_coder_follows_a_late_stream():
    stride = 4 * W + 8
    frames = [F.photo(W, H, seed=71), F.photo(W, H, alpha=True, seed=72), F.noise(W, H, 73)]
    frames[2][..., 3] = 255
    decoys = [F.noise(W, H, 74), F.photo(W, H, seed=75), F.photo(W, H, alpha=True, seed=76)]
    coded = [E4.encode(f, QUALITY, True) for f in frames]
    want = [c[0] for c in coded]
    assert [w[12:16] for w in want] == [b"VP8 ", b"VP8X", b"VP8 "] and all(c[2]["n_i4"] > 0 for c in coded)
    n = len(frames)
    bi, ti = BASE.gbuf("frames", np.stack([BASE.rows_of(f, stride) for f in frames]), np.stack([BASE.rows_of(f, stride) for f in decoys]))
    stage = ENC.WebpLossyEncodeStage(W, H, True, n, DEV, intra4=True)
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    exp = np.zeros((n, pitch), np.uint8)                               # all of a file's pitch is written: zeros behind the file
    for i, f in enumerate(want):
        exp[i, :len(f)] = np.frombuffer(f, np.uint8)
    bf, tf = BASE.gbuf("files", np.full((n, pitch), 0x5C, np.uint8), np.full((n, pitch), 0x3C, np.uint8), exp)
    bl, tl = BASE.gbuf("lengths", np.full(n, -7, np.int32), np.full(n, -8, np.int32), np.array([len(f) for f in want], np.int32), dtype=torch.int32)
    bs, ts = BASE.gbuf("status", np.full(n, -9, np.int32), np.full(n, -10, np.int32), np.zeros(n, np.int32), dtype=torch.int32)
    fn = ENC._bind().ifhip_webp_lossy_encode_batch_device

    def call():
        stage._on_stream(fn, stage._h, ti.data_ptr(), H * stride, stride, n, float(QUALITY), tf.data_ptr(), pitch, tl.data_ptr(), ts.data_ptr())
    # as in the unflagged proof: a run the harness calls "window closed" proves nothing either way and is made again with the
    # next pair of streams, four times at the most; wrong bytes fail at once
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
