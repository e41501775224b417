"""The device lossy WebP coder with IFHIP_VP8_ENC_INTRA4 on an MI355X (vp8e_code4_kernel of csrc/vp8_encode_intra4.hip behind
imageflow_amd.codecs.webp_lossy_encoder's intra4=True and behind the switch value 2 of Context.set_webp_lossy_encoder): every file
equals the CPU emulation's (tests/vp8_encode_intra4_emulate.cpp, whose files libwebp decodes to the emulation's own
reconstruction in tests/test_vp8_encode_intra4_core.py) byte for byte, in every batch position; guard regions stay untouched and
a pitch one byte short drops that image alone; the device's own lossy decoder reads the file back; switch value 1 still writes
the 16x16 coder's file."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import webp_lossy_encoder as ENC  # noqa: E402
from tests import test_gpu_webp_lossy_encode as OLD  # noqa: E402
from tests import vp8_encode_emu as E  # noqa: E402
from tests import vp8_encode_intra4_emu as E4  # noqa: E402
from tests import webp_frames as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = E4.frames()
# one macroblock with every neighbour outside the frame; two columns (above-right exists for column 0 only); three columns (the
# wavefront's first real overlap); one column and eight partitions; alpha; B_PRED beside 16x16 in both directions
NAMES = ["1x1", "16x16", "17x33", "48x32", "16x144", "alpha_90x61", "mix_64x48", "mix_cols_80x32"]
_EMULATED = {}


def emulated(bgra, quality, alpha, key=None, flags=E4.INTRA4):
    """the emulation's file of a frame, the BGRA it expects of a decoder and its stats, computed once per key"""
    if key is None or key not in _EMULATED:
        data, expect, st = E4.encode(bgra, quality, alpha, flags)
        assert st["errors"] == 0
        if key is None:
            return data, expect, st
        _EMULATED[key] = (data, expect, st)
    return _EMULATED[key]


def encode(frames, quality, alpha=True, intra4=True, **kw):
    """files and status words of BGRA frames [n, h, w, 4] of one geometry"""
    n, h, w, _ = frames.shape
    stage = ENC.WebpLossyEncodeStage(w, h, alpha, n, DEV, intra4=intra4)
    return stage.encode(OLD.bitmap(np.stack([OLD.rows_of(f) for f in frames]), w, h, alpha), quality, **kw)


@pytest.mark.parametrize("quality", E4.QUALITIES)
@pytest.mark.parametrize("name", NAMES)
def test_device_file_equals_the_flagged_emulations_byte_for_byte(name, quality):
    frame, alpha = FRAMES[name]
    files, status = encode(frame[None], quality, alpha)
    assert status == [0]
    want, _, st = emulated(frame, quality, alpha, (name, quality))
    assert len(files[0]) == len(want) and files[0] == want, (name, quality, st["n_i4"])


@pytest.mark.parametrize("n", [1, 3, 5])
def test_batches_of_mixed_content_give_equal_bytes_in_every_position(n):
    w, h = 80, 48                                                   # 5 x 3 macroblocks: seven steps of the skew-2 wavefront, two partitions
    kinds = {"a": F.photo(w, h, alpha=True, seed=21), "b": E4.mix(5, 3, lambda x, y: (x + 2 * y) % 3 != 0, 22), "c": F.one_colour(w, h, (9, 8, 7, 255))}
    order = "abaca"[:n]
    files, status = encode(np.stack([kinds[k] for k in order]), 75)
    assert status == [0] * n
    for k, data in zip(order, files):
        want, _, st = emulated(kinds[k], 75, True, ("batch", k))
        assert data == want, (n, k)
    assert 0 < emulated(kinds["b"], 75, True, ("batch", "b"))[2]["n_i4"] < 15
    assert files[0][12:16] == b"VP8X" and (n < 2 or files[1][12:16] == b"VP8 ")
    again, _ = encode(np.stack([kinds[k] for k in order]), 75)
    assert again == files, "the same pixels give the same bytes on every run"


def test_guard_regions_and_file_overflow():
    w, h, n, q = 80, 48, 3, 90
    frames = np.stack([F.photo(w, h, seed=31), E4.mix(5, 3, lambda x, y: True, 32), F.photo(w, h, seed=33)])
    frames[..., 3] = 255
    want = [emulated(f, q, True)[0] for f in frames]
    stage = ENC.WebpLossyEncodeStage(w, h, True, n, DEV, intra4=True)
    assert stage.max_file_bytes == E4.max_file_bytes(w, h, True) >= ENC.WebpLossyEncodeStage(w, h, True, n, DEV).max_file_bytes
    b = OLD.bitmap(np.stack([OLD.rows_of(f) for f in frames]), w, h)
    guard = 4096

    def run(pitch):
        files = torch.full((n * pitch + guard,), 0x5C, dtype=torch.uint8, device=DEV)
        lengths = torch.full((n + 64,), -7, dtype=torch.int32, device=DEV)
        status = torch.full((n + 64,), -9, dtype=torch.int32, device=DEV)
        stage.encode_device(b, q, pitch, files[:n * pitch].view(n, pitch), lengths, status)
        torch.cuda.synchronize()
        assert bool((files[n * pitch:] == 0x5C).all()) and bool((lengths[n:] == -7).all()) and bool((status[n:] == -9).all())
        return files.cpu().numpy(), lengths[:n].cpu().tolist(), status[:n].cpu().tolist()
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    host, ln, st = run(pitch)
    assert st == [0] * n and ln == [len(f) for f in want]
    for i in range(n):
        assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i]
        assert not host[i * pitch + ln[i]:(i + 1) * pitch].any(), "zeros behind a file's end"
    # one byte short of the largest file (the textured frame's): that image alone is dropped
    assert len(want[1]) > max(len(want[0]), len(want[2]))
    pitch = len(want[1]) - 1
    host, ln, st = run(pitch)
    assert st == [0, ENC.VP8_ENC_FILE_OVERFLOW, 0] and ln == [len(want[0]), 0, len(want[2])]
    for i in (0, 2):
        assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i], "the neighbours of a dropped image are whole"
    assert bool((host[pitch:2 * pitch] == 0x5C).all()), "nothing of a dropped image's file is written"


def test_dropin_equals_the_device_form():
    w, h, stride = 37, 23, 4 * 37 + 8
    frame = F.photo(w, h, alpha=True, seed=61)
    for alpha in (True, False):
        host = ENC.encode_webp_lossy_host(OLD.rows_of(frame, stride), w, h, stride, 80, alpha, intra4=True)
        want, _, st = emulated(frame, 80, alpha)
        assert host == want and st["n_i4"] > 0
        assert host == encode(frame[None], 80, alpha)[0][0]
        assert ENC.encode_webp_lossy_host(OLD.rows_of(frame, stride), w, h, stride, 80, alpha) == E.encode(frame, 80, alpha)[0], "without the flag: the 16x16 coder's file"


def test_one_800x450_frame_equals_the_emulation_and_reads_back_on_the_device():
    from imageflow_amd.codecs import webp_lossy_decoder as DEC
    frame = E.photo_frame()
    files, status = encode(frame[None], 75, False)
    want, expect, st = emulated(frame, 75, False)
    assert status == [0] and files[0] == want and 0 < st["n_i4"] < st["n_mbs"]
    back = DEC.decode_webp_lossy(files[0], DEV)
    got = back.to_numpy()[0][:, :4 * back.w].reshape(back.h, back.w, 4)
    assert np.array_equal(got, expect), "the device's own lossy decoder reads the file back to the pixels the coder reconstructed"


# ---- the `webplossy` preset behind the switch's values 1 and 2 --------------------------------------------------------------------------

def _execute(data, form, value):
    with Context() as c:
        assert c.L.ifhip_shim_context_set_webp_lossy_encoder(c.p, value)
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        if form == "graph":
            c.add_output_buffer(2)
        r = OLD._run(c, OLD._job(form, OLD.PRESET))
        out = bytes(c.get_output_buffer(1))
        raw = bytes(c.get_output_buffer(2)) if form == "graph" else None
    entry = [e for e in r["data"]["job_result"]["encodes"] if e["io_id"] == 1][0]
    return out, entry, raw


@pytest.mark.parametrize("form", ["steps", "graph"])
def test_switch_value_2_writes_the_flagged_file_and_value_1_the_16x16_coders(form):
    data, alpha = OLD._inputs()["alpha"]
    _, _, raw = _execute(data, "graph", 1)
    rows, w, h, raw_alpha = unpack_raw_bgra(raw)
    frame = np.ascontiguousarray(rows[:, :4 * w]).reshape(h, w, 4)
    out, entry, _ = _execute(data, form, 2)
    want, expect, st = emulated(frame, 80.0, alpha, ("job", 2))
    assert (entry["preferred_mime_type"], entry["preferred_extension"], entry["w"], entry["h"]) == ("image/webp", "webp", w, h)
    assert out == want and st["n_i4"] > 0, "the job's file is the flagged coder's file of the job's pixels"
    assert np.array_equal(E.pillow_bgra(out)[0], expect)
    plain, entry, _ = _execute(data, form, 1)
    assert plain == E.encode(frame, 80.0, alpha)[0] and plain != out, "value 1: the unflagged emulation's file"
    with Context() as c:                                              # the Python front end sends 2 when both are set
        assert c.set_webp_lossy_encoder(True, intra4=True)
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        if form == "graph":
            c.add_output_buffer(2)
        OLD._run(c, OLD._job(form, OLD.PRESET))
        assert bytes(c.get_output_buffer(1)) == out
