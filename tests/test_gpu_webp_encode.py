"""The device lossless-WebP coder on an MI355X (csrc/webp_encode.hip through imageflow_amd.codecs.webp_encoder and the
`webplossless` preset of `encode`): every file equals the CPU emulation's (tests/webp_emulate.cpp, whose files libwebp and
tests/vp8l_reader.py decode to the source in tests/test_webp_device_coder.py) byte for byte, in every batch position; guard
regions stay untouched and a pitch one byte short drops that image alone; the shim's jobs decode through libwebp to what
the same job's raw tap returns."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import webp_encoder as WEBP  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import util as U  # noqa: E402
from tests import webp_emulation as E  # noqa: E402
from tests import webp_frames as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = F.cases()
_EMULATED = {}
Image.MAX_IMAGE_PIXELS = None


def rows_of(bgra, stride=None):
    """BGRA [h, w, 4] -> one frame [h, stride]; the padding is filled with 0xA5 so that a leak shows."""
    h, w, _ = bgra.shape
    stride = stride or U.stride_for(w)
    out = np.full((h, stride), 0xA5, np.uint8)
    out[:, :4 * w] = bgra.reshape(h, 4 * w)
    return out


def bitmap(frames, w, h, alpha=True):
    frames = np.ascontiguousarray(frames)
    return Bitmap.from_numpy(frames, w, h, frames.shape[-1], DEV, alpha_meaningful=alpha)


def emulated(bgra, alpha, key=None):
    """the emulation's file of a frame, computed once per key"""
    if key is None or key not in _EMULATED:
        data, _ = E.encode(bgra, alpha)
        if key is None:
            return data
        _EMULATED[key] = data
    return _EMULATED[key]


def encode(frames, alpha=True, **kw):
    """files and status words of BGRA frames [n, h, w, 4] of one geometry"""
    n, h, w, _ = frames.shape
    stage = WEBP.WebpEncodeStage(w, h, alpha, n, DEV)
    return stage.encode(bitmap(np.stack([rows_of(f) for f in frames]), w, h, alpha), **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_file_equals_the_emulations_byte_for_byte(name):
    frame, alpha = CASES[name]
    files, status = encode(frame[None], alpha)
    assert status == [0]
    want = emulated(frame, alpha, name)
    assert len(files[0]) == len(want) and files[0] == want, name
    got, mode = F.pillow_decode(files[0])
    assert np.array_equal(got, F.rgba_of(frame, alpha)) and mode == ("RGBA" if alpha else "RGB")


@pytest.mark.parametrize("n", [1, 2, 5])
def test_batches_give_equal_bytes_in_every_position(n):
    w, h = 70, 66                                                   # two bands, two segments a band
    kinds = {"a": F.photo(w, h, alpha=True, seed=21), "b": F.noise(w, h, 22), "c": F.one_colour(w, h, (9, 8, 7, 255))}
    order = "abaca"[:n]
    files, status = encode(np.stack([kinds[k] for k in order]))
    assert status == [0] * n
    for k, data in zip(order, files):
        assert data == emulated(kinds[k], True, ("batch", k)), (n, k)
    again, _ = encode(np.stack([kinds[k] for k in order]))
    assert again == files, "the same pixels give the same bytes on every run"


def test_guard_regions_and_file_overflow():
    w, h, n = 70, 66, 3
    frames = np.stack([F.photo(w, h, seed=31), F.noise(w, h, 32), F.photo(w, h, seed=33)])
    want = [emulated(f, True) for f in frames]
    stage = WEBP.WebpEncodeStage(w, h, True, n, DEV)
    assert stage.max_file_bytes == E.max_file_bytes(w, h)
    b = bitmap(np.stack([rows_of(f) for f in frames]), w, h)
    guard = 4096

    def run(pitch):
        files = torch.full((n * pitch + guard,), 0x5C, dtype=torch.uint8, device=DEV)
        lengths = torch.full((n + 64,), -7, dtype=torch.int32, device=DEV)
        status = torch.full((n + 64,), -9, dtype=torch.int32, device=DEV)
        stage.encode_device(b, pitch, files[:n * pitch].view(n, pitch), lengths, status)
        torch.cuda.synchronize()
        assert bool((files[n * pitch:] == 0x5C).all()) and bool((lengths[n:] == -7).all()) and bool((status[n:] == -9).all())
        return files.cpu().numpy(), lengths[:n].cpu().tolist(), status[:n].cpu().tolist()
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    host, ln, st = run(pitch)
    assert st == [0] * n and ln == [len(f) for f in want]
    for i in range(n):
        assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i]
        assert not host[i * pitch + ln[i]:(i + 1) * pitch].any(), "zeros behind a file's end"
    # one byte short of the largest file (the noise frame's; no multiple of 4 either): that image alone is dropped
    assert len(want[1]) > max(len(want[0]), len(want[2]))
    pitch = len(want[1]) - 1
    host, ln, st = run(pitch)
    assert st == [0, WEBP.WEBP_FILE_OVERFLOW, 0] and ln == [len(want[0]), 0, len(want[2])]
    for i in (0, 2):
        assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i], "the neighbours of a dropped image are whole"
    # and with exactly its size it fits; with an odd pitch the file's last byte lies in a dword that reaches past the pitch
    for pitch in (len(want[1]), len(want[1]) + 1):
        host, ln, st = run(pitch)
        assert st == [0] * n
        for i in range(n):
            assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i], (pitch, i)


def test_dropin_equals_the_device_form():
    w, h, stride = 37, 23, 4 * 37 + 8
    frame, _ = CASES["odd_width"]
    for alpha in (True, False):
        host = WEBP.encode_webp_host(rows_of(frame, stride), w, h, stride, alpha)
        assert host == emulated(frame, alpha)


def test_short_image_bytes_is_refused_on_the_device():
    w, h, stride = 37, 23, 4 * 37 + 8
    frame = torch.zeros(h * stride, dtype=torch.uint8, device=DEV)
    stage = WEBP.WebpEncodeStage(w, h, True, 1, DEV)
    files = torch.zeros(stage.max_file_bytes + 16, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(2, dtype=torch.int32, device=DEV)
    L = WEBP._bind()
    short = (h - 1) * stride + 4 * w - 4
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(DEV):
        assert L.ifhip_webp_encode_batch_device(stage._h, frame.data_ptr(), short, stride, 1, files.data_ptr(), files.numel(), ln.data_ptr(), None, stream) == 1
        assert L.ifhip_webp_encode_batch_device(stage._h, frame.data_ptr(), short + 4, stride, 1, files.data_ptr(), files.numel(), ln.data_ptr(), None, stream) == 0
        torch.cuda.synchronize()
    assert int(ln[0]) > 0


def test_one_full_size_frame_decodes_exactly():
    w, h = 3840, 2160
    frame = F.photo(w, h, alpha=True, seed=41)
    files, status = encode(frame[None])
    assert status == [0] and len(files[0]) <= E.max_file_bytes(w, h)
    print(f"{w}x{h}: {len(files[0])} bytes, {8 * len(files[0]) / (w * h):.2f} bits a pixel")
    got, mode = F.pillow_decode(files[0])
    assert mode == "RGBA" and np.array_equal(got, F.rgba_of(frame))


# ---- the `webplossless` preset of `encode` (csrc/abi_shim.cpp) ---------------------------------------------------------------------

RESAMPLE = {"resample_2d": {"w": 90, "h": 61, "hints": {}}}


def _run(ctx, job, expect=200):
    status, r = ctx.send_json("v1/execute", job)
    assert status == expect, (status, r, ctx.error_message())
    return r


def _inputs():
    b = io.BytesIO()
    Image.fromarray(F.rgba_of(F.photo(203, 131, seed=51))[..., :3].copy(), "RGB").save(b, "JPEG", quality=85)
    with_alpha = F.photo(160, 120, alpha=True, seed=52)
    return {"jpeg": (b.getvalue(), False), "alpha": (pack_raw_bgra(rows_of(with_alpha), 160, 120, alpha_meaningful=True), True)}


def _job(form, preset, tap="gif"):
    """decode -> resample_2d -> encode `preset` into io 1; as a graph the same frame also goes to the raw tap in io 2"""
    if form == "steps":
        return {"framewise": {"steps": [{"decode": {"io_id": 0}}, RESAMPLE, {"encode": {"io_id": 1, "preset": preset}}]}}
    return {"framewise": {"graph": {
        "nodes": {"0": {"decode": {"io_id": 0}}, "1": RESAMPLE, "2": {"encode": {"io_id": 1, "preset": preset}}, "3": {"encode": {"io_id": 2, "preset": tap}}},
        "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 1, "to": 2, "kind": "input"}, {"from": 1, "to": 3, "kind": "input"}]}}}


def _execute(data, form, preset):
    """(the preset's output, its response entry, the raw tap of the same job) -- for steps the tap is the job run again with "gif" """
    with Context() as c:
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        if form == "graph":
            c.add_output_buffer(2)
        r = _run(c, _job(form, preset))
        out = bytes(c.get_output_buffer(1))
        raw = bytes(c.get_output_buffer(2)) if form == "graph" else None
    if raw is None:
        with Context() as c:
            c.add_input_buffer(0, data)
            c.add_output_buffer(1)
            _run(c, _job("steps", "gif"))
            raw = bytes(c.get_output_buffer(1))
    entry = [e for e in r["data"]["job_result"]["encodes"] if e["io_id"] == 1][0]
    return out, entry, raw


@pytest.mark.parametrize("form", ["steps", "graph"])
@pytest.mark.parametrize("source", ["jpeg", "alpha"])
def test_webplossless_preset_writes_the_jobs_pixels(source, form):
    data, alpha = _inputs()[source]
    out, entry, raw = _execute(data, form, "webplossless")
    assert raw[:7] == b"IFBGRA1", "the gif preset still returns the raw container"
    rows, w, h, raw_alpha = unpack_raw_bgra(raw)
    assert (w, h, raw_alpha) == (90, 61, alpha)
    assert (entry["preferred_mime_type"], entry["preferred_extension"], entry["w"], entry["h"]) == ("image/webp", "webp", w, h)
    assert out[:4] == b"RIFF" and out[8:16] == b"WEBPVP8L"
    got, mode = F.pillow_decode(out)
    want = np.ascontiguousarray(rows[:, :4 * w]).reshape(h, w, 4)
    assert mode == ("RGBA" if alpha else "RGB")                     # normalize_unused_alpha: alpha_is_used = 0, alpha 255
    assert np.array_equal(got, F.rgba_of(want, alpha))
    if alpha:
        assert (got[..., 3] < 255).any()


def test_webplossy_preset_still_returns_the_raw_container():
    data, _ = _inputs()["jpeg"]
    out, entry, raw = _execute(data, "steps", {"webplossy": {"quality": 80.0}})
    assert out[:7] == b"IFBGRA1" and out == raw
    assert entry["preferred_extension"] == "ifbgra"
