"""The device lossy WebP coder on an MI355X (csrc/vp8_encode.hip through imageflow_amd.codecs.webp_lossy_encoder and the
`webplossy` preset of `encode` behind Context.set_webp_lossy_encoder): every file equals the CPU emulation's
(tests/vp8_encode_emulate.cpp, whose files libwebp decodes to the emulation's own reconstruction in
tests/test_vp8_encode_core.py) byte for byte, in every batch position; guard regions stay untouched and a pitch one byte
short drops that image alone; the device's own lossy decoder reads the files back; the shim's jobs write the file only with
the switch on."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import webp_lossy_encoder as ENC  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import util as U  # noqa: E402
from tests import vp8_encode_emu as E  # noqa: E402
from tests import webp_frames as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = E.small_frames()
_EMULATED = {}


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


def emulated(bgra, quality, alpha, key=None):
    """the emulation's file of a frame and the BGRA it expects of a decoder, computed once per key"""
    if key is None or key not in _EMULATED:
        data, expect, st = E.encode(bgra, quality, alpha)
        assert st["errors"] == 0
        if key is None:
            return data, expect
        _EMULATED[key] = (data, expect)
    return _EMULATED[key]


def encode(frames, quality, alpha=True, **kw):
    """files and status words of BGRA frames [n, h, w, 4] of one geometry"""
    n, h, w, _ = frames.shape
    stage = ENC.WebpLossyEncodeStage(w, h, alpha, n, DEV)
    return stage.encode(bitmap(np.stack([rows_of(f) for f in frames]), w, h, alpha), quality, **kw)


@pytest.mark.parametrize("quality", E.QUALITIES)
@pytest.mark.parametrize("name", sorted(SMALL))
def test_device_file_equals_the_emulations_byte_for_byte(name, quality):
    frame, alpha = SMALL[name]
    files, status = encode(frame[None], quality, alpha)
    assert status == [0]
    want, _ = emulated(frame, quality, alpha, (name, quality))
    assert len(files[0]) == len(want) and files[0] == want, (name, quality)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_batches_give_equal_bytes_in_every_position(n):
    w, h = 70, 66                                                   # 5 x 5 macroblocks, ragged edges, four partitions
    kinds = {"a": F.photo(w, h, alpha=True, seed=21), "b": F.noise(w, h, 22), "c": F.one_colour(w, h, (9, 8, 7, 255))}
    kinds["b"][..., 3] = 255                                        # an opaque frame between frames with alpha: a simple file
    order = "abaca"[:n]
    files, status = encode(np.stack([kinds[k] for k in order]), 75)
    assert status == [0] * n
    for k, data in zip(order, files):
        assert data == emulated(kinds[k], 75, True, ("batch", k))[0], (n, k)
    assert files[0][12:16] == b"VP8X" and (n < 2 or files[1][12:16] == b"VP8 ")
    again, _ = encode(np.stack([kinds[k] for k in order]), 75)
    assert again == files, "the same pixels give the same bytes on every run"


def test_guard_regions_and_file_overflow():
    w, h, n, q = 70, 66, 3, 90
    frames = np.stack([F.photo(w, h, seed=31), F.noise(w, h, 32), F.photo(w, h, seed=33)])
    frames[..., 3] = 255
    want = [emulated(f, q, True)[0] for f in frames]
    stage = ENC.WebpLossyEncodeStage(w, h, True, n, DEV)
    assert stage.max_file_bytes == int(E.emulator().vp8e_emu_max_file_bytes(w, h, 1))
    b = bitmap(np.stack([rows_of(f) for f in frames]), w, h)
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
    # one byte short of the largest file (the noise frame's; no multiple of 4 either): that image alone is dropped
    assert len(want[1]) > max(len(want[0]), len(want[2]))
    pitch = len(want[1]) - 1
    host, ln, st = run(pitch)
    assert st == [0, ENC.VP8_ENC_FILE_OVERFLOW, 0] and ln == [len(want[0]), 0, len(want[2])]
    for i in (0, 2):
        assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i], "the neighbours of a dropped image are whole"
    assert bool((host[pitch:2 * pitch] == 0x5C).all()), "nothing of a dropped image's file is written"
    # and with exactly its size it fits; with an odd pitch the file's last byte lies in a dword that reaches past the pitch
    for pitch in (len(want[1]), len(want[1]) + 1):
        host, ln, st = run(pitch)
        assert st == [0] * n
        for i in range(n):
            assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i], (pitch, i)


def test_dropin_equals_the_device_form():
    w, h, stride = 37, 23, 4 * 37 + 8
    frame = F.photo(w, h, alpha=True, seed=61)
    for alpha in (True, False):
        host = ENC.encode_webp_lossy_host(rows_of(frame, stride), w, h, stride, 80, alpha)
        assert host == emulated(frame, 80, alpha)[0]
        assert (host[12:16] == b"VP8X") == alpha


def test_short_image_bytes_is_refused_on_the_device():
    w, h, stride = 37, 23, 4 * 37 + 8
    frame = torch.zeros(h * stride, dtype=torch.uint8, device=DEV)
    stage = ENC.WebpLossyEncodeStage(w, h, True, 1, DEV)
    files = torch.zeros(stage.max_file_bytes + 16, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(2, dtype=torch.int32, device=DEV)
    L = ENC._bind()
    short = (h - 1) * stride + 4 * w - 4
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(DEV):
        assert L.ifhip_webp_lossy_encode_batch_device(stage._h, frame.data_ptr(), short, stride, 1, 75.0, files.data_ptr(), files.numel(), ln.data_ptr(), None, stream) == 1
        assert L.ifhip_webp_lossy_encode_batch_device(stage._h, frame.data_ptr(), short + 4, stride, 1, 75.0, files.data_ptr(), files.numel(), ln.data_ptr(), None, stream) == 0
        torch.cuda.synchronize()
    assert int(ln[0]) > 0


def test_one_800x450_frame_equals_the_emulation_and_reads_back_on_the_device():
    from imageflow_amd.codecs import webp_lossy_decoder as DEC
    frame = E.photo_frame()
    files, status = encode(frame[None], 75, False)
    want, expect = emulated(frame, 75, False)
    assert status == [0] and files[0] == want
    pillow, mode = E.pillow_bgra(files[0])
    assert mode == "RGB" and np.array_equal(pillow, expect)
    back = DEC.decode_webp_lossy(files[0], DEV)
    got = back.to_numpy()[0][:, :4 * back.w].reshape(back.h, back.w, 4)
    assert np.array_equal(got, pillow), "the device's own lossy decoder reads the file back to Pillow's pixels"


# ---- the `webplossy` preset of `encode` behind Context.set_webp_lossy_encoder (csrc/abi_shim.cpp) -----------------------------------

RESAMPLE = {"resample_2d": {"w": 90, "h": 61, "hints": {}}}
PRESET = {"webplossy": {"quality": 80.0}}


def _run(ctx, job, expect=200):
    status, r = ctx.send_json("v1/execute", job)
    assert status == expect, (status, r, ctx.error_message())
    return r


def _inputs():
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(F.photo(203, 131, seed=51)[..., [2, 1, 0]]), "RGB").save(b, "JPEG", quality=85)
    with_alpha = F.photo(160, 120, alpha=True, seed=52)
    return {"jpeg": (b.getvalue(), False), "alpha": (pack_raw_bgra(rows_of(with_alpha), 160, 120, alpha_meaningful=True), True)}


def _job(form, preset, tap="gif"):
    """decode -> resample_2d -> encode `preset` into io 1; as a graph the same frame also goes to the raw tap in io 2"""
    if form == "steps":
        return {"framewise": {"steps": [{"decode": {"io_id": 0}}, RESAMPLE, {"encode": {"io_id": 1, "preset": preset}}]}}
    return {"framewise": {"graph": {
        "nodes": {"0": {"decode": {"io_id": 0}}, "1": RESAMPLE, "2": {"encode": {"io_id": 1, "preset": preset}}, "3": {"encode": {"io_id": 2, "preset": tap}}},
        "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 1, "to": 2, "kind": "input"}, {"from": 1, "to": 3, "kind": "input"}]}}}


def _execute(data, form, preset, on):
    """(the preset's output, its response entry, the raw tap of the same job) -- for steps the tap is the job run again with "gif" """
    with Context() as c:
        if on:
            assert c.set_webp_lossy_encoder(True)
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
def test_webplossy_preset_writes_the_file_with_the_switch_on_and_the_raw_container_with_it_off(source, form):
    data, alpha = _inputs()[source]
    out, entry, raw = _execute(data, form, PRESET, True)
    assert raw[:7] == b"IFBGRA1"
    rows, w, h, raw_alpha = unpack_raw_bgra(raw)
    assert (w, h, raw_alpha) == (90, 61, alpha)
    assert (entry["preferred_mime_type"], entry["preferred_extension"], entry["w"], entry["h"]) == ("image/webp", "webp", w, h)
    assert out[:4] == b"RIFF" and out[8:12] == b"WEBP" and out[12:16] == (b"VP8X" if alpha else b"VP8 ")
    frame = np.ascontiguousarray(rows[:, :4 * w]).reshape(h, w, 4)
    want, expect = emulated(frame, 80.0, alpha)
    assert out == want, "the job's file is the coder's file of the job's pixels"
    got, mode = E.pillow_bgra(out)
    assert mode == ("RGBA" if alpha else "RGB") and np.array_equal(got, expect)
    if alpha:
        assert (got[..., 3] < 255).any() and np.array_equal(got[..., 3], frame[..., 3])
    off, entry, raw_off = _execute(data, form, PRESET, False)            # off, as it is by default: the raw container, as ever
    assert off[:7] == b"IFBGRA1" and off == raw_off == raw and entry["preferred_extension"] == "ifbgra"


def test_with_the_switch_on_bad_forms_are_invalid_json_and_a_large_side_is_libwebps_error():
    data, _ = _inputs()["jpeg"]
    for preset in ("webplossy", {"webplossy": {}}, {"webplossy": {"quality": "80"}}):
        with Context() as c:
            assert c.set_webp_lossy_encoder(True)
            c.add_input_buffer(0, data)
            c.add_output_buffer(1)
            _run(c, _job("steps", preset), expect=400)
            assert c.error_code() == 3 and c.error_message()[0].startswith("InvalidJson: encode.preset.webplossy.quality is a number")
    wide = pack_raw_bgra(np.zeros((1, 4 * 16384), np.uint8), 16384, 1, alpha_meaningful=False)
    with Context() as c:
        assert c.set_webp_lossy_encoder(True)
        c.add_input_buffer(0, wide)
        c.add_output_buffer(1)
        limit = {"w": 20000, "h": 20000, "megapixels": 100}              # (the default max_frame_size stops at 10000)
        status, _ = c.send_json("v1/execute", {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": PRESET}}]},
                                               "security": {"max_frame_size": limit, "max_decode_size": limit}})
        assert status == 500 and c.error_code() == 18 and c.error_message()[0].startswith("ImageEncodingError: libwebp encoding error")
    with Context() as c:                                              # the querystring's format=webp stays refused, switch or no switch
        assert c.set_webp_lossy_encoder(True)
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        status, _ = c.send_json("v1/execute", {"framewise": {"steps": [{"command_string": {"kind": "ir4", "value": "width=50&format=webp", "decode": 0, "encode": 1}}]}})
        assert status != 200
