"""The colour indexing of the device lossless-WebP coder on an MI355X (csrc/webp_encode_indexed.hip behind the stage flag
IFHIP_WEBP_ENC_COLOR_INDEXING, through imageflow_amd.codecs.webp_encoder): every flag-on file equals the CPU emulation's
(tests/webp_indexed_emulate.cpp, whose files libwebp and tests/vp8l_reader.py decode to the source in
tests/test_webp_indexed_coder.py) byte for byte, whichever variant was written and in every batch position; guard regions stay
untouched and a pitch one byte short drops that image alone; flags 0 is the plain stage; this project's own device decoder
reads every file back to the source."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.codecs import webp_decoder as DEC  # noqa: E402
from imageflow_amd.codecs import webp_encoder as WEBP  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import util as U  # noqa: E402
from tests import webp_emulation as PLAIN  # noqa: E402
from tests import webp_frames as F  # noqa: E402
from tests import webp_indexed_emulation as E  # noqa: E402
from tests import webp_indexed_frames as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = X.frames()
_EMULATED, _DEVICE = {}, {}


def rows_of(bgra, stride=None):
    """BGRA [h, w, 4] -> one frame [h, stride]; the padding is filled with 0xA5 so that a leak shows."""
    h, w, _ = bgra.shape
    stride = stride or U.stride_for(w)
    out = np.full((h, stride), 0xA5, np.uint8)
    out[:, :4 * w] = bgra.reshape(h, 4 * w)
    return out


def bitmap(frames, alpha=True):
    n, h, w, _ = frames.shape
    rows = np.ascontiguousarray(np.stack([rows_of(f) for f in frames]))
    return Bitmap.from_numpy(rows, w, h, rows.shape[-1], DEV, alpha_meaningful=alpha)


def emulated(bgra, alpha, key):
    """(the emulation's flag-on file of a frame, its counters), computed once per key"""
    if key not in _EMULATED:
        _EMULATED[key] = E.encode(bgra, alpha, E.COLOR_INDEXING)
    return _EMULATED[key]


def encode(frames, alpha=True, color_indexing=True, **kw):
    """files and status words of BGRA frames [n, h, w, 4] of one geometry"""
    n, h, w, _ = frames.shape
    stage = WEBP.WebpEncodeStage(w, h, alpha, n, DEV, color_indexing=color_indexing)
    return stage.encode(bitmap(frames, alpha), **kw)


def device_file(name):
    if name not in _DEVICE:
        frame, alpha = FRAMES[name]
        _DEVICE[name] = encode(frame[None], alpha)
    return _DEVICE[name]


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_flag_on_file_equals_the_emulations_byte_for_byte(name):
    frame, alpha = FRAMES[name]
    files, status = device_file(name)
    assert status == [0]
    want, st = emulated(frame, alpha, name)
    assert len(files[0]) == len(want) and files[0] == want, (name, st)
    got, mode = F.pillow_decode(files[0])
    assert np.array_equal(got, F.rgba_of(frame, alpha)) and mode == ("RGBA" if alpha else "RGB")


def test_both_variants_are_among_the_files():
    chosen = {name: emulated(*FRAMES[name], name)[1]["indexed"] for name in FRAMES}
    assert sum(chosen.values()) >= 20 and sum(1 for v in chosen.values() if not v) >= 10, chosen


def mixed_batch():
    w, h = 70, 66
    return [F.few_colours(w, h, n=17), F.noise(w, h, 81), F.few_colours(w, h, n=2), X.grey_photo(w, h), F.one_colour(w, h), X.exactly(256, w, h)]


def test_a_mixed_batch_gives_equal_bytes_in_every_position():
    """indexed without bundling, plain (too many colours), indexed with 8 pixels a bundle, plain (indexing sized and lost),
    one colour, and a full table, on one stage -- and again in reverse, so that the position does not show"""
    frames = mixed_batch()
    want = [emulated(f, True, ("mixed", i)) for i, f in enumerate(frames)]
    assert [st["indexed"] for _, st in want] == [1, 0, 1, 0, 1, 1] and want[3][1]["indexed_bytes"] > want[3][1]["plain_bytes"] > 0
    n = len(frames)
    stage = WEBP.WebpEncodeStage(70, 66, True, n, DEV, color_indexing=True)
    files, status = stage.encode(bitmap(np.stack(frames)))
    assert status == [0] * n
    for i in range(n):
        assert files[i] == want[i][0], i
    back, status = stage.encode(bitmap(np.stack(frames[::-1])))
    assert status == [0] * n and back == files[::-1]
    fewer, status = stage.encode(bitmap(np.stack(frames[2:4])))          # a smaller batch on the same stage
    assert status == [0, 0] and fewer == files[2:4]


def test_guard_regions_odd_pitches_and_file_overflow():
    w, h, n = 70, 66, 3
    frames = np.stack([F.few_colours(w, h, n=5), F.few_colours(w, h, n=17), F.row_ramp(w, h)])
    emu = [emulated(f, True, ("guard", i)) for i, f in enumerate(frames)]
    want = [d for d, _ in emu]
    assert [st["indexed"] for _, st in emu] == [1, 1, 0]
    stage = WEBP.WebpEncodeStage(w, h, True, n, DEV, color_indexing=True)
    assert stage.max_file_bytes == PLAIN.max_file_bytes(w, h)
    b = bitmap(frames)
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
    # one byte short of the largest file, an indexed one (no multiple of 4 either): that image alone is dropped
    assert len(want[1]) > max(len(want[0]), len(want[2]))
    pitch = len(want[1]) - 1
    host, ln, st = run(pitch)
    assert st == [0, WEBP.WEBP_FILE_OVERFLOW, 0] and ln == [len(want[0]), 0, len(want[2])]
    for i in (0, 2):
        assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i], "the neighbours of a dropped image are whole"
    assert not host[pitch:2 * pitch].any(), "nothing of a dropped image is written"
    # with exactly its size it fits; with an odd pitch the file's last byte lies in a dword that reaches past the pitch
    for pitch in (len(want[1]), len(want[1]) + 1, len(want[1]) + 3):
        host, ln, st = run(pitch)
        assert st == [0] * n
        for i in range(n):
            assert host[i * pitch:i * pitch + ln[i]].tobytes() == want[i], (pitch, i)


def test_flags_zero_is_the_plain_stage():
    for name in ("few_96x80", "photo", "bgrx_few"):
        frame, alpha = FRAMES[name]
        files, status = encode(frame[None], alpha, color_indexing=False)
        assert status == [0] and files[0] == PLAIN.encode(frame, alpha)[0], name
        h, w = frame.shape[:2]
        L, handle = WEBP._bind(), C.c_void_p()
        assert L.ifhip_webp_enc_stage_create_flags(C.byref(handle), w, h, 1 if alpha else 0, 1, 0) == 0
        b = bitmap(frame[None], alpha)
        pitch = (L.ifhip_webp_enc_stage_max_file_bytes(handle) + 15) // 16 * 16
        out = torch.empty(pitch, dtype=torch.uint8, device=DEV)
        ln = torch.zeros(2, dtype=torch.int32, device=DEV)
        with torch.cuda.device(DEV):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert L.ifhip_webp_encode_batch_device(handle, b.data.data_ptr(), b.image_bytes, b.stride, 1, out.data_ptr(), pitch, ln.data_ptr(), None, stream) == 0
            torch.cuda.synchronize()
        L.ifhip_webp_enc_stage_destroy(handle)
        assert out[:int(ln[0])].cpu().numpy().tobytes() == files[0], name


def test_the_host_form_takes_the_flag():
    frame, alpha = FRAMES["few_37x23"]
    stride = 4 * 37 + 8
    assert WEBP.encode_webp_host(rows_of(frame, stride), 37, 23, stride, alpha, color_indexing=True) == emulated(frame, alpha, "few_37x23")[0]
    assert WEBP.encode_webp_host(rows_of(frame, stride), 37, 23, stride, alpha) == PLAIN.encode(frame, alpha)[0]


def test_the_device_decoder_reads_every_flag_on_file_back():
    names = sorted(FRAMES)
    files = [device_file(name)[0][0] for name in names]
    frames, status = DEC.decode_webp_batch(files, DEV)
    assert status == [0] * len(files)
    for name, fr in zip(names, frames):
        frame, alpha = FRAMES[name]
        want = frame.copy()
        if not alpha:
            want[..., 3] = 255
        got = fr.to_numpy()[0][:, :4 * fr.w].reshape(want.shape)
        assert np.array_equal(got, want) and fr.alpha_meaningful == alpha, name
