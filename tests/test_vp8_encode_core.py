"""The lossy WebP coder's algorithm without a device: csrc/vp8_encode_core.hpp (colour conversion, mode decision, forward
transforms, quantisation, the token walk, the probability rule, the run-deferred bool coder, the file's layout) over
csrc/vp8_decode_core.hpp, as tests/vp8_encode_emulate.cpp runs it in the schedule of csrc/vp8_encode.hip.  The contract is not
libwebp's bytes: libwebp 1.6.0 through Pillow decodes every file to EXACTLY the pixels the emulation expects (its own
reconstruction through the decoder core's loop filter, upsampler and conversion) -- coder and decoder cannot drift apart --
and the files' SHA-256 are pinned in tests/vp8_encode_pins.json, so that a later change of one bit shows.  Rate and quality
are measured against libwebp's own files.  The same small cases run again through a stand-alone program under ASan + UBSan."""
import hashlib
import json
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests import vp8_encode_emu as E
from tests import vp8_gen as G
from tests import webp_frames as F

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "vp8_encode_pins.json")
SMALL = E.small_frames()
RATE_QUALITIES = (25, 50, 75, 90)
_CACHE = {}


def coded(name, quality):
    """(file, expected BGRA, stats) of a named frame, computed once"""
    if (name, quality) not in _CACHE:
        frame, alpha = (E.photo_frame(), False) if name == "photo_800x450" else SMALL[name]
        _CACHE[name, quality] = E.encode(frame, quality, alpha)
    return _CACHE[name, quality]


def source(name):
    return E.photo_frame() if name == "photo_800x450" else SMALL[name][0]


def fnv(data):
    s = 0x811C9DC5
    for b in bytes(data):
        s = ((s ^ b) * 0x01000193) & 0xFFFFFFFF
    return s


@pytest.mark.parametrize("quality", E.QUALITIES)
@pytest.mark.parametrize("name", sorted(SMALL) + ["photo_800x450"])
def test_libwebp_decodes_the_file_to_exactly_what_the_coder_reconstructed(name, quality):
    data, expect, st = coded(name, quality)
    assert st["errors"] == 0 and st["max_level"] <= 2047
    assert st["index"] == int(E.emulator().vp8e_emu_quality_to_index(quality)) and st["filter_level"] == int(E.emulator().vp8e_emu_filter_level(st["index"]))
    h, w = source(name).shape[:2]
    assert st["partitions"] == max(p for p in (1, 2, 4, 8) if p <= min(8, (h + 15) // 16))
    assert len(data) <= int(E.emulator().vp8e_emu_max_file_bytes(w, h, 1 if SMALL.get(name, (0, False))[1] else 0))
    got, mode = E.pillow_bgra(data)
    assert got.shape == expect.shape and np.array_equal(got, expect), (name, quality)
    assert mode == ("RGBA" if st["alpha"] else "RGB")


def test_the_quantiser_index_follows_libwebps_quality_curve():
    def index(q):
        c = min(max(q, 0.0), 100.0) / 100.0
        lin = c * 2.0 / 3.0 if c < 0.75 else 2.0 * c - 1.0
        return int(np.floor(127.0 * (1.0 - lin ** (1.0 / 3.0)) + 0.5))
    L = E.emulator()
    for q in (-5.0, 0.0, 10.0, 25.0, 50.0, 74.9, 75.0, 85.0, 90.0, 100.0, 250.0):
        assert int(L.vp8e_emu_quality_to_index(q)) == index(q), q
    assert int(L.vp8e_emu_quality_to_index(0.0)) == 127 and int(L.vp8e_emu_quality_to_index(100.0)) == 0
    for idx in range(128):                                          # the filter level: a pure integer function of the index
        assert int(L.vp8e_emu_filter_level(idx)) == min(63, idx // 2)
    for p in (1, 2, 64, 128, 200, 255, 256):                        # the cost table of the probability rule: 256 * log2(256 / p), eight fraction bits
        assert abs(int(L.vp8e_emu_cost(p)) - 256.0 * np.log2(256.0 / p)) <= 1.0, p


def test_a_meaningful_alpha_plane_comes_back_exactly_and_an_opaque_one_leaves_no_alph():
    frame, _ = SMALL["alpha_90x61"]
    data, expect, st = coded("alpha_90x61", 85)
    assert st["alpha"] == 1 and data[12:16] == b"VP8X" and data[20] == 0x10
    assert struct.unpack("<I", data[24:27] + b"\0")[0] == 89 and struct.unpack("<I", data[27:30] + b"\0")[0] == 60
    tags = [t for t, _, _ in G.chunks_of(data)]
    assert tags == [b"VP8X", b"ALPH", b"VP8 "]
    assert G.chunk_body(data, b"ALPH")[0] == 0x01                   # VP8L-coded, filter none, no pre-processing
    assert all((at & 1) == 0 for _, at, _ in G.chunks_of(data)) and len(data) % 2 == 0 and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    got, mode = E.pillow_bgra(data)
    assert mode == "RGBA" and np.array_equal(got[..., 3], frame[..., 3]) and (frame[..., 3] < 255).any()
    # alpha meaningful but 255 everywhere, and alpha that means nothing: simple files, mode RGB
    opaque, _, st = coded("opaque_alpha_40x24", 85)
    assert st["alpha"] == 0 and opaque[12:16] == b"VP8 " and [t for t, _, _ in G.chunks_of(opaque)] == [b"VP8 "]
    assert E.pillow_bgra(opaque)[1] == "RGB"
    garbage = F.garbage_alpha(SMALL["48x32"][0])
    plain, _, st = E.encode(garbage, 85, False)
    assert st["alpha"] == 0 and plain == coded("48x32", 85)[0], "normalize_unused_alpha: the alpha bytes of a BGRX frame do not show"
    # the RGB under transparent pixels is coded as it is: another colour there is another file
    other = frame.copy()
    other[frame[..., 3] < 200, :3] = 0
    assert E.encode(other, 85, True)[0] != data


def reference_bytes(bits, probs):
    e = G.BoolEncoder()
    for b, p in zip(bits, probs):
        e.put(int(b), int(p))
    return e.finish()


class SpyEncoder(G.BoolEncoder):
    """tests/vp8_gen.py's coder, noting how many 0xFF bytes each carry ran through"""
    def __init__(self):
        super().__init__()
        self.carried_through = []

    def _carry(self):
        k = 0
        while k < len(self.out) and self.out[-1 - k] == 255:
            k += 1
        self.carried_through.append(k)
        super()._carry()


def straddling_sequence(steps, cross):
    """Hand-made by rule, in exact integers: the coder's interval [low, low + range) is kept astride the middle of the first
    byte (B = 128 in the first byte's units) while it narrows, its low end as close below B as a probability allows -- the
    stream is 0x7F and then a run of 0xFF bytes that no carry has settled.  cross: a last one-bit whose split reaches B, so
    that the carry runs through the whole pending run; else the stream ends inside the run."""
    low, rng, mid, seq = 0, 255, 128, []

    def split(p):
        return 1 + (((rng - 1) * p) >> 8)

    def put(bit, p):
        nonlocal low, rng, mid
        s = split(p)
        if bit:
            low, rng = low + s, rng - s
        else:
            rng = s
        while rng < 128:
            low, rng, mid = low << 1, rng << 1, mid << 1
        seq.append((bit, p))
    for _ in range(steps):
        d = mid - low
        assert 0 < d < rng
        up = [p for p in range(255, 0, -1) if split(p) < d]          # a one-bit that stays below B: the largest step
        down = [p for p in range(1, 256) if split(p) > d]            # a zero-bit whose upper end stays above B: the smallest
        put(1, up[0]) if up else put(0, down[0])
    if cross:
        d = mid - low
        over = [p for p in range(1, 256) if d <= split(p) < rng]
        assert over
        put(1, over[0])
        for _ in range(16):
            put(0, 128)
    return [b for b, _ in seq], [p for _, p in seq]


def test_the_bool_coder_carries_across_runs_of_ff_bytes():
    for steps in (40, 200, 1000):
        bits, probs = straddling_sequence(steps, True)
        spy = SpyEncoder()
        for b, p in zip(bits, probs):
            spy.put(b, p)
        assert spy.carried_through and max(spy.carried_through) >= steps // 16, "the carry ran through a long run of pending 0xFF bytes"
        want = spy.finish()
        assert want[0] == 0x80 and not any(want[1:max(spy.carried_through)]), "0x7F 0xFF 0xFF ... became 0x80 0x00 0x00 ..."
        assert E.bool_bytes(bits, probs) == want, steps
    rng = np.random.default_rng(3)
    for _ in range(50):                                             # and random streams of skewed probabilities
        n = int(rng.integers(1, 400))
        probs = rng.choice([1, 2, 128, 254, 255], n)
        bits = (rng.random(n) < 0.5).astype(np.uint8)
        assert E.bool_bytes(bits, probs) == reference_bytes(bits, probs)


def test_a_partition_may_end_inside_a_pending_run():
    """the bytes before finish() are 0x7F and 0xFF bytes that no carry resolved: finish() stores them as they are"""
    for steps in (40, 200, 1000):
        bits, probs = straddling_sequence(steps, False)
        spy = SpyEncoder()
        for b, p in zip(bits, probs):
            spy.put(b, p)
        assert not spy.carried_through and len(spy.out) >= steps // 16 and spy.out[0] == 0x7F and all(v == 255 for v in spy.out[1:])
        want = spy.finish()
        assert E.bool_bytes(bits, probs) == want, steps
    assert E.bool_bytes([], []) == reference_bytes([], [])


def test_frames_with_no_and_with_many_probability_updates_round_trip():
    none, _, st0 = coded("16x16", 0)
    assert st0["updates"] == 0, "a macroblock of two levels cannot pay for an update"
    many, _, st1 = coded("photo_800x450", 100)
    assert st1["updates"] > 300
    for data, (name, q) in ((none, ("16x16", 0)), (many, ("photo_800x450", 100))):
        assert np.array_equal(E.pillow_bgra(data)[0], coded(name, q)[1])
    flat, _, st = coded("flat_40x40", 50)                           # skipped macroblocks: the flag and its probability
    assert st["skipped"] > 0 and st["skip_prob"] < 255


def test_the_same_cases_run_clean_under_asan_and_ubsan():
    """the stand-alone program: its own main, no sanitizer in this process; its output buffer is exactly the bound"""
    d = tempfile.mkdtemp(prefix="vp8_encode_sanitize_")
    exe, cases = os.path.join(d, "vp8_encode_emulate"), os.path.join(d, "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DVP8_ENC_EMU_MAIN", "-Wno-unused-function",
                    E.SRC, "-o", exe], check=True)
    want = []
    with open(cases, "wb") as f:
        for name in sorted(SMALL):
            frame, alpha = SMALL[name]
            for q in E.QUALITIES:
                data, expect, _ = coded(name, q)
                f.write(struct.pack("<IIII", frame.shape[1], frame.shape[0], 1 if alpha else 0, q) + np.ascontiguousarray(frame).tobytes())
                want.append("0 %d %d %d" % (len(data), fnv(data), fnv(expect.tobytes())))
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want


def test_the_files_are_the_pinned_bytes():
    pins = json.load(open(PINS))
    names = sorted(SMALL) + ["photo_800x450"]
    assert sorted(pins) == sorted("%s q%d" % (n, q) for n in names for q in E.QUALITIES)
    for n in names:
        for q in E.QUALITIES:
            assert hashlib.sha256(coded(n, q)[0]).hexdigest() == pins["%s q%d" % (n, q)], (n, q)


# ---- rate and quality against libwebp's own files (the photo-like 800 x 450 frame) ------------------------------------------------------
# D(q): this coder's PSNR minus libwebp's at the quality whose file is the smallest one not smaller than this coder's -- libwebp
# gets at least as many bytes.  Measured with Pillow 12.2.0 / libwebp 1.6.0 and recorded in DESIGN section 6; the test asserts
# D(q) >= recorded - 0.25 dB, so that a change that costs quality fails and a Pillow rebuild does not.
RECORDED_D = {0: {25: 0.66, 50: 0.53, 75: 0.54, 90: -0.11}, 4: {25: 0.12, 50: -0.09, 75: 0.12, 90: -0.28}}


def libwebp_curve(method):
    if ("curve", method) not in _CACHE:
        frame = E.photo_frame()
        _CACHE["curve", method] = [(len(d), E.psnr(p, frame)) for d, p in (E.pillow_lossy(frame, q, method) for q in range(0, 101))]
    return _CACHE["curve", method]


def measured_d(quality, method):
    data, expect, _ = coded("photo_800x450", quality)
    mine = E.psnr(expect, E.photo_frame())
    fits = [(size, p) for size, p in libwebp_curve(method) if size >= len(data)]
    assert fits, "libwebp has no file as large at any quality"
    return mine - min(fits)[1], len(data), mine


def test_size_and_psnr_rise_with_quality():
    frame = E.photo_frame()
    sizes = [len(coded("photo_800x450", q)[0]) for q in RATE_QUALITIES]
    psnrs = [E.psnr(coded("photo_800x450", q)[1], frame) for q in RATE_QUALITIES]
    print("sizes", sizes, "psnr", ["%.2f" % p for p in psnrs])
    assert sizes == sorted(sizes) and len(set(sizes)) == 4 and psnrs == sorted(psnrs) and len(set(psnrs)) == 4
    assert E.psnr(coded("photo_800x450", 100)[1], frame) > E.psnr(coded("photo_800x450", 0)[1], frame)


@pytest.mark.parametrize("method", [0, 4])
def test_psnr_at_equal_size_against_libwebp(method):
    for q in RATE_QUALITIES:
        d, size, mine = measured_d(q, method)
        print("quality %d: %d bytes, %.2f dB, D = %+.2f dB against method=%d" % (q, size, mine, d, method))
    for q in RATE_QUALITIES:
        assert measured_d(q, method)[0] >= RECORDED_D[method][q] - 0.25, (q, method)
