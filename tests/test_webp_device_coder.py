"""The device lossless-WebP coder's algorithm without a device (csrc/webp_encode_core.hpp: the predictors and their choice,
the parse, the five alphabets, code construction with its simple / fixed / Huffman forms, the headers, the layout's bit
offsets, bit placement, RIFF framing -- what the gfx950 kernels of csrc/webp_encode.hip are built from).
tests/webp_emulate.cpp runs the passes on the CPU; libwebp (through Pillow) AND tests/vp8l_reader.py must decode every file
to exactly the source pixels, and the reader must find the structure the coder claims.  The GPU tests
(tests/test_gpu_webp_encode.py) require the kernels' files to equal these byte for byte."""
import struct

import numpy as np
import pytest

from tests import webp_emulation as E
from tests import webp_frames as F
from tests.vp8l_reader import _predict, _prefix_value, read_vp8l

CASES = F.cases()
_FILES = {}


def emulated(name):
    """computed once, shared by the tests below"""
    if name not in _FILES:
        frame, alpha = CASES[name]
        _FILES[name] = E.encode(frame, alpha)
    return _FILES[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_libwebp_and_the_reader_decode_every_file_to_the_source(name):
    frame, alpha = CASES[name]
    data, st = emulated(name)
    want = F.rgba_of(frame, alpha)
    got, mode = F.pillow_decode(data)
    assert np.array_equal(got, want), name
    assert mode == ("RGBA" if alpha else "RGB")                     # alpha_is_used follows alpha_meaningful
    mine, info = read_vp8l(data)
    assert np.array_equal(mine, want), name
    assert info["alpha_is_used"] == (1 if alpha else 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_structure_layout_and_framing(name):
    frame, alpha = CASES[name]
    h, w = frame.shape[:2]
    data, st = emulated(name)
    _, info = read_vp8l(data)
    assert info["transforms"] == ["subtract_green", "predictor"] and info["tile_bits"] == [None, 4]
    assert info["color_cache_bits"] == 0
    bands = -(-h // 64)
    assert info["prefix_bits"] == 6 and info["groups"] == bands == st["groups"]
    assert np.array_equal(info["entropy_image"], np.repeat(np.arange(bands, dtype=np.uint32)[:, None], -(-w // 64), 1))   # one group per band
    assert info["bits"] == st["payload_bits"]                       # the layout's sum is what a decoder consumes
    assert info["head_bits"] == st["head_bits"]
    assert all(0 < d and (d == 1 or d == w) and 3 <= n <= 4096 for _, n, d in info["matches"])
    if st["constant_bands"] == 0 and st["literal_bands"] == 0:      # (such a band's parse is set aside: it is coded as literals)
        assert len(info["matches"]) == st["matches_left"] + st["matches_row"]
    payload = (st["payload_bits"] + 7) // 8
    assert data[:4] == b"RIFF" and data[8:16] == b"WEBPVP8L"
    assert struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and struct.unpack_from("<I", data, 16)[0] == payload
    assert len(data) == 20 + payload + (payload & 1) and len(data) % 2 == 0
    assert len(data) <= E.max_file_bytes(w, h)
    again, _ = E.encode(frame.copy(), alpha)
    assert again == data, "the same pixels give the same bytes"


def test_segments_and_bands_are_decoupled():
    g = E.shape(129, 64)
    assert (g["n_bands"], g["segs_per_band"], g["n_segs"]) == (1, 3, 3)
    _, st = emulated("three_segments")
    assert st["segments"] == 3 and st["second_segment_bit"] != 0, "the segment boundary of this frame is not byte-aligned"
    g = E.shape(40, 70)
    assert (g["n_bands"], g["segs_per_band"]) == (2, 1)
    assert E.shape(16384, 16384)["segs_per_band"] == 256 and E.shape(16384, 16384)["n_bands"] == 256


def test_one_colour_bands_take_one_symbol_codes_and_no_pixel_bits():
    data, st = emulated("black")
    _, info = read_vp8l(data)
    assert info["code_kinds"] == ["simple1"] * 5 and st["pixel_bits"] == 0 and st["constant_bands"] == 1
    assert info["bits"] == info["pixel_bits_start"]
    # any other colour: the first pixel's residual (against 0xFF000000) differs from the rest of its band, the other bands are one pixel throughout
    data, st = emulated("one_colour")
    _, info = read_vp8l(data)
    assert st["constant_bands"] == 2 and info["code_kinds"][5:] == ["simple1"] * 10
    assert st["pixel_bits"] <= 64 and len(data) < 120


def test_two_colours_use_simple_codes_where_two_symbols_suffice():
    data, st = emulated("two_colours")
    _, info = read_vp8l(data)
    assert "simple2" in info["code_kinds"] and "simple1" not in info["code_kinds"][1:4]


def test_runs_are_cut_at_4096_and_matches_reach_one_row_up():
    data, st = emulated("repeated_rows")
    _, info = read_vp8l(data)
    assert st["matches_4096"] >= 1 and max(n for _, n, _ in info["matches"]) == 4096
    assert all(p // 4096 == (p + n - 1) // 4096 for p, n, _ in info["matches"] if p < 64 * 130), "matches end at their segment's end"
    data, st = emulated("row_ramp")
    _, info = read_vp8l(data)
    assert st["matches_row"] > 0 and any(d == 61 for _, _, d in info["matches"])


def test_noise_takes_the_fixed_codes_and_stays_below_the_bound():
    frame, _ = CASES["noise"]
    h, w = frame.shape[:2]
    data, st = emulated("noise")
    assert st["fixed_codes"] >= 4, st                                # at least one channel in every group
    assert st["pixel_bits"] <= 32 * w * h                            # the flat-code floor
    assert len(data) <= E.max_file_bytes(w, h)
    assert E.encode(frame, True, cap=len(data) - 1) == (None, len(data))
    for (ww, hh) in ((1, 1), (16384, 1), (1, 16384), (64, 64), (65, 65)):
        g = E.shape(ww, hh)
        bits = 8 * (E.max_file_bytes(ww, hh) - 20)
        floor = 32 * ww * hh + 4 * g["tiles_x"] * g["tiles_y"] + 8 * g["ent_x"] * g["n_bands"] + 57 + 2 * (63 + 280 * 14 + 44)
        assert floor + 400 * g["n_bands"] <= bits <= floor + 1200 * g["n_bands"] + 15, (ww, hh)    # 32 bits a pixel, four flat-code headers a band


def test_a_band_larger_than_its_literals_is_written_as_literals():
    """the first band of this frame holds a match, so its green code needs length symbols and cannot be the flat one; the
    band as a whole falls back to literals under four flat codes: exactly 32 bits a pixel, which is what the bound rests on"""
    frame, _ = CASES["noise_with_a_run"]
    h, w = frame.shape[:2]
    data, st = emulated("noise_with_a_run")
    _, info = read_vp8l(data)
    assert st["matches_left"] >= 1 and st["literal_bands"] >= 1
    assert not any(p < 64 * w for p, _, _ in info["matches"]), "the band's matches are set aside"
    assert st["pixel_bits"] <= 32 * w * h and len(data) <= E.max_file_bytes(w, h)


def test_bands_of_matches_only_get_complete_codes():
    """behind the first band every pixel of this frame is inside a match one row up: green alphabets of length symbols alone"""
    frame, _ = CASES["row_ramp_tall"]
    data, st = emulated("row_ramp_tall")
    _, info = read_vp8l(data)
    later = [(p, n, d) for p, n, d in info["matches"] if p >= 64 * 61]
    assert sum(n for _, n, _ in later) == (140 - 64) * 61 and all(d == 61 for _, _, d in later)


def test_predictors_and_prefix_values_agree_with_the_reader():
    """csrc/webp_encode_core.hpp against the reader's own arithmetic, which is pinned to libwebp (tests/test_vp8l_reader.py)"""
    lib, rng = E.emulator(), np.random.default_rng(17)
    px = rng.integers(0, 2 ** 32, (300, 4), dtype=np.uint64)
    px[:40] &= 0x03030303                                            # small values: the clamps and the halving's sign
    px[40:80] |= 0xFCFCFCFC
    for L, T, TL, TR in px.tolist():
        for mode in range(14):
            assert lib.webp_emu_predict(mode, L, T, TL, TR) == _predict(mode, L, T, TL, TR), (mode, L, T, TL)
    assert lib.webp_emu_predict(13, 0x00000000, 0x00000000, 0x01010101, 0) == 0                  # (0 - 1) / 2 is 0, not -1
    assert lib.webp_emu_predict(13, 0x0A0A0A0A, 0x0A0A0A0A, 0x0D0D0D0D, 0) == 0x09090909         # 10 + (-3) / 2 = 9

    class Extra:
        def __init__(self, v):
            self.v = v

        def read(self, n):
            return self.v
    out = np.zeros(3, np.uint32)
    for v in list(range(1, 300)) + [1023, 1024, 1025, 4095, 4096]:
        lib.webp_emu_prefix(v, out.ctypes.data)
        sym, ebits, extra = (int(t) for t in out)
        assert sym < 24 and ebits == (0 if sym < 4 else (sym - 2) >> 1) and _prefix_value(Extra(extra), sym) == v
