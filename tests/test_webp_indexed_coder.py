"""The colour indexing of the device lossless-WebP coder without a device (csrc/webp_encode_core.hpp: the sorted palette, the
bundling of 8, 4 or 2 indices into a pixel, the indexed stream's head, the choice between the indexed and the plain file --
what the gfx950 kernels of csrc/webp_encode_indexed.hip are built from).  tests/webp_indexed_emulate.cpp runs the coder with
its stage flags on the CPU; libwebp (through Pillow) AND tests/vp8l_reader.py must decode every file to exactly the source
pixels, and the reader must find the structure the coder claims.  The GPU tests (tests/test_gpu_webp_encode_indexed.py)
require the kernels' files to equal these byte for byte."""
import struct

import numpy as np
import pytest

from tests import webp_emulation as PLAIN
from tests import webp_frames as F
from tests import webp_indexed_emulation as E
from tests import webp_indexed_frames as X
from tests.vp8l_reader import read_vp8l

CASES = F.cases()
FRAMES = X.frames()
_FILES, _PLAIN = {}, {}


def indexed(name):
    """the flag-on file of a frame and its counters, computed once"""
    if name not in _FILES:
        frame, alpha = FRAMES[name]
        _FILES[name] = E.encode(frame, alpha, E.COLOR_INDEXING)
    return _FILES[name]


def plain(name):
    if name not in _PLAIN:
        frame, alpha = FRAMES[name]
        _PLAIN[name] = PLAIN.encode(frame, alpha)
    return _PLAIN[name]


def palette_size(data):
    """the colour table's size as the stream states it: 8 bits behind the 40 of the image header, the transform bit and type 3"""
    bits = int.from_bytes(data[20:28], "little")
    assert (bits >> 40) & 1 == 1 and (bits >> 41) & 3 == 3
    return ((bits >> 43) & 255) + 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_flags_zero_is_the_plain_emulation_byte_for_byte(name):
    frame, alpha = CASES[name]
    data, st = E.encode(frame, alpha, 0)
    want, want_st = plain(name)
    assert data == want
    assert st["indexed"] == 0 and st["colours"] == 0 and st["indexed_bytes"] == 0
    assert all(st[k] == want_st[k] for k in PLAIN.STATS)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_libwebp_and_the_reader_decode_every_flag_on_file_to_the_source(name):
    frame, alpha = FRAMES[name]
    h, w = frame.shape[:2]
    data, st = indexed(name)
    want = F.rgba_of(frame, alpha)
    got, mode = F.pillow_decode(data)
    assert np.array_equal(got, want), name
    assert mode == ("RGBA" if alpha else "RGB")                     # alpha_is_used follows alpha_meaningful
    mine, info = read_vp8l(data)
    assert np.array_equal(mine, want), name
    assert info["alpha_is_used"] == (1 if alpha else 0)
    colours = X.colours_of(frame, alpha)
    assert st["colours"] == (colours if colours <= 256 else 0)
    assert st["indexed"] == (1 if 0 < st["indexed_bytes"] < st["plain_bytes"] else 0)
    assert len(data) == (st["indexed_bytes"] if st["indexed"] else st["plain_bytes"])
    if st["indexed"]:
        bits = E.emulator().webp_ix_index_width_bits(colours)
        assert info["transforms"] == ["color_indexing"] and info["tile_bits"] == [bits] == [st["width_bits"]]
        assert palette_size(data) == colours
        packed = -(-w // (1 << bits))
        assert st["packed_width"] == packed
        bands = -(-h // 64)
        assert info["prefix_bits"] == 6 and info["groups"] == bands == st["groups"]
        assert np.array_equal(info["entropy_image"], np.repeat(np.arange(bands, dtype=np.uint32)[:, None], -(-packed // 64), 1))
        assert all(d == 1 or d == packed for _, n, d in info["matches"])   # one row up is the packed width
    else:
        assert info["transforms"] == ["subtract_green", "predictor"]
        assert data == plain(name)[0]
    assert info["color_cache_bits"] == 0
    assert info["bits"] == st["payload_bits"] and info["head_bits"] == st["head_bits"]
    payload = (st["payload_bits"] + 7) // 8
    assert data[:4] == b"RIFF" and data[8:16] == b"WEBPVP8L"
    assert struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and struct.unpack_from("<I", data, 16)[0] == payload
    assert len(data) == 20 + payload + (payload & 1)


@pytest.mark.parametrize("n,bits", list(zip(X.EDGE_COLOURS, X.EDGE_BITS)))
def test_bundling_at_the_edges_of_the_palette_sizes(n, bits):
    """37 is no multiple of 8, 4 or 2: the last bundle of every row is partly filled.  (One colour is sized like the others
    and then written plain: that file is five one-symbol codes already, and a tie goes to the plain file.)"""
    data, st = indexed("exactly_%d" % n)
    assert st["colours"] == n and st["width_bits"] == bits and st["packed_width"] == -(-37 // (1 << bits)) and st["indexed_bytes"] > 0
    assert st["indexed"] == (1 if n > 1 else 0)
    if st["indexed"]:
        assert read_vp8l(data)[1]["tile_bits"] == [bits] and palette_size(data) == n


@pytest.mark.parametrize("name,packed", [("width_1_two", 1), ("width_7_two", 1), ("height_1", 10)])
def test_bundles_of_narrow_and_flat_frames(name, packed):
    data, st = indexed(name)
    assert st["indexed"] == 1 and st["packed_width"] == packed
    assert np.array_equal(F.pillow_decode(data)[0], F.rgba_of(FRAMES[name][0]))


def test_257_colours_give_the_plain_file():
    data, st = indexed("colours_257")
    assert st["indexed"] == 0 and st["colours"] == 0 and st["indexed_bytes"] == 0
    assert data == plain("colours_257")[0]


def test_garbage_alpha_does_not_count_as_colours():
    frame, alpha = FRAMES["bgrx_few"]
    assert not alpha and X.colours_of(frame, True) > 256
    data, st = indexed("bgrx_few")
    assert st["indexed"] == 1 and st["colours"] == 5 and palette_size(data) == 5 and st["width_bits"] == 1
    got, info = read_vp8l(data)
    assert info["alpha_is_used"] == 0 and np.all(got[..., 3] == 255)         # the palette's own alpha, not a decoder's fill
    assert np.array_equal(got, F.rgba_of(frame, False))


@pytest.mark.parametrize("name,is_indexed", [("two_colours", 1), ("transparent_few", 1), ("transparent_rgb", 0)])
def test_meaningful_alpha_lives_in_the_palette(name, is_indexed):
    """(transparent_rgb's 216 colours on 216 pixels make a table larger than what it saves: sized, and written plain)"""
    frame, alpha = FRAMES[name]
    data, st = indexed(name)
    assert alpha and st["indexed"] == is_indexed and st["indexed_bytes"] > 0
    got, info = read_vp8l(data)
    assert info["alpha_is_used"] == 1 and np.array_equal(got, F.rgba_of(frame))
    assert np.array_equal(F.pillow_decode(data)[0], F.rgba_of(frame))          # the RGB under alpha 0 survives
    assert got[..., 3].min() < 255


def test_bands_and_segments_follow_the_packed_image():
    data, st = indexed("packed_bands")
    assert st["indexed"] == 1 and st["width_bits"] == 1 and st["packed_width"] == 150
    assert st["groups"] == 3 and st["segments"] == 9                  # 150 x 64 pixels: segments of 4096, 4096 and 1408
    assert st["matches_row"] > 0 and st["matches_left"] > 0
    data, st = indexed("unbundled_200")
    assert st["indexed"] == 1 and st["width_bits"] == 0 and st["packed_width"] == 96 and st["colours"] == 200


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_the_flag_never_makes_a_file_larger(name):
    assert len(indexed(name)[0]) <= len(plain(name)[0])
    assert indexed(name)[1]["plain_bytes"] == len(plain(name)[0])


@pytest.mark.parametrize("name,parent", [("few_96x80", 13274), ("few_70x66_17", 8924)])
def test_busy_graphics_of_few_colours_halve(name, parent):
    """An order-0 estimate of the bundled indices with the palette and the heads is about 2960 and 2520 bytes: well under half
    of the plain coder's files, whose sizes are pinned here as the flag-off coder writes them."""
    assert len(plain(name)[0]) == parent
    data, st = indexed(name)
    assert st["indexed"] == 1 and 2 * len(data) <= parent, (len(data), parent)
