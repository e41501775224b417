"""tests/png_decode_oracle.py against Pillow, on the types where Pillow implements libpng's semantics: palette with and
without tRNS, RGB 8 with tRNS, 16-bit RGB (Pillow takes the high byte too), gray 1/2/4/8 without tRNS, gray+alpha 8 and
RGBA 8.

Pillow does NOT agree on gray + tRNS at low depth (it compares the key after scaling to 8 bits; libpng's png_set_expand
compares at the file's depth) and it reads 16-bit gray as I;16.  Those types, and GA16 / RGBA16, rest on the oracle alone:
on the PNG specification and libpng's documented transforms (expand, filler, strip_16 = the high byte, gray_to_rgb, bgr)."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

from tests import png_decode_oracle as O


def pillow_bgra(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    rgba = np.asarray(im.convert("RGBA"))
    return rgba[..., [2, 1, 0, 3]]


def make(ct, depth, w=13, h=11, interlace=False, filters=(0, 1, 2, 3, 4), trns=None, palette=None, seed=0):
    rng = np.random.default_rng(seed + ct * 100 + depth)
    s = O.random_samples(rng, w, h, ct, depth)
    if ct == 3 and palette is None:
        palette = rng.integers(0, 256, (1 << depth, 3), dtype=np.uint8)
    return O.write_png(s, ct, depth, filters=list(filters), interlace=interlace, palette=palette, trns=trns), s


@pytest.mark.parametrize("interlace", [False, True])
@pytest.mark.parametrize("ct,depth", [(3, 1), (3, 2), (3, 4), (3, 8), (0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (4, 8), (6, 8)])
def test_eight_bit_types_equal_pillow(ct, depth, interlace):
    data, _ = make(ct, depth, interlace=interlace)
    got, info = O.decode(data)
    assert np.array_equal(got, pillow_bgra(data))
    assert info["alpha_used"] == (ct in (3, 4, 6))


@pytest.mark.parametrize("depth", [1, 2, 4, 8])
def test_palette_trns_equals_pillow(depth):
    n = 1 << depth
    trns = bytes((i * 37) & 255 for i in range(max(1, n // 2)))       # shorter than the palette: 255 beyond
    data, _ = make(3, depth, trns=trns)
    got, info = O.decode(data)
    assert np.array_equal(got, pillow_bgra(data))
    assert info["alpha_used"] and (got[..., 3] != 255).any()


def test_rgb8_trns_equals_pillow_and_is_not_alpha_used():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 3, (9, 14, 3)).astype(np.uint32)
    data = O.write_png(s, 2, 8, filters=4, trns=struct.pack(">HHH", 1, 2, 0))
    got, info = O.decode(data)
    assert np.array_equal(got, pillow_bgra(data))
    assert (got[..., 3] == 0).sum() == int(np.all(s == [1, 2, 0], axis=2).sum()) > 0
    assert not info["alpha_used"]                                     # the quirk: real alpha bytes in a frame marked bgr_32


def test_rgb16_takes_the_high_byte_like_pillow():
    data, s = make(2, 16)
    got, _ = O.decode(data)
    assert np.array_equal(got[..., :3], pillow_bgra(data)[..., :3])
    assert np.array_equal(got[..., 2], (s[..., 0] >> 8).astype(np.uint8))


def test_types_that_rest_on_the_oracle_alone():
    # gray + tRNS at low depth: the key is compared at the file's depth
    s = np.arange(16, dtype=np.uint32).reshape(1, 16, 1) % 4
    got, info = O.decode(O.write_png(s, 0, 2, trns=struct.pack(">H", 2)))
    assert np.array_equal(got[0, :, 3], np.where(s[0, :, 0] == 2, 0, 255)) and np.array_equal(got[0, :, 0], s[0, :, 0] * 85)
    assert not info["alpha_used"]
    # 16-bit: the key at 16 bits, before the strip -- two samples with the same high byte, one of them the key
    s = np.array([[[0x1234], [0x12FF], [0x1234]]], np.uint32)
    got, _ = O.decode(O.write_png(s, 0, 16, trns=struct.pack(">H", 0x1234)))
    assert got[0, :, 3].tolist() == [0, 255, 0] and got[0, :, 0].tolist() == [0x12] * 3
    s = np.array([[[0xFFFF, 0x8001], [0x0100, 0x00FF]]], np.uint32)
    got, info = O.decode(O.write_png(s, 4, 16))
    assert got[0].tolist() == [[255, 255, 255, 0x80], [1, 1, 1, 0]] and info["alpha_used"]
    s = np.array([[[0xABCD, 0x0102, 0xFF00, 0x7FFF]]], np.uint32)
    got, _ = O.decode(O.write_png(s, 6, 16))
    assert got[0, 0].tolist() == [0xFF, 0x01, 0xAB, 0x7F]


def test_palette_index_beyond_plte_is_opaque_black():
    s = np.array([[[0], [3]]], np.uint32)
    got, _ = O.decode(O.write_png(s, 3, 2, palette=[[9, 8, 7], [1, 2, 3]]))
    assert got[0].tolist() == [[7, 8, 9, 255], [0, 0, 0, 255]]


def test_geometry_and_refusals():
    assert O.inflated_size(1, 1, 6, 8, True) == 5 and O.inflated_size(5, 5, 0, 1, False) == 10
    assert [O.pass_shape(5, 3, p) for p in range(7)] == [(1, 1), (1, 1), (2, 0), (1, 1), (3, 1), (2, 2), (5, 1)]
    data, _ = make(2, 8)
    bad = bytearray(data)
    bad[29] ^= 1                                                      # IHDR's CRC
    with pytest.raises(O.Malformed):
        O.decode(bytes(bad))
    for ct, depth in O.LEGAL:
        for interlace in (False, True):
            d, s = make(ct, depth, w=9, h=10, interlace=interlace, seed=5)
            got, _ = O.decode(d)
            assert got.shape == (10, 9, 4)
