"""tests/vp8_gen.py writes legal files: libwebp (through Pillow) decodes every one of them, to the size asked for, with an alpha
channel exactly where an ALPH chunk was written -- and the bool encoder's bytes are what a bool decoder reads back."""
import numpy as np
import pytest

from tests import vp8_gen as G
from tests import webp_frames as F
from tests.webp_decode_fixtures import pillow_refuses

FILES = G.option_files()


@pytest.mark.parametrize("name", sorted(FILES))
def test_pillow_decodes_every_generated_file(name):
    data = FILES[name]
    assert not pillow_refuses(data), name
    rgba, mode = F.pillow_decode(data)
    vp8 = G.chunk_body(data, b"VP8 ")
    w, h = (vp8[6] | vp8[7] << 8) & 0x3FFF, (vp8[8] | vp8[9] << 8) & 0x3FFF
    assert rgba.shape == (h, w, 4)
    assert mode == ("RGBA" if G.chunk_body(data, b"ALPH") is not None else "RGB"), name
    assert rgba[..., :3].std() > 5, name                                   # a picture, not one colour


def test_the_options_reach_the_file():
    def first_bits(name):
        vp8 = G.chunk_body(FILES[name], b"VP8 ")
        return vp8[0] | vp8[1] << 8 | vp8[2] << 16, vp8
    for p in (1, 2, 3):
        assert (first_bits("profile_%d" % p)[0] >> 1) & 7 == p
    _, vp8 = first_bits("scale_bits")
    assert vp8[7] >> 6 == 1 and vp8[9] >> 6 == 2
    for name in FILES:
        tag, vp8 = first_bits(name)
        assert tag & 1 == 0 and (tag >> 4) & 1 == 1 and vp8[3:6] == b"\x9d\x01\x2a" and 10 + (tag >> 5) < len(vp8), name
    for filt in range(4):
        assert G.chunk_body(FILES["alph_raw_f%d" % filt], b"ALPH")[0] == filt << 2
        assert G.chunk_body(FILES["alph_vp8l_f%d" % filt], b"ALPH")[0] == 1 | filt << 2


def test_the_alpha_planes_come_back_through_libwebp():
    for filt in range(4):
        for kind, seed in (("raw", filt), ("vp8l", 10 + filt)):
            rgba, _ = F.pillow_decode(FILES["alph_%s_f%d" % (kind, filt)])
            assert np.array_equal(rgba[..., 3], G.random_alpha(seed, G.W, G.H)), (kind, filt)


def test_the_bool_encoder_against_a_bool_decoder():
    """RFC 6386 7.3: what the encoder writes, the decoder of the same section reads"""
    rng = np.random.default_rng(5)
    bits, probs = rng.integers(0, 2, 4000), rng.integers(1, 256, 4000)
    e = G.BoolEncoder()
    for b, p in zip(bits, probs):
        e.put(int(b), int(p))
    data = e.finish() + b"\0\0"
    value, rng_, count, pos = data[0] << 8 | data[1], 255, 0, 2
    for b, p in zip(bits, probs):
        split = 1 + (((rng_ - 1) * int(p)) >> 8)
        big = split << 8
        if value >= big:
            got, rng_, value = 1, rng_ - split, value - big
        else:
            got, rng_ = 0, split
        while rng_ < 128:
            value, rng_, count = value << 1, rng_ << 1, count + 1
            if count == 8:
                count, value, pos = 0, value | data[pos], pos + 1
        assert got == b
