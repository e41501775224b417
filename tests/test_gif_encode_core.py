"""The device GIF coder's algorithm without a device (csrc/gif_encode_core.hpp: the segment coder with its hash table, the
gather of the segments' bits, the sub-block positions, the head -- what the gfx950 kernels of csrc/gif_encode.hip are built
from; the palette is the quantiser's of csrc/png_quantize_core.hpp under the GIF key rule).  tests/gif_encode_emulate.cpp
runs the passes on the CPU over slots and a stream of exactly the device's sizes.  Two independent decoders read what comes
out: Pillow, and this project's own (tests/gif_oracle.py and the CPU emulation of its device decoder,
tests/gif_decode_emulate.cpp).  The GPU tests (tests/test_gpu_gif_encode.py) hold the kernels to this emulation byte for byte.

Measured with Pillow 12.2.0 on the photo-like 150 x 130 frame at 256 colours, segments of 16384 pixels: this coder's file
13 175 bytes, Pillow's GIF of the same palette and indices 14 366 bytes."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import gif_encode_emu as G
from tests import gif_oracle as O

CASES = G.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_decoders_read_what_the_coder_chose(name):
    rgba, alpha = CASES[name]
    h, w, _ = rgba.shape
    q = G.encode(rgba, alpha=alpha)
    assert q["status"] == 0 and q["file"] is not None
    assert len(q["file"]) <= G.max_file_bytes(w, h), "the arithmetic bound holds"
    assert q["segments"] == -(-w * h // G.segment_pixels())
    info = G.check_file(q, w, h)
    assert "loop" not in info, "no NETSCAPE2.0 block unless a repeat count is given"
    assert int(q["indices"].max()) < len(q["palette"]) <= 256
    assert q["min_code"] == max(2, (len(q["palette"]) - 1).bit_length())
    if q["n_trans"]:
        assert q["n_trans"] == 1 and q["palette"][0].tolist() == [0, 0, 0, 0], "the transparent entry is first"
        assert (q["palette"][1:, 3] == 255).all()
    else:
        assert (q["palette"][:, 3] == 255).all()


@pytest.mark.parametrize("name", ["one_colour", "two_colours", "256_colours", "alpha_edge_meaningful", "alpha_edge_ignored", "all_transparent", "photo_3x5"])
def test_at_most_256_colours_after_the_alpha_rule_are_kept_exactly(name):
    rgba, alpha = CASES[name]
    q = G.encode(rgba, alpha=alpha)
    src = G.normalized(rgba, alpha)
    assert sorted(map(tuple, q["palette"])) == sorted(map(tuple, np.unique(src.reshape(-1, 4), axis=0)))
    assert np.array_equal(G.decoded(q), src)


def test_the_alpha_rule():
    rgba = G.alpha_edge_frame()
    q = G.encode(rgba, alpha=True)
    out = G.decoded(q)
    assert (out[:, [0, 1, 4, 6], 3] == 0).all() and not out[:, [0, 1, 4, 6], :3].any(), "alpha 0, 1, 15: the transparent entry"
    assert (out[:, [2, 3, 5, 7], 3] == 255).all(), "alpha 16 and above: opaque"
    assert np.array_equal(out[:, [2, 3, 5, 7], :3], rgba[:, [2, 3, 5, 7], :3])
    plain = G.encode(rgba, alpha=False)                                  # bgr_32: no transparent entry at all
    assert plain["n_trans"] == 0 and np.array_equal(G.decoded(plain)[..., :3], rgba[..., :3])
    rgba, _ = CASES["all_transparent"]
    q = G.encode(rgba, alpha=True)
    assert q["palette"].tolist() == [[0, 0, 0, 0]] and q["min_code"] == 2 and not q["indices"].any()


def test_one_and_two_colours_have_minimum_code_size_2():
    for name in ("one_colour", "two_colours"):
        q = G.encode(CASES[name][0], alpha=False)
        fr = O.parse(q["file"])["frames"][0]
        assert q["min_code"] == 2 and fr["m"] == 2 and len(fr["palette"]) == 2


def test_257_colours_leave_256_entries():
    q = G.encode(CASES["257_colours"][0], alpha=False)
    assert len(q["palette"]) == 256 and q["min_code"] == 8


def test_the_noise_frame_fills_the_table_inside_a_segment():
    rgba, _ = CASES["noise_128x130"]
    q = G.encode(rgba, alpha=False)
    fr = O.parse(q["file"])["frames"][0]
    from tests import gif_gen
    clears, k, pos, width = 0, 0, 0, 9
    acc = int.from_bytes(fr["stream"], "little")
    while True:                                                           # the codes with the width rule of the decoder
        width = gif_gen.width_at(8, k)
        c = (acc >> pos) & ((1 << width) - 1)
        pos += width
        if c == 257:
            break
        if c == 256:
            clears, k = clears + 1, 0
        else:
            k += 1
            assert k <= 4094 - 256, "a clear follows the code that would make entry 4095"
    assert clears > q["segments"], "more clear codes than segments: a table filled inside a segment"


@pytest.mark.parametrize("residue", [0, 1, 254])
def test_data_lengths_at_the_sub_block_boundaries(residue):
    rgba = G.modulo_frames()[residue]
    h, w, _ = rgba.shape
    q = G.encode(rgba, alpha=False)
    assert q["data_bytes"] % 255 == residue
    G.check_file(q, w, h)
    data = q["file"]
    at = data.index(b"\x21\xf9\x04") + 8                             # the image descriptor behind the graphic control extension
    assert data[at] == 0x2C
    at += 10 + 3 * max(2, 1 << (len(q["palette"]) - 1).bit_length()) + 1
    sizes = []
    while data[at]:
        sizes.append(data[at])
        at += 1 + data[at]
    assert data[at:] == b"\x00\x3b"
    full, rest = divmod(q["data_bytes"], 255)
    assert sizes == [255] * full + ([rest] if rest else []), "no empty sub-block in front of the terminator"


def test_the_file_is_no_larger_than_pillows_of_the_same_palette_and_indices():
    rgba, _ = CASES["photo_150x130"]
    q = G.encode(rgba, alpha=False)
    im = Image.fromarray(q["indices"], "P")
    im.putpalette(q["palette"][:, :3].tobytes())
    buf = io.BytesIO()
    im.save(buf, "GIF")
    print(f"photo 150x130, 256 colours, segments of {G.segment_pixels()}: this coder {len(q['file'])} bytes, Pillow {buf.tell()} bytes")
    assert len(q["file"]) <= buf.tell(), "the kept segment length costs more bytes than Pillow's whole file"


def test_repeat_delay_and_user_input_reach_the_head():
    rgba, _ = CASES["photo_3x5"]
    plain = G.encode(rgba, alpha=False)
    for repeat, delay, user in ((0, 0, False), (3, 7, False), (65535, 65535, True)):
        q = G.encode(rgba, alpha=False, repeat=repeat, delay=delay, user_input=user)
        info = G.check_file(q, 3, 5)
        assert info["loop"] == repeat and info.get("duration", 0) == delay * 10
        assert len(q["file"]) == len(plain["file"]) + 19
        at = q["file"].index(b"\x21\xf9\x04")
        assert q["file"][at + 3] == (4 | (2 if user else 0)), "disposal keep, the user-input flag, no transparent index"
    t = G.encode(CASES["all_transparent"][0], alpha=True)
    at = t["file"].index(b"\x21\xf9\x04")
    assert t["file"][at + 3] == 5 and t["file"][at + 6] == 0, "the transparent flag and index 0"


def test_same_pixels_same_bytes_whatever_the_stride_and_a_short_buffer_is_an_overflow():
    rgba, _ = CASES["photo_17x40"]
    a = G.encode(rgba, alpha=False)
    b = G.encode(rgba, alpha=False, stride=4 * 17 + 24)
    assert a["file"] == b["file"]
    short = G.encode(rgba, alpha=False, cap=len(a["file"]) - 1)
    assert short["status"] == G.FILE_OVERFLOW and short["file"] is None
    assert G.encode(rgba, alpha=False, cap=len(a["file"]))["file"] == a["file"]


def test_max_file_bytes_is_the_documented_arithmetic():
    S = G.segment_pixels()
    for w, h in ((1, 1), (800, 450), (3840, 2160), (65535, 4096)):
        n = w * h
        codes = n + n // (4094 - 256) + 2 * -(-n // S)               # a code per pixel, a clear per full table, two per segment
        data = -(-codes * 12 // 8)
        assert G.max_file_bytes(w, h) == (6 + 7 + 19 + 8 + 10 + 768 + 1) + data + -(-data // 255) + 2
