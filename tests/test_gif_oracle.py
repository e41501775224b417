"""tests/gif_oracle.py pinned: its serial LZW decoder gives Pillow's indices on files Pillow's own encoder wrote (interlaced and
not, 2 to 256 colours, photo-like, flat and noise), and its statement of Screen::blit / Disposal gives hand-checked screens on
tiny animations."""
import io

import numpy as np
import pytest

from tests import gif_gen as G
from tests import gif_oracle as O

PIL = pytest.importorskip("PIL.Image")


def pillow_written(idx, palette, interlace):
    im = PIL.fromarray(np.asarray(idx, np.uint8), "P")
    im.putpalette(np.asarray(palette, np.uint8).ravel().tolist())
    buf = io.BytesIO()
    im.save(buf, "GIF", interlace=interlace, optimize=False)
    return buf.getvalue()


def pillow_indices(data):
    im = PIL.open(io.BytesIO(data))
    im.load()
    assert im.mode in ("P", "L")
    return np.asarray(im)


CASES = [("noise256", G.noise(301, 97, 256, 1), 256), ("noise16", G.noise(64, 64, 16, 2), 16), ("noise2", G.noise(33, 17, 2, 3), 2),
         ("runs64", G.runs(120, 80, 64, 4), 64), ("flat", np.zeros((90, 130), np.uint8), 4), ("one", np.ones((1, 1), np.uint8), 2),
         ("column", G.noise(1, 50, 8, 5), 8), ("row", G.noise(50, 1, 8, 6), 8)]


@pytest.mark.parametrize("interlace", [False, True])
@pytest.mark.parametrize("name,idx,colours", CASES, ids=[c[0] for c in CASES])
def test_lzw_decoder_gives_pillows_indices_on_pillow_written_files(name, idx, colours, interlace):
    data = pillow_written(idx, G.palette_of(colours), interlace)
    P = O.parse(data)
    assert P["status"] == O.OK and len(P["frames"]) == 1
    assert P["frames"][0]["interlace"] == (interlace and min(idx.shape) >= 16)        # (Pillow's writer leaves small images progressive)
    st, got = O.frame_indices(P["frames"][0])
    assert st == O.OK
    assert np.array_equal(got, pillow_indices(data)) and np.array_equal(got, idx)


def test_the_noise_frame_holds_several_clear_codes():
    data = pillow_written(G.noise(301, 97, 256, 1), G.palette_of(256), False)
    fr = O.parse(data)["frames"][0]
    acc, pos, k, clears = int.from_bytes(fr["stream"], "little"), 0, 0, 0
    while pos + 12 <= len(fr["stream"]) * 8:
        w = G.width_at(8, k)
        c = (acc >> pos) & ((1 << w) - 1)
        pos += w
        k += 1
        if c == 256:
            clears, k = clears + 1, 0
        elif c == 257:
            break
    assert clears >= 8


R, Gn, B, W = (0, 0, 255, 255), (0, 255, 0, 255), (255, 0, 0, 255), (255, 255, 255, 255)      # BGRA
PAL = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)], np.uint8)


def screen(rows):
    return np.array(rows, np.uint8)


def test_blit_and_disposal_on_hand_checked_cases():
    # a 3 x 2 screen, background white (index 3); frame 0 red everywhere, frame 1 a green pixel at (1, 0), frame 2 a blue pixel at (2, 1)
    def files(d0, d1):
        f0 = G.frame(np.zeros((2, 3), np.uint8), 3, 2, m=2, dispose=d0)
        f1 = G.frame(np.ones((1, 1), np.uint8), 1, 1, left=1, top=0, m=2, dispose=d1)
        f2 = G.frame(np.full((1, 1), 2, np.uint8), 1, 1, left=2, top=1, m=2)
        return G.gif(3, 2, [f0, f1, f2], palette=PAL, bg=3)
    keep = files(O.KEEP, O.KEEP)
    assert np.array_equal(O.decode(keep, 0)[1], screen([[R, R, R], [R, R, R]]))
    assert np.array_equal(O.decode(keep, 1)[1], screen([[R, Gn, R], [R, R, R]]))
    assert np.array_equal(O.decode(keep, 2)[1], screen([[R, Gn, R], [R, R, B]]))
    back = files(O.BACKGROUND, O.BACKGROUND)                                  # frame 0's whole rectangle goes white before frame 1
    assert np.array_equal(O.decode(back, 1)[1], screen([[W, Gn, W], [W, W, W]]))
    assert np.array_equal(O.decode(back, 2)[1], screen([[W, W, W], [W, W, B]]))
    prev = files(O.KEEP, O.PREVIOUS)                                          # frame 1's pixel goes back to red before frame 2
    assert np.array_equal(O.decode(prev, 2)[1], screen([[R, R, R], [R, R, B]]))
    first_prev = files(O.PREVIOUS, O.KEEP)                                    # what lay under frame 0 was the background
    assert np.array_equal(O.decode(first_prev, 1)[1], screen([[W, Gn, W], [W, W, W]]))
    assert O.decode(keep, 3)[0] == O.NO_SUCH_FRAME


def test_transparency_palettes_and_clipping_on_hand_checked_cases():
    idx = np.array([[0, 1], [2, 3]], np.uint8)
    T = (0, 0, 0, 0)
    # transparent index 1 over the white background; index 3 of a two-entry local palette is beyond it: (0,0,0,0)
    data = G.gif(2, 2, [G.frame(idx, 2, 2, m=2, transparent=1, palette=PAL[:2])], palette=PAL, bg=3)
    assert np.array_equal(O.decode(data)[1], screen([[R, W], [T, T]]))
    # no global palette: the screen starts as (0,0,0,0), whatever the background index says
    data = G.gif(3, 2, [G.frame(idx, 2, 2, m=2, palette=PAL)], bg=1)
    assert np.array_equal(O.decode(data)[1], screen([[R, Gn, T], [B, W, T]]))
    # a background index beyond the global palette: (0,0,0,0)
    data = G.gif(3, 2, [G.frame(idx, 2, 2, m=2)], palette=PAL, bg=9)
    assert np.array_equal(O.decode(data)[1], screen([[R, Gn, T], [B, W, T]]))
    # a frame hanging over the right and bottom edges: its left column and top row land
    data = G.gif(3, 2, [G.frame(idx, 2, 2, left=2, top=1, m=2)], palette=PAL, bg=3)
    assert np.array_equal(O.decode(data)[1], screen([[W, W, W], [W, W, R]]))
    # wholly off the canvas: the background alone
    data = G.gif(3, 2, [G.frame(idx, 2, 2, left=3, top=0, m=2)], palette=PAL, bg=3)
    assert np.array_equal(O.decode(data)[1], screen([[W, W, W], [W, W, W]]))
    # neither palette: the frame must have _some_ palette
    assert O.decode(G.gif(2, 2, [G.frame(idx, 2, 2, m=2)]))[0] == O.NO_PALETTE


def test_interlace_row_map():
    assert O.row_map(1) == [0] and O.row_map(5) == [0, 4, 2, 1, 3] and O.row_map(9) == [0, 8, 4, 2, 6, 1, 3, 5, 7]
