"""The GIF decoder's corpus: small files from tests/gif_gen.py, one per way the kernels can go wrong, each with the frame it is
decoded to.  good_files() -> {name: (file, frame_index)}; damaged_files() -> {name: (file, frame_index, status)}; expected(name)
is the oracle's screen (tests/gif_oracle.py), computed once.  No frame is larger than 300 x 200."""
import functools
import os

import numpy as np

from tests import gif_gen as G
from tests import gif_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gif")
RGB = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)]


def one(idx, m, colours=None, w=None, h=None, **kw):
    idx = np.asarray(idx, np.uint8)
    h, w = (h, w) if w is not None else idx.shape
    n = max(2, colours or (1 << m))
    return G.gif(w, h, [G.frame(idx, w, h, m=m, **kw)], palette=G.palette_of(1 << (n - 1).bit_length()))


def animation(dispose, offscreen=False):
    """three frames over a 12 x 9 screen with one disposal method each; the second lies partly off the canvas when asked"""
    pal = G.palette_of(8, 3)
    a = G.frame(G.noise(12, 9, 8, 1), 12, 9, m=3, dispose=dispose[0])
    b = G.frame(G.noise(7, 5, 8, 2), 7, 5, left=8 if offscreen else 3, top=6 if offscreen else 2, m=3, dispose=dispose[1], transparent=2)
    c = G.frame(G.noise(5, 4, 8, 3), 5, 4, left=1, top=4, m=3, dispose=dispose[2], transparent=5, palette=G.palette_of(8, 4))
    return G.gif(12, 9, [a, b, c], palette=pal, bg=6)


def rgb_animation():
    """the shape of the reference's tests/integration/visuals/animation.rs: a 4 x 4 screen, a red, a green and a blue frame"""
    frames = [G.frame(np.full((4, 4), k, np.uint8), 4, 4, m=2, delay=10) for k in range(3)]
    return G.gif(4, 4, frames, palette=np.array(RGB, np.uint8))


@functools.lru_cache(maxsize=None)
def good_files():
    out = {}
    for m in range(1, 9):
        out["m%d_noise" % m] = (one(G.noise(37, 23, 1 << m, m), m), 0)
        out["m%d_runs" % m] = (one(G.runs(37, 23, 1 << m, 10 + m), m), 0)
    big2, big8 = G.noise(150, 100, 4, 20), G.noise(200, 150, 256, 21)
    out["widths_m2_clear_at_full"] = (one(big2, 2), 0)                       # every width 3..12, the table fills, a clear exactly there
    out["widths_m8_clear_at_full"] = (one(big8, 8), 0)
    out["clear_early"] = (one(big8, 8, segments=[1000]), 0)
    out["two_clears_in_a_row"] = (one(big8, 8, segments=[700], double_clear=True), 0)
    out["deferred_m8_long_tail"] = (one(big8, 8, deferred=True), 0)          # 3 838 codes fill the table; the tail is far beyond one chunk
    out["deferred_m2_long_tail"] = (one(G.noise(300, 200, 4, 22), 2, deferred=True), 0)
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257):
        out["clear_at_%d" % n] = (one(G.noise(61, 47, 16, n), 4, segments=[n]), 0)
        out["end_at_%d" % n] = (one(G.noise(n, 1, 16, n), 4, literal_only=True), 0)
    for n in (4095, 4096, 4097, 5119, 5120, 5121):                            # the first chunk's and a tail chunk's last code
        out["clear_at_%d" % n] = (one(big8, 8, segments=[n]), 0)
    out["mixed_segments"] = (one(G.runs(120, 90, 32, 5), 5, segments=[1, 2, 64, 1, 300, 65, 5000]), 0)
    out["flat_kwkwk_chain"] = (one(np.zeros((200, 300), np.uint8), 2), 0)    # KwKwK as the second code, then chains as long as they get
    out["flat_deferred"] = (one(np.full((200, 300), 3, np.uint8), 2, deferred=True), 0)
    out["no_leading_clear"] = (one(G.runs(61, 47, 16, 6), 4, leading_clear=False), 0)
    out["no_end_code"] = (one(G.runs(61, 47, 16, 7), 4, end_code=False), 0)
    idx = G.runs(61, 47, 16, 8)
    stream = G.lzw_stream(idx.ravel(), 4) + bytes(range(1, 40))
    out["bytes_after_the_end_code"] = (G.gif(61, 47, [G.frame(None, 61, 47, m=4, stream=stream)], palette=G.palette_of(16)), 0)
    stream = G.lzw_stream(np.concatenate([idx.ravel(), G.noise(50, 1, 16, 9).ravel()]), 4)
    out["more_indices_than_pixels"] = (G.gif(61, 47, [G.frame(None, 61, 47, m=4, stream=stream)], palette=G.palette_of(16)), 0)
    for w, h in ((1, 1), (1, 37), (37, 1), (2, 2), (3, 5), (299, 7)):
        out["size_%dx%d" % (w, h)] = (one(G.noise(w, h, 8, w + h), 3), 0)
    for h in list(range(1, 10)) + [37]:
        out["interlaced_h%d" % h] = (one(G.noise(13, h, 8, 40 + h), 3, interlace=True), 0)
    out["small_sub_blocks"] = (one(G.noise(37, 23, 16, 50), 4, block=7), 0)
    # palettes
    g, loc = G.palette_of(8, 1), G.palette_of(8, 2)
    idx = G.noise(9, 7, 8, 60)
    out["local_over_global"] = (G.gif(9, 7, [G.frame(idx, 9, 7, m=3, palette=loc)], palette=g), 0)
    out["no_global_palette"] = (G.gif(9, 7, [G.frame(idx, 9, 7, m=3, palette=loc)]), 0)
    out["index_beyond_the_palette"] = (G.gif(9, 7, [G.frame(idx, 9, 7, m=3)], palette=G.palette_of(4)), 0)
    out["transparent_index"] = (G.gif(9, 7, [G.frame(idx, 9, 7, m=3, transparent=3)], palette=g, bg=1), 0)
    out["background_beyond_the_palette"] = (G.gif(12, 9, [G.frame(idx, 9, 7, left=2, top=1, m=3)], palette=g, bg=200), 0)
    out["gif87a_with_extensions"] = (G.gif(9, 7, [G.frame(idx, 9, 7, m=3)], palette=g, version=b"GIF87a",
                                           extensions=b"\x21\xFF\x0BNETSCAPE2.0\x03\x01\x00\x00\x00" + b"\x21\xFE\x05hello\x00" + b"\x21\x42\x02ab\x00"), 0)
    out["no_trailer"] = (G.gif(9, 7, [G.frame(idx, 9, 7, m=3)], palette=g, trailer=False), 0)
    # compositing
    out["frame_partly_off_the_canvas"] = (G.gif(10, 8, [G.frame(G.noise(9, 7, 8, 61), 9, 7, left=4, top=5, m=3)], palette=g, bg=2), 0)
    out["frame_wholly_off_the_canvas"] = (G.gif(10, 8, [G.frame(G.noise(9, 7, 8, 62), 9, 7, left=10, top=3, m=3)], palette=g, bg=2), 0)
    out["frame_beyond_the_corner"] = (G.gif(10, 8, [G.frame(G.noise(9, 7, 8, 63), 9, 7, left=60000, top=60000, m=3)], palette=g, bg=2), 0)
    zero = G.frame(None, 0, 0, m=3, stream=G.pack_tokens([("clear",), ("end",)], 3))
    out["zero_size_frame_then_one"] = (G.gif(10, 8, [zero, G.frame(G.noise(9, 7, 8, 64), 9, 7, m=3)], palette=g, bg=2), 1)
    out["zero_size_frame_alone"] = (G.gif(10, 8, [zero], palette=g, bg=2), 0)
    for name, dispose in (("keep", (O.KEEP, O.KEEP, O.KEEP)), ("background", (O.BACKGROUND, O.BACKGROUND, O.KEEP)), ("previous", (O.KEEP, O.PREVIOUS, O.PREVIOUS)),
                          ("mixed", (O.PREVIOUS, O.BACKGROUND, O.ANY))):
        for target in range(3):
            out["dispose_%s_frame%d" % (name, target)] = (animation(dispose), target)
    out["dispose_background_off_the_canvas_frame2"] = (animation((O.KEEP, O.BACKGROUND, O.KEEP), offscreen=True), 2)
    out["dispose_previous_off_the_canvas_frame2"] = (animation((O.KEEP, O.PREVIOUS, O.KEEP), offscreen=True), 2)
    for target in range(3):
        out["rgb_animation_frame%d" % target] = (rgb_animation(), target)
    return out


@functools.lru_cache(maxsize=None)
def damaged_files():
    idx = G.runs(61, 47, 16, 70)
    pal = G.palette_of(16)
    stream = G.lzw_stream(idx.ravel(), 4)
    out = {}

    def with_stream(s, m=4, **kw):
        return G.gif(61, 47, [G.frame(None, 61, 47, m=m, stream=s, **kw)], palette=pal)
    out["too_little_cut"] = (with_stream(stream[:len(stream) // 2]), 0, O.TOO_LITTLE)
    out["too_little_early_end"] = (with_stream(G.lzw_stream(idx.ravel()[:-1], 4)), 0, O.TOO_LITTLE)
    out["too_little_empty"] = (with_stream(b""), 0, O.TOO_LITTLE)
    tokens = G.lzw_tokens(idx.ravel(), 4)
    bad = list(tokens)
    bad[40] = ("code", 16 + 2 + 39)                                         # code 39 of the segment (a clear leads): j = 39 = k
    out["bad_code_beyond_the_table"] = (with_stream(G.pack_tokens(bad, 4)), 0, O.BAD_CODE)
    first = list(tokens)
    first[1] = ("code", 16 + 2)                                              # a table code as the first code after a clear
    out["bad_code_first_after_clear"] = (with_stream(G.pack_tokens(first, 4)), 0, O.BAD_CODE)
    late = G.lzw_tokens(idx.ravel(), 4, segments=[60])
    clears = [i for i, t in enumerate(late) if t[0] == "clear"]
    late[clears[2] + 3] = ("code", 16 + 2 + 2)                               # in the third segment: j = 2 = k
    out["bad_code_in_a_later_segment"] = (with_stream(G.pack_tokens(late, 4)), 0, O.BAD_CODE)
    out["min_code_size_0"] = (with_stream(stream, m=0), 0, O.MIN_CODE_SIZE)
    out["min_code_size_9"] = (with_stream(stream, m=9), 0, O.MIN_CODE_SIZE)
    out["no_palette_at_all"] = (G.gif(61, 47, [G.frame(idx, 61, 47, m=4)]), 0, O.NO_PALETTE)
    good = G.frame(idx, 61, 47, m=4)
    out["unknown_block"] = (G.gif(61, 47, [b"\x99\x01\x02", good], palette=pal), 0, O.CONTAINER)
    out["global_table_cut_short"] = (G.gif(61, 47, [good], palette=pal)[:30], 0, O.CONTAINER)
    out["no_such_frame"] = (G.gif(61, 47, [good, good], palette=pal), 2, O.NO_SUCH_FRAME)
    out["second_frame_damaged"] = (G.gif(61, 47, [good, G.frame(None, 61, 47, m=4, stream=stream[:50])], palette=pal), 1, O.TOO_LITTLE)
    out["rgb_animation_frame3"] = (rgb_animation(), 3, O.NO_SUCH_FRAME)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    data, target = good_files()[name]
    st, bgra, _ = O.decode(data, target)
    assert st == O.OK, (name, st)
    bgra.setflags(write=False)
    return bgra


def golden_files():
    return {n: open(os.path.join(GOLDEN, n), "rb").read() for n in sorted(os.listdir(GOLDEN)) if n.endswith(".gif")}
