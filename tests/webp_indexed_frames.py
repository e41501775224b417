"""The frames the tests of the lossless-WebP coder's colour indexing share, on the CPU (tests/test_webp_indexed_coder.py) and
on the device (tests/test_gpu_webp_encode_indexed.py): those of tests/webp_frames.py and the ones that sit on the edges of
the palette's size, of the bundling and of the packed geometry."""
import math

import numpy as np

from tests import webp_frames as F

EDGE_COLOURS = (1, 2, 3, 4, 5, 16, 17, 256)
EDGE_BITS = (3, 3, 2, 2, 1, 1, 0, 0)


def exactly(n, w, h):
    """few_colours' pattern with exactly n colours in use: its own colours are renumbered into n distinct ones, and n pixels
    spread over the frame (a stride that shares no factor with w * h hits no position twice) hold one of each"""
    assert n <= w * h
    step = next(p for p in (3, 5, 7, 11, 13, 17, 19, 23) if math.gcd(p, w * h) == 1)
    base = np.ascontiguousarray(F.few_colours(w, h, n=max(n, 1))).view(np.uint32).reshape(-1)
    index = np.unique(base, return_inverse=True)[1].reshape(-1) % n
    index[(np.arange(n) * step) % (w * h)] = np.arange(n)
    i = np.arange(n)
    colours = np.stack([(i * 37) & 255, i & 255, i >> 8, np.full(n, 255)], -1).astype(np.uint8)
    frame = colours[index].reshape(h, w, 4)
    assert len(np.unique(np.ascontiguousarray(frame).view(np.uint32))) == n
    return frame


def grey_photo(w, h):
    f = F.photo(w, h).copy()
    f[..., 0] = f[..., 1]
    f[..., 2] = f[..., 1]
    return f


def transparent_few(w, h):
    """six colours, three of them with alpha 0 over RGB that differs: what lies under alpha 0 must come back"""
    f = exactly(6, w, h).copy()
    f[f[..., 1] % 2 == 1, 3] = 0
    return f


def own():
    """name -> (frame, alpha_meaningful): the frames beyond webp_frames.cases()"""
    d = {"exactly_%d" % n: (exactly(n, 37, 23), True) for n in EDGE_COLOURS}
    d.update({
        "width_1_two": (exactly(2, 1, 23), True),
        "width_7_two": (exactly(2, 7, 23), True),
        "height_1": (exactly(3, 37, 1), True),
        "colours_257": (exactly(257, 37, 23), True),
        "transparent_few": (transparent_few(37, 23), True),
        "bgrx_few": (F.garbage_alpha(F.few_colours(50, 45, n=5)), False),
        "packed_bands": (F.few_colours(300, 140, n=5), True),         # packs to 150 x 140: 3 bands, 3 segments in each of the first two
        "unbundled_200": (F.few_colours(96, 80, n=200), True),
        "few_96x80": (F.few_colours(96, 80), True),
        "few_70x66_17": (F.few_colours(70, 66, n=17), True),
        "few_33x70_5": (F.few_colours(33, 70, n=5), True),
        "few_37x23": (F.few_colours(37, 23), True),
        "flat_160x90": (F.flat(160, 90), True),
        "grey_photo": (grey_photo(96, 80), True),
    })
    return d


def frames():
    d = dict(F.cases())
    d.update(own())
    return d


def colours_of(frame, alpha_meaningful):
    f = np.ascontiguousarray(frame).copy()
    if not alpha_meaningful:
        f[..., 3] = 255
    return len(np.unique(f.view(np.uint32)))
