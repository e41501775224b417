"""The small frames the tests of the device WebP coder share (BGRA [h, w, 4] uint8, deterministic) and their helpers."""
import io

import numpy as np


def photo(w, h, alpha=False, seed=5):
    """photo-like: smooth gradients, a few edges, a little noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    b = 120 + 70 * np.sin(x / 9.0) + 40 * np.cos(y / 7.0)
    g = 100 + 0.8 * x + 0.5 * y + 30 * np.sin((x + y) / 13.0)
    r = 90 + 60 * np.cos(x / 11.0 - y / 17.0) + 50 * ((x // 19 + y // 23) % 2)
    a = 255 - (40 * (1 + np.sin(x / 5.0 + y / 3.0)) if alpha else 0 * x)
    f = np.stack([b, g, r, a], -1) + rng.normal(0, 1.5, (h, w, 4)) * (1, 1, 1, 1 if alpha else 0)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def noise(w, h, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def one_colour(w, h, bgra=(10, 200, 30, 255)):
    f = np.empty((h, w, 4), np.uint8)
    f[:] = bgra
    return f


def two_colours(w, h):
    f = one_colour(w, h, (1, 2, 3, 255))
    f[((np.arange(h)[:, None] * 7 + np.arange(w)[None, :] * 3) % 5) < 2] = (200, 100, 50, 128)
    return f


def flat(w, h):
    """large areas of few colours with sharp edges (a chart, a logo)"""
    f = one_colour(w, h, (250, 250, 250, 255))
    f[h // 5:h // 2, w // 6:w // 2] = (30, 60, 200, 255)
    f[h // 3:, 2 * w // 3:] = (40, 160, 40, 255)
    f[::9, :] = (0, 0, 0, 255)
    return f


def few_colours(w, h, n=11, seed=3):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    pal[:, 3] = 255
    y, x = np.mgrid[0:h, 0:w]
    return pal[((x // 3) * 5 + (y // 2) * 3 + rng.integers(0, 2, (h, w))) % n]


def repeated_rows(w, h, seed=9):
    """every row equals the first: a noise row, so the residuals of row 0 are literals and the rest is one long run"""
    return np.repeat(noise(w, 1, seed), h, 0)


def row_ramp(w, h, seed=11):
    """every row is the row above plus a small per-column step: under the T predictor the residuals repeat row by row
    without being constant, so matches lie one row up"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (1, w, 4)).astype(np.int64)
    step = rng.integers(0, 4, (1, w, 4)).astype(np.int64)
    f = (base + np.arange(h)[:, None, None] * step) % 256
    f[..., 3] = 255
    return f.astype(np.uint8)


def noise_with_a_run(w, h, seed=15):
    """noise whose first row (always predicted from the left) holds five equal pixels: a band with a match, and still
    smaller as plain 32-bit literals than under codes of its own"""
    f = noise(w, h, seed)
    f[0, 20:25] = f[0, 20]
    return f


def garbage_alpha(bgra, seed=13):
    """the frame with alpha bytes that mean nothing (a BGRX frame)"""
    f = bgra.copy()
    f[..., 3] = np.random.default_rng(seed).integers(0, 256, f.shape[:2], dtype=np.uint8)
    return f


# name -> (frame, alpha_meaningful): the shapes the emulation and the device are both checked on
def cases():
    return {
        "1x1": (noise(1, 1), True),
        "1x37": (noise(1, 37), True),
        "37x1": (noise(37, 1), True),
        "5x3": (photo(5, 3), True),
        "odd_width": (photo(37, 23), True),                           # no multiple of the 16-pixel tile
        "two_bands": (photo(40, 70, alpha=True), True),
        "three_segments": (garbage_alpha(photo(129, 64)), False),     # one band of 8256 pixels: segments of 4096, 4096 and 64
        "one_colour": (one_colour(40, 150), True),                    # three bands; the first holds the first pixel's residual
        "black": (one_colour(33, 20, (0, 0, 0, 255)), True),          # every residual is zero
        "two_colours": (two_colours(37, 29), True),
        "repeated_rows": (repeated_rows(130, 70), True),
        "row_ramp": (row_ramp(61, 40), True),
        "row_ramp_tall": (row_ramp(61, 140), True),                   # the bands behind the first hold matches only
        "noise_with_a_run": (noise_with_a_run(70, 66), True),         # its first band falls back to literals under flat codes
        "noise": (noise(70, 66), True),
        "photo": (photo(96, 80), True),
        "photo_bgrx": (garbage_alpha(photo(50, 45)), False),
        "transparent_rgb": (np.concatenate([noise(24, 9)[..., :3], np.zeros((9, 24, 1), np.uint8)], -1), True),   # RGB under alpha 0 survives
    }


def rgba_of(bgra, alpha_meaningful=True):
    out = bgra[..., [2, 1, 0, 3]].copy()
    if not alpha_meaningful:
        out[..., 3] = 255
    return out


def pillow_decode(data):
    """(RGBA [h, w, 4], the mode Pillow opened the file in) through libwebp; fails where Pillow lacks WebP"""
    from PIL import Image, features
    assert features.check("webp"), "Pillow without WebP support: the decoder these tests are pinned to is missing"
    im = Image.open(io.BytesIO(data))
    assert im.format == "WEBP"
    im.load()
    return np.asarray(im.convert("RGBA")), im.mode
