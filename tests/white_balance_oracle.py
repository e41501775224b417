"""CPU restatement of flow/nodes/white_balance.rs (:13-93) and graphics/histogram.rs, for the tests of
csrc/white_balance.hip.  Test infrastructure only: the library has no CPU path.

Kept as the reference's release build computes it: the threshold is an f32 widened to f64 (None is the f32 literal 0.006);
`high` is searched with the LOW threshold (:33, sic); `(high - low)` is a usize subtraction that wraps when high < low; the
map is `(v.saturating_sub(low) as f64 * scale).round().min(255).max(0) as u8` with round half away from zero and a NaN
product (0 * inf) taken to 255 by `min`.
"""
import math

import numpy as np

DEFAULT_THRESHOLD = float(np.float32(0.006))      # :77 `unwrap_or(0.006)` on an Option<f32>: 0.006000000052154064


def histograms(img):
    """populate_histogram_from_window (histogram.rs): uint8 [h][w][4] BGRA -> uint64 [3][256] in R, G, B order."""
    px = img.reshape(-1, 4)
    return np.stack([np.bincount(px[:, c], minlength=256) for c in (2, 1, 0)]).astype(np.uint64)


def area_threshold(hist, total, low_t, high_t):
    """:13-40 -> (low, high)."""
    low, high = 0, len(hist) - 1
    area = 0
    for ix, v in enumerate(hist):
        area += int(v)
        if float(area) / float(total) > low_t:
            low = ix
            break
    area = 0
    for ix in range(len(hist) - 1, -1, -1):
        area += int(hist[ix])
        if float(area) / float(total) > low_t:          # sic: low_t (high_t is passed but unused)
            high = ix
            break
    return low, high


def byte_mapping(low, high):
    """create_byte_mapping (:43-50)."""
    d = (high - low) % (1 << 64)                       # usize subtraction, wrapping in a release build
    scale = math.inf if d == 0 else 255.0 / float(d)
    out = np.zeros(256, np.uint8)
    for v in range(256):
        p = float(max(v - low, 0)) * scale            # 0 * inf is NaN
        if p != p or p >= 255.0:
            r = 255.0                                 # NaN.round().min(255.0) = 255; inf and large values clamp
        else:
            r = math.floor(p)                         # f64::round, half away from zero (p >= 0; p - floor(p) is exact)
            r = min(r + 1.0 if p - r >= 0.5 else r, 255.0)
        out[v] = int(r)
    return out


def maps(hist, total, threshold=None):
    t = DEFAULT_THRESHOLD if threshold is None else float(np.float32(threshold))
    return [byte_mapping(*area_threshold(hist[c], total, t, t)) for c in range(3)]


def white_balance(img, threshold=None):
    """WhiteBalanceSrgbMutDef::mutate (:106-122) in place: R, G and B through their maps, alpha untouched."""
    h, w, _ = img.shape
    mr, mg, mb = maps(histograms(img), w * h, threshold)
    img[..., 2] = mr[img[..., 2]]
    img[..., 1] = mg[img[..., 1]]
    img[..., 0] = mb[img[..., 0]]
    return img
