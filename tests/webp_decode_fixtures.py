"""The files the WebP decoder's tests share: good files (Pillow's lossless encoder at settings chosen for the features they
give, this project's own coder through its emulation, and tests/vp8l_gen.py's legal streams libwebp never writes) with the
yardstick's pixels, and damaged files with the status word each must get.  The yardstick is libwebp through Pillow;
tests/vp8l_reader.py supplies the alpha bytes of files Pillow opens as RGB, and the structure each fixture is there for.
Everything is made once per process, seeded."""
import io
import struct

import numpy as np

from tests import vp8l_gen as G
from tests import webp_frames as F
from tests.vp8l_reader import read_vp8l

OK, TRUNCATED, CODE_LENGTHS, BAD_CODE, DISTANCE, COPY_END, CACHE_SYMBOL, TRANSFORM, TOO_LITTLE, CONTAINER = range(10)
_CACHE = {}


def pillow_file(rgba, **settings):
    from PIL import Image, features
    assert features.check("webp"), "Pillow without WebP support"
    buf = io.BytesIO()
    a = np.ascontiguousarray(rgba, np.uint8)
    Image.fromarray(a, "RGBA" if a.shape[2] == 4 else "RGB").save(buf, "WEBP", lossless=True, **settings)
    return buf.getvalue()


def smooth_photo(w, h, seed=21):
    """a smooth photo-like RGB frame with noise of sigma about 3"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [128 + 90 * np.sin(x / (17.0 + 5 * k) + k) * np.cos(y / (23.0 - 4 * k)) + rng.normal(0, 3, (h, w)) for k in range(3)]
    return np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)


def indexed(w, h, colours, seed):
    rng = np.random.default_rng(seed)
    palette = rng.integers(0, 256, (colours, 3), dtype=np.uint8)
    f = palette[rng.integers(0, colours, (h, w))]
    f[20:40] = f[0:20]                                           # rows that come again: matches
    f[50:, 10:] = f[45:45 + h - 50, :w - 10]
    return f


def graphic(w, h):
    """two colours in a pattern that repeats every 54 rows: long matches far back"""
    f = np.zeros((h, w, 3), np.uint8)
    rng = np.random.default_rng(8)
    block = rng.integers(0, 2, (54, w)).astype(bool)
    for y in range(h):
        f[y, block[y % 54]] = (250, 20, 40)
    return f


def payload_of(data):
    """the VP8L chunk's bytes of a file"""
    at = 12
    while at + 8 <= len(data):
        tag, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        if tag == b"VP8L":
            return data[at + 8:at + 8 + size]
        at += 8 + size + (size & 1)
    raise AssertionError("no VP8L chunk")


def good_files():
    """name -> file bytes"""
    if "good" in _CACHE:
        return _CACHE["good"]
    rng = np.random.default_rng(33)
    photo = smooth_photo(150, 130)
    files = {
        "photo_q70_m4": pillow_file(photo, quality=70, method=4),
        "photo_q100_m6": pillow_file(photo, quality=100, method=6),
        "photo_q0_m0": pillow_file(photo, quality=0, method=0),
        "photo_cache": pillow_file(F.rgba_of(F.photo(45, 38)), quality=70, method=6, exact=True),
        "rgba_exact": pillow_file(rng.integers(0, 256, (23, 31, 4), dtype=np.uint8), quality=70, method=4, exact=True),
        "graphic": pillow_file(graphic(90, 70), quality=70, method=4),
        "1x1": pillow_file(np.full((1, 1, 3), 77, np.uint8), quality=70, method=4),
        "1xN": pillow_file(smooth_photo(1, 67, 2), quality=70, method=4),
        "Nx1": pillow_file(smooth_photo(67, 1, 3), quality=70, method=4),
        "w17": pillow_file(smooth_photo(17, 40, 4), quality=70, method=4),
    }
    for colours in (2, 4, 16, 200):
        files["indexed_%d" % colours] = pillow_file(indexed(77, 61, colours, colours), quality=70, method=4)
    from tests import webp_emulation as E
    for name, (frame, alpha) in F.cases().items():
        if frame.shape[0] * frame.shape[1] <= 3000:
            files["own_" + name] = E.encode(frame, alpha)[0]
    for name, (data, _counts) in G.legal_files().items():
        files["gen_" + name] = data
    for name, (data, _counts) in G.files_beyond_the_reader().items():
        files["gen_" + name] = data
    _CACHE["good"] = files
    return files


def expected_bgra(name):
    """(BGRA [h, w, 4] as libwebp decodes the good file `name`, the reader's info)"""
    key = ("want", name)
    if key not in _CACHE:
        data = good_files()[name]
        rgba, mode = F.pillow_decode(data)
        if name[4:] in G.files_beyond_the_reader():            # Pillow alone: the reader does not read these
            assert mode == "RGBA", mode
            _CACHE[key] = (np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]), {"alpha_is_used": 1, "transforms": [], "tile_bits": []})
            return _CACHE[key]
        mine, info = read_vp8l(data)
        assert np.array_equal(mine[..., :3], rgba[..., :3]), name
        if mode == "RGBA":
            assert np.array_equal(mine, rgba), name
        else:
            assert mode == "RGB", mode
            rgba = mine                                         # MODE_BGRA keeps the coded alpha bytes: the reader's
        _CACHE[key] = (np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]), info)
    return _CACHE[key]


def pillow_refuses(data):
    from PIL import Image
    try:
        im = Image.open(io.BytesIO(data))
        im.load()
    except Exception:                                            # (OSError, SyntaxError, UnidentifiedImageError ...)
        return True
    return False


def rewrap(payload):
    return G.riff(payload)


def damaged_files(library=False):
    """name -> (file bytes, the status word of the core; library: of the batch call, whose container walk already refuses a
    VP8L chunk shorter than its header).  Every one is refused by Pillow (asserted by the tests that use them)."""
    if library:
        return {n: (d, CONTAINER if s == TOO_LITTLE else s) for n, (d, s) in damaged_files().items()}
    if "bad" in _CACHE:
        return _CACHE["bad"]
    files = {}
    photo = payload_of(good_files()["photo_q70_m4"])
    for cut in (5, 9, 40, len(photo) // 2, len(photo) - 1):
        files["truncated_%d" % cut] = (rewrap(photo[:cut]), TRUNCATED)
    files["too_little"] = (rewrap(photo[:3]), TOO_LITTLE)
    for name, (data, status) in G.damaged_files().items():
        files[name] = (data, status)
    whole = good_files()["photo_q70_m4"]
    files["riff_cut_short"] = (whole[:len(whole) - 7], CONTAINER)
    _CACHE["bad"] = files
    return files
