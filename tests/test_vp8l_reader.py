"""tests/vp8l_reader.py pinned to libwebp: files Pillow writes (lossless, methods 0, 4 and 6; photo-like, flat and
few-colour frames, with and without alpha, so that the colour cache, colour indexing, cross-colour and the 2-D distance
codes are all read) decode to exactly what Pillow decodes from them."""
import io

import numpy as np
import pytest

from tests import webp_frames as F
from tests.vp8l_reader import read_vp8l

FRAMES = {"photo": lambda: F.photo(45, 38), "photo_alpha": lambda: F.photo(45, 38, alpha=True), "flat": lambda: F.flat(50, 41),
          "few_colours": lambda: F.few_colours(43, 37), "two_colours": lambda: F.two_colours(37, 29), "noise": lambda: F.noise(19, 21)}


def _pillow_file(bgra, method):
    from PIL import Image, features
    assert features.check("webp"), "Pillow without WebP support"
    buf = io.BytesIO()
    Image.fromarray(F.rgba_of(bgra), "RGBA").save(buf, "WEBP", lossless=True, quality=70, method=method, exact=True)
    return buf.getvalue()


_DECODED = {}


def decoded(name, method):
    """(Pillow's file, the reader's pixels and structure), computed once"""
    if (name, method) not in _DECODED:
        data = _pillow_file(FRAMES[name](), method)
        _DECODED[(name, method)] = (data,) + read_vp8l(data)
    return _DECODED[(name, method)]


@pytest.mark.parametrize("method", [0, 4, 6])
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_reader_decodes_what_pillow_writes(name, method):
    data, got, info = decoded(name, method)
    want, _ = F.pillow_decode(data)
    assert got.shape == want.shape and np.array_equal(got, want), (name, method, info["transforms"])
    assert (info["width"], info["height"]) == (want.shape[1], want.shape[0])
    assert (info["bits"] + 7) // 8 == info["payload_bytes"]                # the reader consumed the whole stream, no more


def test_the_files_above_exercise_every_part_of_the_reader():
    """libwebp used all four transforms, a colour cache and backward references beyond the previous pixel on them"""
    infos = [decoded(name, method)[2] for name in FRAMES for method in (0, 4, 6)]
    assert set().union(*(i["transforms"] for i in infos)) == {"predictor", "cross_color", "subtract_green", "color_indexing"}
    assert any(i["color_cache_bits"] > 0 for i in infos)
    assert any(d > 1 for i in infos for _, _, d in i["matches"])


def test_reader_refuses_what_is_no_stream():
    data = bytearray(_pillow_file(FRAMES["photo"](), 0))
    with pytest.raises(ValueError):
        read_vp8l(bytes(data[:len(data) // 2]))
    data[20] = 0x2E
    with pytest.raises(ValueError):
        read_vp8l(bytes(data))
