"""The test-side PNG oracle (tests/png_oracle.py) pinned on its own: its un-filter inverts its filter, and Pillow opens a
file assembled from the oracle's parts (its filters, zlib, its chunk writer) and returns the same pixels."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import png_oracle as P


def _frames(w, h, bpp):
    rng = np.random.default_rng(w * 131 + h * 7 + bpp)
    y, x = np.mgrid[0:h, 0:w]
    structured = np.stack([(x * 3 + y) & 255, (y * 5) & 255, (x ^ y) & 255, (x + 2 * y) & 255][:bpp], -1).astype(np.uint8)
    flat = np.full((h, w, bpp), 200, np.uint8)
    banded = structured.copy()
    banded[h // 2:] = 17
    return {"random": rng.integers(0, 256, (h, w, bpp), dtype=np.uint8), "structured": structured, "flat": flat, "banded": banded}


@pytest.mark.parametrize("bpp", [3, 4])
@pytest.mark.parametrize("size", [(1, 1), (2, 5), (37, 23), (800, 6), (1, 300), (300, 1), (2, 1), (37, 1), (800, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_unfilter_inverts_filter(size, bpp):
    w, h = size
    for name, px in _frames(w, h, bpp).items():
        types, stream = P.filter_image(px)
        assert len(stream) == h * (1 + w * bpp) and types.max() <= 4
        t2, back = P.unfilter(stream, w, h, bpp)
        assert np.array_equal(t2, types) and np.array_equal(back, px), name


def test_every_filter_type_inverts():
    """filter_image only emits the types its choice takes; force each of the five through the un-filter."""
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (9, 14, 4), dtype=np.uint8)
    rows = px.reshape(9, -1)
    for f in range(5):
        out, prev = bytearray(), np.zeros(rows.shape[1], np.uint8)
        for y in range(9):
            out.append(f)
            out += P._candidates(rows[y], prev, 4)[f].astype(np.uint8).tobytes()
            prev = rows[y]
        types, back = P.unfilter(bytes(out), 14, 9, 4)
        assert (types == f).all() and np.array_equal(back, px), f


def test_filter_choice_prefers_the_lowest_number_on_a_tie_and_up_on_flat_rows():
    flat = np.full((4, 10, 3), 90, np.uint8)
    types, _ = P.filter_image(flat)
    assert types.tolist() == [1, 2, 2, 2]                 # Sub on the first row (Paeth ties with it), Up below (all zero; Paeth ties)
    zero = np.zeros((3, 5, 4), np.uint8)
    assert P.filter_image(zero)[0].tolist() == [0, 0, 0]  # every filter gives zeros: None wins


@pytest.mark.parametrize("bpp", [3, 4])
def test_pillow_opens_the_oracles_file(bpp):
    px = P.product_frame(120) if bpp == 4 else P.photo_frame(150, 90)
    data = P.write_png(px)
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.mode == ("RGBA" if bpp == 4 else "RGB")
    assert np.array_equal(np.asarray(im), px)
    d = P.decode(data)
    P.check_ancillary(d["chunks"])
    assert np.array_equal(d["pixels"], px) and np.array_equal(d["filters"], P.filter_image(px)[0])
    # Pillow's own file (libpng-compatible writer, its own filter choice) goes through the parser and un-filter too
    b = io.BytesIO()
    Image.fromarray(px).save(b, "PNG")
    chunks = P.parse(b.getvalue())
    import zlib
    stream = zlib.decompress(b"".join(p for k, p in chunks if k == b"IDAT"))
    assert np.array_equal(P.unfilter(stream, px.shape[1], px.shape[0], bpp)[1], px)


def test_a_damaged_crc_is_caught():
    data = bytearray(P.write_png(P.photo_frame(20, 10)))
    data[40] ^= 1
    with pytest.raises(AssertionError):
        P.parse(bytes(data))
