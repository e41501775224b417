"""Test-side PNG oracle, numpy only: restated from the PNG specification and libpng's default filter choice; libpng itself
is not available here.

  * parse(data): the chunks of a file, every CRC checked;
  * decode(data): IHDR fields, the inflated IDAT stream (zlib.decompress of the concatenated IDAT data, which also checks
    the Adler-32), the filter byte of every row and the un-filtered pixels;
  * filter_image(pixels): libpng's default row choice for 8-bit truecolour -- all five filters, the sum of
    `v < 128 ? v : 256 - v` over the filtered bytes, the smallest sum, a tie to the lowest filter number -- computed from
    pixels; returns the filter types and the filtered stream h * (1 + w * bpp);
  * reference_size(stream, level): what libpng's deflate call writes for a filtered image,
    zlib.compressobj(level, DEFLATED, 15, 8, Z_FILTERED), applied to the ORACLE's stream;
  * write_png(pixels): a file assembled from the above (Pillow opens it: tests/test_png_oracle.py)."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
GAMA = 45455
CHRM = (31270, 32900, 64000, 33000, 30000, 60000, 15000, 6000)


def parse(data):
    """[(type, payload)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND."""
    data = bytes(data)
    assert data[:8] == SIGNATURE, "signature"
    at, chunks = 8, []
    while at < len(data):
        assert at + 12 <= len(data), "truncated chunk"
        n, = struct.unpack(">I", data[at:at + 4])
        kind = data[at + 4:at + 8]
        assert at + 12 + n <= len(data), "chunk runs past the file"
        payload = data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + payload), f"CRC of {kind!r}"
        chunks.append((kind, payload))
        at += 12 + n
        if kind == b"IEND":
            break
    assert at == len(data), "bytes behind IEND"
    assert chunks and chunks[0][0] == b"IHDR" and chunks[-1][0] == b"IEND"
    return chunks


def _paeth(a, b, c):
    p = a.astype(np.int32) + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _candidates(row, prev, bpp):
    """The five filtered versions of a row (int32 arrays holding bytes); prev: the unfiltered row above."""
    x = row.astype(np.int32)
    b = prev.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if x.size > bpp else np.zeros_like(x)
    c = np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]]) if x.size > bpp else np.zeros_like(x)
    if x.size <= bpp:
        a, c = np.zeros_like(x), np.zeros_like(x)
    return [x & 255, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - _paeth(a, b, c)) & 255]


def filter_image(pixels):
    """pixels: uint8 [h, w, bpp].  Returns (filter types [h], the filtered stream as bytes)."""
    h, w, bpp = pixels.shape
    rows = pixels.reshape(h, w * bpp)
    prev = np.zeros(w * bpp, np.uint8)
    types, out = [], bytearray()
    for y in range(h):
        cands = _candidates(rows[y], prev, bpp)
        sums = [int(np.where(c < 128, c, 256 - c).sum()) for c in cands]
        f = int(np.argmin(sums))                      # argmin: the first of equal sums, the lowest filter number
        types.append(f)
        out.append(f)
        out += cands[f].astype(np.uint8).tobytes()
        prev = rows[y]
    return np.array(types, np.uint8), bytes(out)


def unfilter(stream, w, h, bpp):
    """The filtered stream back to (filter types [h], pixels [h, w, bpp])."""
    pitch = 1 + w * bpp
    assert len(stream) == h * pitch, f"stream of {len(stream)} bytes for {h} rows of {pitch}"
    s = np.frombuffer(bytes(stream), np.uint8).reshape(h, pitch)
    out = np.zeros((h, w * bpp), np.uint8)
    prev = np.zeros(w * bpp, np.int32)
    for y in range(h):
        f, r = int(s[y, 0]), s[y, 1:].astype(np.int32)
        assert f <= 4, f"filter type {f}"
        if f == 0:
            cur = r
        elif f == 2:
            cur = (r + prev) & 255
        elif f == 1:
            cur = (np.cumsum(r.reshape(w, bpp), axis=0) & 255).reshape(-1)
        else:
            rl, pl, cl = r.tolist(), prev.tolist(), [0] * (w * bpp)
            for i in range(w * bpp):                  # Average and Paeth depend on the byte just rebuilt
                a = cl[i - bpp] if i >= bpp else 0
                b = pl[i]
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    c = pl[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cl[i] = (rl[i] + pred) & 255
            cur = np.array(cl, np.int32)
        out[y] = cur
        prev = cur
    return s[:, 0].copy(), out.reshape(h, w, bpp)


def decode(data, pixels=True):
    """dict(width, height, color_type, bpp, chunks, idat (the concatenated IDAT data), stream, filters, pixels).
    pixels=False leaves the (serial, slow) un-filtering out: a large frame is checked through the stream instead, which
    must equal filter_image(source)'s -- the filters are bijections, so that is the same statement."""
    chunks = parse(data)
    w, h, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ct in (2, 6)
    bpp = 3 if ct == 2 else 4
    kinds = [k for k, _ in chunks]
    first, last = kinds.index(b"IDAT"), len(kinds) - 1 - kinds[::-1].index(b"IDAT")
    assert all(k == b"IDAT" for k in kinds[first:last + 1]), "IDAT chunks must be consecutive"
    idat = b"".join(p for k, p in chunks if k == b"IDAT")
    stream = zlib.decompress(idat)                    # raises on a bad block, a bad code set or a wrong Adler-32
    if pixels:
        filters, pixels = unfilter(stream, w, h, bpp)
    else:
        assert len(stream) == h * (1 + w * bpp)
        filters, pixels = np.frombuffer(stream, np.uint8).reshape(h, 1 + w * bpp)[:, 0].copy(), None
    return dict(width=w, height=h, color_type=ct, bpp=bpp, chunks=chunks, idat=idat, stream=stream, filters=filters, pixels=pixels)


def check_ancillary(chunks):
    """gAMA 45455, sRGB intent 0 and cHRM with the specification's sRGB values, all in front of the first IDAT; no other chunks."""
    kinds = [k for k, _ in chunks]
    assert sorted(set(kinds)) == sorted({b"IHDR", b"gAMA", b"sRGB", b"cHRM", b"IDAT", b"IEND"}), kinds
    first = kinds.index(b"IDAT")
    d = {k: p for k, p in chunks if k != b"IDAT"}
    for k in (b"gAMA", b"sRGB", b"cHRM"):
        assert kinds.count(k) == 1 and kinds.index(k) < first, k
    assert struct.unpack(">I", d[b"gAMA"]) == (GAMA,)
    assert d[b"sRGB"] == b"\x00"
    assert struct.unpack(">8I", d[b"cHRM"]) == CHRM


def stored_only(idat):
    """True when the zlib stream's blocks are all stored blocks (walks the block headers)."""
    at, n = 2, len(idat) - 4
    while at < n:
        final, btype = idat[at] & 1, (idat[at] >> 1) & 3
        if btype != 0:
            return False
        ln, nln = struct.unpack("<HH", idat[at + 1:at + 5])
        assert ln ^ nln == 0xFFFF
        at += 5 + ln
        if final:
            break
    return at == n


def reference_size(stream, level):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_FILTERED)
    return len(co.compress(stream) + co.flush())


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def write_png(pixels, level=6):
    h, w, bpp = pixels.shape
    _, stream = filter_image(pixels)
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_FILTERED)
    z = co.compress(stream) + co.flush()
    return (SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if bpp == 3 else 6, 0, 0, 0)) + _chunk(b"gAMA", struct.pack(">I", GAMA)) +
            _chunk(b"sRGB", b"\x00") + _chunk(b"cHRM", struct.pack(">8I", *CHRM)) + _chunk(b"IDAT", z) + _chunk(b"IEND", b""))


# ---- frames of the acceptance conditions ------------------------------------------------------------------------------------------

def photo_frame(w, h, seed=7):
    """A seeded sum of low-frequency sinusoids per channel, Gaussian noise sigma = 2.5, a dozen offset rectangles.  RGB uint8."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for ch in range(3):
        acc = np.full((h, w), 128.0)
        for _ in range(6):
            fx, fy = rng.uniform(0.5, 6.0, 2) * 2 * np.pi / max(w, h)
            acc += rng.uniform(8, 30) * np.sin(fx * x + fy * y + rng.uniform(0, 2 * np.pi))
        img[..., ch] = acc
    for _ in range(12):
        x0, y0 = int(rng.integers(0, max(1, w - 1))), int(rng.integers(0, max(1, h - 1)))
        x1, y1 = min(w, x0 + int(rng.integers(4, max(5, w // 4)))), min(h, y0 + int(rng.integers(4, max(5, h // 4))))
        img[y0:y1, x0:x1] += rng.uniform(-40, 40, 3)
    img += rng.normal(0, 2.5, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def product_frame(n, seed=11):
    """That photo inside a disc, on white, with transparent rounded corners.  RGBA uint8 [n, n, 4]."""
    rgb = photo_frame(n, n, seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    c = (n - 1) / 2
    disc = (x - c) ** 2 + (y - c) ** 2 <= (0.38 * n) ** 2
    out = np.full((n, n, 4), 255, np.uint8)
    out[..., :3][disc] = rgb[disc]
    r = 0.12 * n
    dx, dy = np.minimum(x, n - 1 - x), np.minimum(y, n - 1 - y)
    corner = (dx < r) & (dy < r) & ((r - dx) ** 2 + (r - dy) ** 2 > r * r)
    out[corner] = 0
    return out
