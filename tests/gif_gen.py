"""A seeded writer of legal GIF files whose LZW streams Pillow's encoder never writes (tests/test_gif_gen.py checks it
against Pillow's decoder byte for byte): clear codes wherever a test wants them, none at all (a deferred clear: the table
fills and the codes stay 12 bits wide), two in a row, no leading clear, no end code, bytes behind the end code, minimum code
sizes 1..8 whatever the palette's size.  The container writer takes every field a test may want to set.

The code widths are the GIF89a rule (appendix F, "variable-length-code LZW"): the k-th code after a clear code is read when
the table holds size(k) = min(clear + 2 + max(k - 1, 0), 4096) entries, and is as wide as the smallest w >= m + 1 with
size(k) < 2^w, 12 at the most; the first code after a clear (k = 0) is m + 1 bits wide, which the rule gives by itself for
every m but 1."""
import struct

import numpy as np


def width_at(m, k):
    size = min((1 << m) + 2 + max(k - 1, 0), 4096)
    w = m + 1
    while k and w < 12 and size >= (1 << w):
        w += 1
    return w


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, w):
        self.acc |= v << self.n
        self.n += w
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def lzw_tokens(indices, m, segments=None, leading_clear=True, end_code=True, double_clear=False, deferred=False, literal_only=False):
    """-> a list of ("code", value) / ("clear",) / ("end",) in stream order.
    segments: the number of codes of each segment in turn (the last value repeats; None: a clear when the table is full,
    the usual encoder); deferred: never a clear, the table stays full; literal_only: no table code is ever used (the table
    fills all the same)."""
    clear = 1 << m
    out = []
    if leading_clear:
        out.append(("clear",))
    table, k, seg = {}, 0, 0
    seg_len = (lambda i: segments[min(i, len(segments) - 1)]) if segments else (lambda i: None)
    i, n = 0, len(indices)
    while i < n:
        cur = int(indices[i])
        assert cur < clear, "an index that no literal of this code size can write"
        i += 1
        while not literal_only and i < n and (cur, int(indices[i])) in table:
            cur = table[(cur, int(indices[i]))]
            i += 1
        out.append(("code", cur))
        nxt = clear + 2 + k
        if i < n and nxt < 4096:
            table[(cur, int(indices[i]))] = nxt
        k += 1
        if i >= n:
            break
        want = seg_len(seg)
        full = clear + 2 + k - 1 >= 4096                    # what the reader's table holds before the next code
        if (want is not None and k >= want) or (want is None and full and not deferred):
            out.append(("clear",))
            if double_clear:
                out.append(("clear",))
            table, k, seg = {}, 0, seg + 1
    if end_code:
        out.append(("end",))
    return out


def pack_tokens(tokens, m):
    clear = 1 << m
    b, k = Bits(), 0
    for t in tokens:
        w = width_at(m, k)
        if t[0] == "clear":
            b.put(clear, w)
            k = 0
        elif t[0] == "end":
            b.put(clear + 1, w)
            k += 1
        else:
            b.put(t[1], w)
            k += 1
    return b.done()


def lzw_stream(indices, m, **kw):
    return pack_tokens(lzw_tokens(indices, m, **kw), m)


def sub_blocks(data, block=255):
    out = bytearray()
    for i in range(0, len(data), block):
        chunk = data[i:i + block]
        out.append(len(chunk))
        out += chunk
    out.append(0)
    return bytes(out)


def interlace_rows(h):
    return [y for start, step in ((0, 8), (4, 8), (2, 4), (1, 2)) for y in range(start, h, step)]


def frame(indices, w, h, left=0, top=0, m=None, palette=None, interlace=False, transparent=None, dispose=None, delay=0, stream=None, block=255, **lzw):
    """One image: a graphic control extension when transparent / dispose / delay ask for one, the descriptor, the local
    palette, the LZW stream.  indices: [h, w] in image order (an interlaced frame's rows are re-ordered here); stream: raw
    LZW bytes to use instead."""
    out = bytearray()
    if transparent is not None or dispose is not None or delay:
        flags = ((dispose or 0) << 2) | (1 if transparent is not None else 0)
        out += b"\x21\xF9\x04" + struct.pack("<BHB", flags, delay, transparent if transparent is not None else 0) + b"\0"
    flags = 0
    if palette is not None:
        bits = max(1, (len(palette) - 1).bit_length())
        assert len(palette) == 1 << bits, "a colour table holds 2^n entries"
        flags |= 0x80 | (bits - 1)
    if interlace:
        flags |= 0x40
    out += b"\x2C" + struct.pack("<HHHHB", left, top, w, h, flags)
    if palette is not None:
        out += bytes(np.asarray(palette, np.uint8).reshape(-1, 3).tobytes())
    if m is None:
        m = 8
    out.append(m)
    if stream is None:
        idx = np.asarray(indices, np.uint8).reshape(h, w) if w * h else np.zeros((0,), np.uint8)
        if interlace and w * h:
            idx = idx[interlace_rows(h)]
        stream = lzw_stream(idx.ravel(), m, **lzw)
    out += sub_blocks(stream, block)
    return bytes(out)


def gif(w, h, frames, palette=None, bg=0, version=b"GIF89a", trailer=True, extensions=b""):
    """frames: the bytes frame() returns, in order; extensions: raw blocks put between the screen descriptor and the first frame."""
    flags = 0
    if palette is not None:
        bits = max(1, (len(palette) - 1).bit_length())
        assert len(palette) == 1 << bits
        flags = 0x80 | 0x70 | (bits - 1)
    out = bytearray(version + struct.pack("<HHBBB", w, h, flags, bg, 0))
    if palette is not None:
        out += np.asarray(palette, np.uint8).reshape(-1, 3).tobytes()
    out += extensions
    for f in frames:
        out += f
    if trailer:
        out += b"\x3B"
    return bytes(out)


def palette_of(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, 256, (n, 3), dtype=np.uint8)


def noise(w, h, colours, seed):
    return np.random.default_rng(seed).integers(0, colours, (h, w), dtype=np.uint8)


def runs(w, h, colours, seed):
    """long and short runs and repeated rows: table codes of every length"""
    rng = np.random.default_rng(seed)
    out = np.zeros(w * h, np.uint8)
    i = 0
    while i < w * h:
        n = int(rng.integers(1, 40))
        out[i:i + n] = rng.integers(0, colours)
        i += n
    return out.reshape(h, w)
