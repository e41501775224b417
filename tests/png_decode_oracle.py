"""A numpy statement of what the PNG decoder must give (test infrastructure): parse, zlib.decompress, un-filter at every
depth, Adam7, then libpng's transforms in the order the reference sets them (c_components/lib/codec_png_wrapper.c:131-212):
expand (palette -> RGB, gray 1/2/4 -> 8 bits by bit replication, tRNS -> alpha with the key compared at the FILE's depth),
filler 0xFF, strip 16 -> 8 by the high byte, gray -> RGB, BGR.  alpha_used (codec_png_wrapper.c:215-246,
libpng_decoder.rs:340-383) is true for colour types with alpha and for palette files, with or without tRNS: gray / RGB
with a tRNS key decode with real alpha bytes in a frame marked bgr_32.

Also the small PNG writer of the tests: any (colour type, depth), a forced filter type per row, Adam7, IDAT split at will."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
LEGAL = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]      # x0, y0, dx, dy


def chunk(tag, data=b"", crc=None):
    body = tag + bytes(data)
    return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) if crc is None else crc)


def filter_bpp(ct, depth):
    return max(1, CHANNELS[ct] * depth // 8)


def row_bytes(w, ct, depth):
    return (w * CHANNELS[ct] * depth + 7) // 8


def pass_shape(w, h, p):
    x0, y0, dx, dy = ADAM7[p]
    return (max(0, (w - x0 + dx - 1) // dx) if w > x0 else 0), (max(0, (h - y0 + dy - 1) // dy) if h > y0 else 0)


def inflated_size(w, h, ct, depth, interlace):
    if not interlace:
        return h * (1 + row_bytes(w, ct, depth))
    n = 0
    for p in range(7):
        pw, ph = pass_shape(w, h, p)
        if pw and ph:
            n += ph * (1 + row_bytes(pw, ct, depth))
    return n


# ---- writer ----------------------------------------------------------------------------------------------------------------------
def pack_rows(samples, depth):
    """samples: (h, w, channels) integers below 2^depth -> (h, row bytes) uint8, as the file stores them"""
    h, w, c = samples.shape
    flat = samples.reshape(h, w * c).astype(np.uint32)
    if depth == 8:
        return flat.astype(np.uint8)
    if depth == 16:
        out = np.empty((h, w * c * 2), np.uint8)
        out[:, 0::2], out[:, 1::2] = flat >> 8, flat & 255
        return out
    per = 8 // depth
    pad = (-flat.shape[1]) % per
    flat = np.pad(flat, ((0, 0), (0, pad)))
    out = np.zeros((h, flat.shape[1] // per), np.uint32)
    for k in range(per):
        out |= flat[:, k::per] << (8 - depth * (k + 1))
    return out.astype(np.uint8)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(rows, bpp, filters):
    """rows: (h, row bytes); filters: an int 0..4 for every row, a sequence (cycled), or a callable(y) -> the filtered stream"""
    h, rb = rows.shape
    out = bytearray()
    prev = np.zeros(rb, np.int32)
    for y in range(h):
        f = filters if isinstance(filters, int) else filters(y) if callable(filters) else filters[y % len(filters)]
        cur = rows[y].astype(np.int32)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        ul = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        if f == 0:
            pred = np.zeros(rb, np.int32)
        elif f == 1:
            pred = left
        elif f == 2:
            pred = prev
        elif f == 3:
            pred = (left + prev) >> 1
        else:
            p = left + prev - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def filtered_stream(samples, ct, depth, filters=0, interlace=False):
    bpp = filter_bpp(ct, depth)
    if not interlace:
        return filter_rows(pack_rows(samples, depth), bpp, filters)
    out = b""
    for x0, y0, dx, dy in ADAM7:
        sub = samples[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            out += filter_rows(pack_rows(sub, depth), bpp, filters)
    return out


def compress(stream, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(stream) + c.flush()


def split_idat(z, split=None):
    """split: None (one chunk), an int (chunks of that many bytes, an empty chunk in front, in the middle and behind)"""
    if split is None:
        return chunk(b"IDAT", z)
    parts = [z[i:i + split] for i in range(0, len(z), split)]
    out = chunk(b"IDAT")
    for i, p in enumerate(parts):
        out += chunk(b"IDAT", p)
        if i == len(parts) // 2:
            out += chunk(b"IDAT")
    return out + chunk(b"IDAT")


def write_png(samples, ct, depth, filters=0, interlace=False, palette=None, trns=None, ancillary=b"", split=None, level=6,
              strategy=zlib.Z_DEFAULT_STRATEGY, z=None):
    """samples: (h, w, channels).  palette: (n, 3) uint8; trns: bytes of the tRNS chunk; ancillary: chunks in front of PLTE; z: a
    zlib stream to use in place of the compressed samples."""
    h, w, _ = samples.shape
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, 1 if interlace else 0)) + ancillary
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", trns)
    if z is None:
        z = compress(filtered_stream(samples, ct, depth, filters, interlace), level, strategy)
    return out + split_idat(z, split) + chunk(b"IEND")


def random_samples(rng, w, h, ct, depth, smooth=False):
    c = CHANNELS[ct]
    if smooth and depth >= 8:
        yy, xx = np.mgrid[0:h, 0:w]
        base = ((xx * 3 + yy * 5)[..., None] + np.arange(c) * 40) % (1 << depth)
        return ((base + rng.integers(0, 4, (h, w, c))) % (1 << depth)).astype(np.uint32)
    return rng.integers(0, 1 << depth, (h, w, c)).astype(np.uint32)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
class Malformed(Exception):
    pass


def parse(data):
    if data[:8] != SIGNATURE:
        raise Malformed("signature")
    pos, chunks = 8, []
    while pos + 12 <= len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if pos + 12 + n > len(data):
            raise Malformed("chunk length")
        if zlib.crc32(tag + body) != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise Malformed("crc " + tag.decode("latin1"))
        chunks.append((tag, body))
        pos += 12 + n
        if tag == b"IEND":
            break
    if not chunks or chunks[0][0] != b"IHDR" or len(chunks[0][1]) != 13:
        raise Malformed("IHDR")
    w, h, depth, ct, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    if (ct, depth) not in LEGAL or comp or filt or inter > 1 or not w or not h:
        raise Malformed("IHDR fields")
    info = dict(width=w, height=h, depth=depth, color_type=ct, interlace=inter, palette=None, trns=None,
                idat=b"".join(b for t, b in chunks if t == b"IDAT"), chunks=chunks)
    for t, b in chunks:
        if t == b"PLTE":
            info["palette"] = np.frombuffer(b, np.uint8).reshape(-1, 3)
        if t == b"tRNS":
            info["trns"] = b
    info["alpha_used"] = ct in (4, 6) or ct == 3
    info["uses_palette"] = ct == 3
    return info


def unfilter_image(buf, w, h, ct, depth):
    """filtered bytes of one (sub-)image -> (h, row bytes) uint8"""
    bpp, rb = filter_bpp(ct, depth), row_bytes(w, ct, depth)
    rows = np.zeros((h, rb), np.uint8)
    prev = np.zeros(rb, np.int64)
    for y in range(h):
        f = buf[y * (rb + 1)]
        x = np.frombuffer(buf, np.uint8, rb, y * (rb + 1) + 1).astype(np.int64)
        if f == 0:
            cur = x
        elif f == 2:
            cur = (x + prev) & 255
        elif f == 1:
            cur = x.copy()
            for k in range(bpp):
                cur[k::bpp] = np.cumsum(x[k::bpp]) & 255
        elif f in (3, 4):
            cur = x.tolist()
            pv = prev.tolist()
            for i in range(rb):
                a = cur[i - bpp] if i >= bpp else 0
                c = pv[i - bpp] if i >= bpp else 0
                cur[i] = (cur[i] + ((a + pv[i]) >> 1 if f == 3 else paeth(a, pv[i], c))) & 255
            cur = np.array(cur, np.int64)
        else:
            raise Malformed("filter type %d" % f)
        rows[y] = cur
        prev = cur
    return rows


def unpack_rows(rows, w, ct, depth):
    """(h, row bytes) -> (h, w, channels) samples at the file's depth"""
    h, c = rows.shape[0], CHANNELS[ct]
    if depth == 8:
        s = rows.astype(np.uint32)
    elif depth == 16:
        s = rows[:, 0::2].astype(np.uint32) << 8 | rows[:, 1::2]
    else:
        per = 8 // depth
        s = np.zeros((h, rows.shape[1] * per), np.uint32)
        for k in range(per):
            s[:, k::per] = (rows >> (8 - depth * (k + 1))) & ((1 << depth) - 1)
    return s[:, :w * c].reshape(h, w, c)


def samples_of(info):
    w, h, ct, depth = info["width"], info["height"], info["color_type"], info["depth"]
    want = inflated_size(w, h, ct, depth, info["interlace"])
    raw = zlib.decompress(info["idat"])
    if len(raw) < want:
        raise Malformed("not enough image data")
    if not info["interlace"]:
        return unpack_rows(unfilter_image(raw, w, h, ct, depth), w, ct, depth)
    out = np.zeros((h, w, CHANNELS[ct]), np.uint32)
    off = 0
    for p, (x0, y0, dx, dy) in enumerate(ADAM7):
        pw, ph = pass_shape(w, h, p)
        if not pw or not ph:
            continue
        n = ph * (1 + row_bytes(pw, ct, depth))
        out[y0::dy, x0::dx] = unpack_rows(unfilter_image(raw[off:off + n], pw, ph, ct, depth), pw, ct, depth)
        off += n
    return out


def to8(v, depth):
    return v >> 8 if depth == 16 else v * {8: 1, 4: 17, 2: 85, 1: 255}[depth]


def palette_table(info):
    """256 BGRA entries: PLTE with tRNS applied, 255 beyond the chunk's length; beyond PLTE opaque black (libpng's zero-filled palette)"""
    t = np.zeros((256, 4), np.uint8)
    t[:, 3] = 255
    if info["palette"] is not None:
        n = len(info["palette"])
        t[:n, 0], t[:n, 1], t[:n, 2] = info["palette"][:, 2], info["palette"][:, 1], info["palette"][:, 0]
    if info["trns"] is not None and info["color_type"] == 3:
        a = np.frombuffer(info["trns"], np.uint8)[:256]
        t[:len(a), 3] = a
    return t


def decode(data):
    """-> (BGRA (h, w, 4) uint8, info)"""
    info = parse(data)
    s = samples_of(info)
    ct, depth, trns = info["color_type"], info["depth"], info["trns"]
    h, w = s.shape[:2]
    out = np.zeros((h, w, 4), np.uint8)
    if ct == 3:
        if info["palette"] is None:
            raise Malformed("no PLTE")
        out[:] = palette_table(info)[s[..., 0]]
    elif ct in (0, 4):
        g = to8(s[..., 0], depth)
        out[..., 0] = out[..., 1] = out[..., 2] = g
        if ct == 4:
            out[..., 3] = to8(s[..., 1], depth)
        else:
            out[..., 3] = 255
            if trns is not None:
                key = struct.unpack(">H", trns[:2])[0] & ((1 << depth) - 1)               # (png_do_expand keeps the key's low bits)
                out[..., 3][s[..., 0] == key] = 0                          # at the file's depth, before any scaling or stripping
    else:
        out[..., 2], out[..., 1], out[..., 0] = to8(s[..., 0], depth), to8(s[..., 1], depth), to8(s[..., 2], depth)
        if ct == 6:
            out[..., 3] = to8(s[..., 3], depth)
        else:
            out[..., 3] = 255
            if trns is not None:
                key = np.array(struct.unpack(">HHH", trns[:6]), np.uint32) & ((1 << depth) - 1)
                out[..., 3][np.all(s == key, axis=2)] = 0
    return out, info
