"""A small VP8L (lossless WebP) reader in plain Python, written for the tests of the device WebP coder from the format
specification: it gives the pixels AND the structure of a file -- the transforms in order, their tile bits, the number of
prefix-code groups, whether a colour cache is present, and the bits the stream consumed.  It reads everything libwebp's
lossless encoder writes (predictor, cross-colour, subtract-green and colour-indexing transforms, the colour cache, meta
prefix codes, 2-D distance codes): tests/test_vp8l_reader.py pins it to libwebp on files Pillow writes, before any test
relies on what it says about this project's own files.  Slow (a pixel at a time): for small frames."""
import struct

import numpy as np

TRANSFORM_NAMES = {0: "predictor", 1: "cross_color", 2: "subtract_green", 3: "color_indexing"}
CODE_LENGTH_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
# distance codes 1..120: (dx, dy), the pixel dx to the left and dy rows up (specification, "LZ77 backward reference")
DISTANCE_MAP = (
    (0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3),
    (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4),
    (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2),
    (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2),
    (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1),
    (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5),
    (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7),
    (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7))


class FormatError(ValueError):
    pass


class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def read(self, n):
        v = 0
        for i in range(n):
            p = self.pos + i
            if (p >> 3) >= len(self.data):
                raise FormatError("the stream ends early")
            v |= ((self.data[p >> 3] >> (p & 7)) & 1) << i
        self.pos += n
        return v


class _Code:
    """A canonical prefix code from its lengths; a code with one used symbol reads no bits."""

    def __init__(self, lengths):
        used = [s for s, l in enumerate(lengths) if l]
        self.single = used[0] if len(used) == 1 else None
        self.table = {}
        if not used:
            raise FormatError("a code without symbols")
        if self.single is not None:
            return
        kraft = sum(1 << (15 - l) for l in lengths if l)
        if kraft != 1 << 15:
            raise FormatError("an incomplete or over-subscribed code (Kraft sum %d / 32768)" % kraft)
        code = 0
        for n in range(1, 16):
            for s, l in enumerate(lengths):
                if l == n:
                    self.table[(n, code)] = s
                    code += 1
            code <<= 1

    def read(self, br):
        if self.single is not None:
            return self.single
        code = 0
        for n in range(1, 16):
            code = (code << 1) | br.read(1)
            s = self.table.get((n, code))
            if s is not None:
                return s
        raise FormatError("bits that are no code")


def _read_code(br, alphabet):
    if br.read(1):                                           # simple: one or two symbols
        count = br.read(1) + 1
        lengths = [0] * alphabet
        first = br.read(8 if br.read(1) else 1)
        lengths[first] = 1
        if count == 2:
            lengths[br.read(8)] = 1
        return _Code(lengths), "simple%d" % count
    n = 4 + br.read(4)
    cl = [0] * 19
    for i in range(n):
        cl[CODE_LENGTH_ORDER[i]] = br.read(3)
    cl_code = _Code(cl)
    max_symbol = alphabet
    if br.read(1):
        nbits = 2 + 2 * br.read(3)
        max_symbol = 2 + br.read(nbits)
        if max_symbol > alphabet:
            raise FormatError("max_symbol beyond the alphabet")
    lengths, prev, s = [0] * alphabet, 8, 0
    while s < alphabet and max_symbol:
        max_symbol -= 1
        c = cl_code.read(br)
        if c < 16:
            lengths[s] = c
            s += 1
            if c:
                prev = c
        else:
            rep = (3 + br.read(2)) if c == 16 else (3 + br.read(3)) if c == 17 else (11 + br.read(7))
            if s + rep > alphabet:
                raise FormatError("a run of code lengths beyond the alphabet")
            if c == 16:
                lengths[s:s + rep] = [prev] * rep
            s += rep
    return _Code(lengths), "normal"


def _prefix_value(br, sym):
    if sym < 4:
        return sym + 1
    extra = (sym - 2) >> 1
    return ((2 + (sym & 1)) << extra) + br.read(extra) + 1


def _image_stream(br, xsize, ysize, main, info):
    """ARGB values of an xsize * ysize entropy-coded image (the main image when `main`, else a sub-image)."""
    cache_bits = br.read(4) if br.read(1) else 0
    if cache_bits and not 1 <= cache_bits <= 11:
        raise FormatError("colour cache bits %d" % cache_bits)
    cache = [0] * (1 << cache_bits) if cache_bits else None
    prefix_bits, entropy, n_groups, ent_x = 0, None, 1, 0
    if main:
        info["color_cache_bits"] = cache_bits
        if br.read(1):
            prefix_bits = br.read(3) + 2
            ent_x = (xsize + (1 << prefix_bits) - 1) >> prefix_bits
            ent_y = (ysize + (1 << prefix_bits) - 1) >> prefix_bits
            entropy = [(v >> 8) & 0xFFFF for v in _image_stream(br, ent_x, ent_y, False, info)]
            n_groups = max(entropy) + 1
            info["entropy_image"] = np.array(entropy, np.uint32).reshape(ent_y, ent_x)
        info["prefix_bits"], info["groups"] = prefix_bits, n_groups
        info["head_bits"] = br.pos
    groups, kinds = [], []
    for _ in range(n_groups):
        codes = []
        for size in (256 + 24 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40):
            code, kind = _read_code(br, size)
            codes.append(code)
            kinds.append(kind)
        groups.append(codes)
    if main:
        info["code_kinds"] = kinds
        info["pixel_bits_start"] = br.pos
    out, n, i = [0] * (xsize * ysize), xsize * ysize, 0
    matches = []

    def insert(v):
        if cache is not None:
            cache[((0x1E35A7BD * v) & 0xFFFFFFFF) >> (32 - cache_bits)] = v
    while i < n:
        g = groups[entropy[((i // xsize) >> prefix_bits) * ent_x + ((i % xsize) >> prefix_bits)]] if entropy is not None else groups[0]
        s = g[0].read(br)
        if s < 256:
            red = g[1].read(br)
            blue = g[2].read(br)
            alpha = g[3].read(br)
            v = (alpha << 24) | (red << 16) | (s << 8) | blue
            out[i] = v
            insert(v)
            i += 1
        elif s < 280:
            length = _prefix_value(br, s - 256)
            dcode = _prefix_value(br, g[4].read(br))
            if dcode > 120:
                dist = dcode - 120
            else:
                dx, dy = DISTANCE_MAP[dcode - 1]
                dist = max(1, dx + dy * xsize)
            if dist > i or i + length > n:
                raise FormatError("a match outside the image (distance %d, length %d at %d of %d)" % (dist, length, i, n))
            matches.append((i, length, dist))
            for _k in range(length):
                out[i] = out[i - dist]
                insert(out[i])
                i += 1
        else:
            if cache is None or s - 280 >= len(cache):
                raise FormatError("a colour cache symbol without a cache")
            out[i] = cache[s - 280]
            insert(out[i])
            i += 1
    if main:
        info["matches"] = matches
    return out


def _add(a, b):
    return (((a & 0xFF00FF00) + (b & 0xFF00FF00)) & 0xFF00FF00) | (((a & 0x00FF00FF) + (b & 0x00FF00FF)) & 0x00FF00FF)


def _avg2(a, b):
    return (((a ^ b) & 0xFEFEFEFE) >> 1) + (a & b)


def _channels(v):
    return (v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255


def _clamp(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _predict(mode, L, T, TL, TR):
    if mode == 0:
        return 0xFF000000
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg2(_avg2(L, TR), T)
    if mode == 6:
        return _avg2(L, TL)
    if mode == 7:
        return _avg2(L, T)
    if mode == 8:
        return _avg2(TL, T)
    if mode == 9:
        return _avg2(T, TR)
    if mode == 10:
        return _avg2(_avg2(L, TL), _avg2(T, TR))
    l, t, tl = _channels(L), _channels(T), _channels(TL)
    if mode == 11:
        dl = sum(abs(t[k] - tl[k]) for k in range(4))        # |L + T - TL - L|
        dt = sum(abs(l[k] - tl[k]) for k in range(4))
        return L if dl < dt else T
    if mode == 12:
        c = [_clamp(l[k] + t[k] - tl[k]) for k in range(4)]
    elif mode == 13:
        a = _channels(_avg2(L, T))
        c = [_clamp(a[k] + int((a[k] - tl[k]) / 2)) for k in range(4)]      # truncation toward zero
    else:
        raise FormatError("predictor mode %d" % mode)
    return (c[0] << 24) | (c[1] << 16) | (c[2] << 8) | c[3]


def _inverse_predictor(px, w, h, bits, modes):
    tiles_x = (w + (1 << bits) - 1) >> bits
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                pred = 0xFF000000 if x == 0 else px[i - 1]
            elif x == 0:
                pred = px[i - w]
            else:
                mode = (modes[(y >> bits) * tiles_x + (x >> bits)] >> 8) & 0xFF
                pred = _predict(mode, px[i - 1], px[i - w], px[i - w - 1], px[i - w + 1])   # TR of the last column: the row's first
            px[i] = _add(px[i], pred)


def _s8(v):
    return v - 256 if v >= 128 else v


def _inverse_cross_color(px, w, h, bits, data):
    tiles_x = (w + (1 << bits) - 1) >> bits
    for y in range(h):
        for x in range(w):
            e = data[(y >> bits) * tiles_x + (x >> bits)]
            r2b, g2b, g2r = (e >> 16) & 255, (e >> 8) & 255, e & 255
            v = px[y * w + x]
            green = (v >> 8) & 255
            red = ((v >> 16) + ((_s8(g2r) * _s8(green)) >> 5)) & 255
            blue = (v + ((_s8(g2b) * _s8(green)) >> 5) + ((_s8(r2b) * _s8(red)) >> 5)) & 255
            px[y * w + x] = (v & 0xFF00FF00) | (red << 16) | blue


def read_vp8l(data):
    """(rgba [h, w, 4] uint8, info) of a .webp file that holds a VP8L chunk.  info: width, height, alpha_is_used,
    transforms (names in file order), tile_bits (per transform, None where it has none), color_cache_bits, prefix_bits,
    groups, entropy_image, code_kinds, matches [(position, length, distance)], bits (consumed by the stream), payload_bytes,
    riff_size, head_bits / pixel_bits_start (bit positions in the payload: the groups' codes, the main image's pixels)."""
    data = bytes(data)
    if data[:4] != b"RIFF" or data[8:12] != b"WEBP":
        raise FormatError("no RIFF / WEBP container")
    riff_size = struct.unpack_from("<I", data, 4)[0]
    at, payload = 12, None
    while at + 8 <= len(data):
        tag, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        if tag == b"VP8L":
            payload = data[at + 8:at + 8 + size]
            if len(payload) != size:
                raise FormatError("the VP8L chunk is cut short")
            break
        at += 8 + size + (size & 1)
    if payload is None:
        raise FormatError("no VP8L chunk")
    br = _Bits(payload)
    if br.read(8) != 0x2F:
        raise FormatError("no VP8L signature")
    w, h = br.read(14) + 1, br.read(14) + 1
    info = {"width": w, "height": h, "alpha_is_used": br.read(1), "transforms": [], "tile_bits": [], "payload_bytes": len(payload), "riff_size": riff_size,
            "file_bytes": len(data)}
    if br.read(3) != 0:
        raise FormatError("version")
    transforms, xsize, seen = [], w, set()
    while br.read(1):
        kind = br.read(2)
        if kind in seen:
            raise FormatError("a transform twice")
        seen.add(kind)
        info["transforms"].append(TRANSFORM_NAMES[kind])
        if kind in (0, 1):
            bits = br.read(3) + 2
            sub = _image_stream(br, (xsize + (1 << bits) - 1) >> bits, (h + (1 << bits) - 1) >> bits, False, info)
            transforms.append((kind, bits, sub, xsize))
            info["tile_bits"].append(bits)
        elif kind == 2:
            transforms.append((kind, 0, None, xsize))
            info["tile_bits"].append(None)
        else:
            size = br.read(8) + 1
            table = _image_stream(br, size, 1, False, info)
            for i in range(1, size):
                table[i] = _add(table[i], table[i - 1])
            bits = 3 if size <= 2 else 2 if size <= 4 else 1 if size <= 16 else 0
            transforms.append((kind, bits, table, xsize))
            info["tile_bits"].append(bits)
            xsize = (xsize + (1 << bits) - 1) >> bits
    px = _image_stream(br, xsize, h, True, info)
    info["bits"] = br.pos
    for kind, bits, sub, width in reversed(transforms):
        if kind == 0:
            _inverse_predictor(px, width, h, bits, sub)
        elif kind == 1:
            _inverse_cross_color(px, width, h, bits, sub)
        elif kind == 2:
            px = [(v & 0xFF00FF00) | ((((v >> 16) + (v >> 8)) & 255) << 16) | ((v + (v >> 8)) & 255) for v in px]
        else:
            packed_w, per, mask, step = (width + (1 << bits) - 1) >> bits, 1 << bits, (1 << (8 >> bits)) - 1, 8 >> bits
            out = [0] * (width * h)
            for y in range(h):
                for x in range(width):
                    idx = ((px[y * packed_w + (x >> bits)] >> 8) >> ((x & (per - 1)) * step)) & mask if bits else (px[y * packed_w + x] >> 8) & 255
                    out[y * width + x] = sub[idx] if idx < len(sub) else 0
            px = out
    a = np.array(px, np.uint32).reshape(h, w)
    rgba = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], -1).astype(np.uint8)
    return rgba, info
