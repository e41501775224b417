"""A seeded writer of legal VP8 key frames (RFC 6386) for the lossy WebP decoder's tests, in the spirit of tests/vp8l_gen.py: a
bool ENCODER, random modes and random coefficient levels (large ones too: they drive every clamp), and a switch for each
feature libwebp's own encoder never writes -- the simple filter, sharpness, loop-filter deltas, 2/4/8 token partitions,
segments in delta mode or without a map, coefficient probability updates, no skip probability, profiles 1..3, scale bits --
and ALPH chunks raw or VP8L-coded under every filter.  The pictures are noise; libwebp through Pillow says what they decode to."""
import io
import os
import re
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_T = {}


def tables():
    """the format's constants, read from csrc/vp8_tables.inc"""
    if _T:
        return _T
    text = open(os.path.join(HERE, "..", "imageflow_amd", "csrc", "vp8_tables.inc")).read()
    text = re.sub(r"//[^\n]*", "", text)
    for m in re.finditer(r"static const (\w+) (\w+)((?:\[\d+\])+) = \{(.*?)\};", text, re.S):
        dims = [int(d) for d in re.findall(r"\[(\d+)\]", m.group(3))]
        vals = np.array([int(v) for v in re.findall(r"-?\d+", m.group(4))], np.int64)
        _T[m.group(2)] = vals.reshape(dims)
    return _T


class BoolEncoder:
    """RFC 6386 7.3"""

    def __init__(self):
        self.out = bytearray()
        self.range, self.bottom, self.bit_count = 255, 0, 24

    def _carry(self):
        i = len(self.out) - 1
        while i >= 0 and self.out[i] == 255:
            self.out[i] = 0
            i -= 1
        self.out[i] += 1

    def put(self, bit, prob=128):
        split = 1 + (((self.range - 1) * int(prob)) >> 8)
        if bit:
            self.bottom += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            if self.bottom & (1 << 31):
                self._carry()
            self.bottom = (self.bottom << 1) & 0xFFFFFFFF
            self.bit_count -= 1
            if self.bit_count == 0:
                self.out.append(self.bottom >> 24)
                self.bottom &= (1 << 24) - 1
                self.bit_count = 8

    def value(self, v, bits):
        for i in range(bits - 1, -1, -1):
            self.put((v >> i) & 1)

    def signed(self, v, bits):
        self.value(abs(v), bits)
        self.put(1 if v < 0 else 0)

    def optional_signed(self, v, bits):
        self.put(1 if v else 0)
        if v:
            self.signed(v, bits)

    def finish(self):
        c, v = self.bit_count, self.bottom
        if v & (1 << (32 - c)):
            self._carry()
        v = (v << (c & 7)) & 0xFFFFFFFF
        for _ in range(c >> 3):
            v = (v << 8) & 0xFFFFFFFF
        for _ in range(4):
            self.out.append((v >> 24) & 255)
            v = (v << 8) & 0xFFFFFFFF
        return bytes(self.out)


def _tree_paths(tree):
    """leaf -> [(node, bit)] along the sub-block mode tree (node: which probability)"""
    paths = {}

    def walk(node, path):
        for bit in (0, 1):
            nxt = int(tree[2 * node + bit])
            if nxt <= 0:
                paths[-nxt] = path + [(node, bit)]
            else:
                walk(nxt, path + [(node, bit)])
    walk(0, [])
    return paths


def _put_large(e, v, p):
    if v == 2:
        e.put(0, p[3]); e.put(0, p[4])
    elif v <= 4:
        e.put(0, p[3]); e.put(1, p[4]); e.put(v - 3, p[5])
    elif v <= 6:
        e.put(1, p[3]); e.put(0, p[6]); e.put(0, p[7]); e.put(v - 5, 159)
    elif v <= 10:
        e.put(1, p[3]); e.put(0, p[6]); e.put(1, p[7]); e.put((v - 7) >> 1, 165); e.put((v - 7) & 1, 145)
    else:
        T = tables()
        cat = 0 if v <= 18 else 1 if v <= 34 else 2 if v <= 66 else 3
        tab = [int(x) for x in T[("kVp8Cat3", "kVp8Cat4", "kVp8Cat5", "kVp8Cat6")[cat]] if x]
        e.put(1, p[3]); e.put(1, p[6]); e.put(cat >> 1, p[8]); e.put(cat & 1, p[9 + (cat >> 1)])
        extra = v - 3 - (8 << cat)
        for i, prob in enumerate(tab):
            e.put((extra >> (len(tab) - 1 - i)) & 1, prob)


def _put_block(e, probs, ctx, first, levels):
    """levels: 16 values in zigzag order; -> 1 where a level was coded"""
    bands = tables()["kVp8Bands"]
    last = max([i for i in range(first, 16) if levels[i]], default=-1)
    n = first
    p = probs[bands[n]][ctx]
    while n < 16:
        if n > last:
            e.put(0, p[0])
            break
        e.put(1, p[0])
        while not levels[n]:
            e.put(0, p[1])
            n += 1
            p = probs[bands[n]][0]
        e.put(1, p[1])
        v = abs(int(levels[n]))
        if v == 1:
            e.put(0, p[2])
        else:
            e.put(1, p[2])
            _put_large(e, v, p)
        e.put(1 if levels[n] < 0 else 0, 128)
        n += 1
        p = probs[bands[n]][1 if v == 1 else 2]
    return 1 if last >= first else 0


def _random_levels(rng, first, density, big):
    lv = np.zeros(16, np.int64)
    if rng.random() < density:
        count = int(rng.integers(1, 17 - first))
        at = rng.choice(np.arange(first, 16), count, replace=False)
        kind = rng.random(count)
        mag = np.where(kind < 0.6, rng.integers(1, 3, count), np.where(kind < 0.9, rng.integers(1, 12, count), rng.integers(11, big, count)))
        lv[at] = mag * rng.choice([-1, 1], count)
    return lv


def write_frame(seed, w, h, simple=False, level=20, sharpness=0, lf_delta=None, log2_parts=0, segments=None, coeff_updates=0,
                skip_prob=200, profile=0, scale=(0, 0), base_q=40, dq=(0, 0, 0, 0, 0), density=0.5, big=300, i4_share=0.5):
    """-> the `VP8 ` chunk's bytes.  lf_delta: (ref deltas[4], mode deltas[4]); segments: dict(update_map, absolute, quant[4],
    strength[4], probs[3]) -- update_map False writes the data without a map; skip_prob None: no skip flags."""
    T = tables()
    rng = np.random.default_rng(seed)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    e = BoolEncoder()
    e.put(0); e.put(0)                                                        # colour space, clamp type
    e.put(1 if segments else 0)
    if segments:
        e.put(1 if segments["update_map"] else 0)
        e.put(1)                                                              # update the segments' data
        e.put(1 if segments["absolute"] else 0)
        for q in segments["quant"]:
            e.optional_signed(q, 7)
        for s in segments["strength"]:
            e.optional_signed(s, 6)
        if segments["update_map"]:
            for p in segments["probs"]:
                e.put(0 if p == 255 else 1)
                if p != 255:
                    e.value(p, 8)
    e.put(1 if simple else 0); e.value(level, 6); e.value(sharpness, 3)
    e.put(1 if lf_delta else 0)
    if lf_delta:
        e.put(1)
        for group in lf_delta:
            for d in group:
                e.optional_signed(d, 6)
    e.value(log2_parts, 2)
    e.value(base_q, 7)
    for d in dq:
        e.optional_signed(d, 4)
    e.put(0)                                                                  # refresh entropy probabilities
    probs = T["kVp8CoeffProba0"].copy()
    update = T["kVp8CoeffUpdateProba"]
    chosen = set(int(i) for i in rng.choice(4 * 8 * 3 * 11, coeff_updates, replace=False)) if coeff_updates else set()
    for i, idx in enumerate(np.ndindex(4, 8, 3, 11)):
        if i in chosen:
            e.put(1, update[idx])
            probs[idx] = int(rng.integers(1, 256))
            e.value(int(probs[idx]), 8)
        else:
            e.put(0, update[idx])
    e.put(0 if skip_prob is None else 1)
    if skip_prob is not None:
        e.value(skip_prob, 8)

    paths = _tree_paths(T["kVp8BModeTree"])
    bprob = T["kVp8BModesProba"]
    n_parts = 1 << log2_parts
    parts = [BoolEncoder() for _ in range(n_parts)]
    intra_t = np.zeros(4 * mbw, np.int64)
    top_nz, top_dc = np.zeros((mbw, 8), np.int64), np.zeros(mbw, np.int64)       # 4 luma, 2 U, 2 V columns
    zig = T["kVp8Zigzag"]
    del zig                                                                        # (levels are written in zigzag order: nothing to undo)
    for my in range(mbh):
        left_modes = np.zeros(4, np.int64)
        left_nz, left_dc = np.zeros(8, np.int64), 0
        t = parts[my & (n_parts - 1)]
        for mx in range(mbw):
            if segments and segments["update_map"]:
                seg = int(rng.integers(0, 4))
                sp = segments["probs"]
                e.put(seg >> 1, sp[0]); e.put(seg & 1, sp[1 + (seg >> 1)])
            skip = 0
            if skip_prob is not None:
                skip = 1 if rng.random() < 0.25 else 0
                e.put(skip, skip_prob)
            i4 = rng.random() < i4_share
            top = intra_t[4 * mx:4 * mx + 4]
            if not i4:
                ymode = int(rng.integers(0, 4))                                    # DC TM V H
                e.put(1, 145)
                if ymode in (1, 3):
                    e.put(1, 156); e.put(1 if ymode == 1 else 0, 128)
                else:
                    e.put(0, 156); e.put(1 if ymode == 2 else 0, 163)
                top[:] = ymode
                left_modes[:] = ymode
            else:
                e.put(0, 145)
                for y in range(4):
                    ymode = int(left_modes[y])
                    for x in range(4):
                        mode = int(rng.integers(0, 10))
                        p = bprob[top[x]][ymode]
                        for node, bit in paths[mode]:
                            e.put(bit, p[node])
                        ymode = mode
                        top[x] = mode
                    left_modes[y] = ymode
            uv = int(rng.integers(0, 4))
            if uv == 0:
                e.put(0, 142)
            elif uv == 2:
                e.put(1, 142); e.put(0, 114)
            else:
                e.put(1, 142); e.put(1, 114); e.put(1 if uv == 1 else 0, 183)
            # tokens
            if skip:
                top_nz[mx] = 0
                left_nz[:] = 0
                if not i4:
                    top_dc[mx] = 0
                    left_dc = 0
                continue
            first, kind = 0, 3
            if not i4:
                nz = _put_block(t, probs[1], int(top_dc[mx] + left_dc), 0, _random_levels(rng, 0, density, big))
                top_dc[mx] = left_dc = nz
                first, kind = 1, 0
            for y in range(4):
                for x in range(4):
                    nz = _put_block(t, probs[kind], int(top_nz[mx][x] + left_nz[y]), first, _random_levels(rng, first, density, big))
                    top_nz[mx][x] = left_nz[y] = nz
            for c in (4, 6):
                for y in range(2):
                    for x in range(2):
                        nz = _put_block(t, probs[2], int(top_nz[mx][c + x] + left_nz[c + y]), 0, _random_levels(rng, 0, density, big))
                        top_nz[mx][c + x] = left_nz[c + y] = nz
    first_part = e.finish()
    bodies = [p.finish() for p in parts]
    sizes = b"".join(struct.pack("<I", len(b))[:3] for b in bodies[:-1])
    tag = (0) | (profile << 1) | (1 << 4) | (len(first_part) << 5)
    head = struct.pack("<I", tag)[:3] + b"\x9d\x01\x2a" + struct.pack("<HH", w | scale[0] << 14, h | scale[1] << 14)
    return head + first_part + sizes + b"".join(bodies)


def chunk(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def riff(vp8, alph=None, w=0, h=0, iccp=None):
    """a simple file, or VP8X (+ ICCP) (+ ALPH) + VP8"""
    if alph is None and iccp is None:
        body = chunk(b"VP8 ", vp8)
    else:
        flags = (0x10 if alph is not None else 0) | (0x20 if iccp is not None else 0)
        vp8x = bytes([flags, 0, 0, 0]) + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3]
        body = chunk(b"VP8X", vp8x) + (chunk(b"ICCP", iccp) if iccp is not None else b"") + (chunk(b"ALPH", alph) if alph is not None else b"") + chunk(b"VP8 ", vp8)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body


def chunks_of(data):
    """[(tag, offset of the body, size)] of a RIFF file"""
    out, at = [], 12
    while at + 8 <= len(data):
        size = struct.unpack_from("<I", data, at + 4)[0]
        out.append((data[at:at + 4], at + 8, size))
        at += 8 + size + (size & 1)
    return out


def chunk_body(data, tag):
    for t, at, size in chunks_of(data):
        if t == tag:
            return data[at:at + size]
    return None


def alpha_residual(alpha, filt):
    """what the ALPH chunk codes for an alpha plane [h, w] under filter 0..3"""
    a = alpha.astype(np.int64)
    pred = np.zeros_like(a)
    if filt:
        pred[0, 1:] = a[0, :-1]
        pred[1:, 0] = a[:-1, 0]
        left, top, tl = a[1:, :-1], a[:-1, 1:], a[:-1, :-1]
        pred[1:, 1:] = left if filt == 1 else top if filt == 2 else np.clip(left + top - tl, 0, 255)
    return ((a - pred) & 255).astype(np.uint8)


def alph_chunk(alpha, filt, vp8l):
    """the ALPH chunk's bytes: raw, or VP8L-coded (libwebp's lossless encoder through Pillow, its five header bytes dropped)"""
    res = alpha_residual(alpha, filt)
    if not vp8l:
        return bytes([filt << 2]) + res.tobytes()
    from PIL import Image
    rgba = np.zeros(res.shape + (4,), np.uint8)
    rgba[..., 1] = res
    rgba[..., 3] = 255
    buf = io.BytesIO()
    Image.fromarray(rgba, "RGBA").save(buf, "WEBP", lossless=True, quality=50, method=3, exact=True)
    return bytes([1 | filt << 2]) + chunk_body(buf.getvalue(), b"VP8L")[5:]


def random_alpha(seed, w, h):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(128 + 100 * np.sin(x / 5.0 + y / 7.0) + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)


SEGMENTS = dict(update_map=True, absolute=True, quant=[20, 50, 90, 120], strength=[10, 25, 45, 63], probs=[120, 200, 60])
W, H = 48, 32


def option_files():
    """name -> file bytes: one file per feature libwebp's encoder never writes, 48 x 32, and one 17 x 33"""
    f = {}

    def add(name, seed, alph=None, w=W, h=H, **k):
        f[name] = riff(write_frame(seed, w, h, **k), alph, w, h)
    add("plain", 1)
    add("simple_filter", 2, simple=True, level=30)
    for s in range(1, 8):
        add("sharpness_%d" % s, 10 + s, sharpness=s, level=10 + 7 * s)
    add("lf_deltas", 20, lf_delta=([6, 0, -3, 2], [-12, 3, 0, 1]), level=25)
    add("lf_deltas_clamped", 21, lf_delta=([40, 0, 0, 0], [30, 0, 0, 0]), level=50)
    for p in (1, 2, 3):
        add("partitions_%d" % (1 << p), 30 + p, log2_parts=p, w=40, h=72)
    add("segments_absolute", 40, segments=SEGMENTS)
    add("segments_delta", 41, segments=dict(SEGMENTS, absolute=False, quant=[-20, 0, 15, 60], strength=[-15, 0, 9, 40]))
    add("segments_no_map", 42, segments=dict(SEGMENTS, update_map=False))
    add("segments_simple", 43, segments=SEGMENTS, simple=True)
    add("coeff_updates", 50, coeff_updates=200)
    add("no_skip_probability", 51, skip_prob=None)
    for p in (1, 2, 3):
        add("profile_%d" % p, 60 + p, profile=p)
    add("scale_bits", 64, scale=(1, 2))
    add("quant_deltas", 65, base_q=100, dq=(-7, 5, -15, 15, 9))
    add("quant_low", 66, base_q=0, dq=(-3, 0, -9, 0, 0))
    add("large_levels", 67, big=2114, base_q=127, density=0.8)
    add("no_filter", 68, level=0)
    add("all_i16", 69, i4_share=0.0)
    add("all_i4", 70, i4_share=1.0, density=0.9)
    add("odd_17x33", 71, w=17, h=33)
    for filt in range(4):
        add("alph_raw_f%d" % filt, 80 + filt, alph=alph_chunk(random_alpha(filt, W, H), filt, False))
        add("alph_vp8l_f%d" % filt, 90 + filt, alph=alph_chunk(random_alpha(10 + filt, W, H), filt, True))
    add("alph_tall_gradient", 99, alph=alph_chunk(random_alpha(20, 17, 133), 3, True), w=17, h=133)
    return f
