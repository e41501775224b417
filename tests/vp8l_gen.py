"""A seeded writer of VP8L streams libwebp's encoder does not produce, for the tests of the device WebP decoder (in the spirit
of tests/deflate_gen.py): transforms in any order (a predictor behind colour indexing), predictor tiles whose modes cycle
through all 14, tile bits 2 and 9, a colour cache of 11 bits, normal codes with one used symbol of a length above 1,
max_symbol below the alphabet, 15-bit codes, distance codes 1..120 at widths where the clamp to 1 fires, distance-1 copies
of 4096 pixels, copies that cross a meta-tile boundary into another group, VP8X wrappers with odd padding -- and streams
damaged in one chosen way.  The writer never computes a pixel: it writes RESIDUALS and tokens, and what they decode to is
what libwebp says (a generated file counts only if Pillow decodes it and tests/vp8l_reader.py agrees: tests/test_vp8l_gen.py).
Every writer returns its counts, from which the tests assert the coverage."""
import struct

import numpy as np

from tests.vp8l_reader import CODE_LENGTH_ORDER, DISTANCE_MAP

PREDICTOR, CROSS_COLOR, SUBTRACT_GREEN, COLOR_INDEXING = range(4)
_CACHE = {}


class Bits:
    """values low bit first, prefix codes high bit first"""
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0 and value == 0, (value, bits)
        self.v |= value << self.n
        self.n += bits

    def code(self, value, bits):
        for i in range(bits - 1, -1, -1):
            self.put((value >> i) & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def shape_lengths(m, deep):
    """the lengths of a complete code of m >= 2 symbols: balanced, or (deep) with a branch that goes down to 15 bits"""
    leaves = [1, 1]
    while len(leaves) < m:
        l = max(leaves) if deep and max(leaves) < 15 else min(leaves)
        leaves.remove(l)
        leaves += [l + 1, l + 1]
    return sorted(leaves)


class Code:
    def __init__(self, alphabet, lengths):
        self.alphabet, self.lengths = alphabet, dict(lengths)
        self.single = len(self.lengths) == 1
        self.table, code = {}, 0
        for n in range(1, 16):
            for s in sorted(self.lengths):
                if self.lengths[s] == n:
                    self.table[s] = (code, n)
                    code += 1
            code <<= 1

    def emit(self, w, s):
        assert s in self.lengths, (s, sorted(self.lengths))
        if not self.single:
            w.code(*self.table[s])

    def write_simple(self, w):
        used = sorted(self.lengths)
        assert len(used) in (1, 2) and used[-1] < 256
        w.put(1, 1)
        w.put(len(used) - 1, 1)
        if used[0] < 2:
            w.put(0, 1)
            w.put(used[0], 1)
        else:
            w.put(1, 1)
            w.put(used[0], 8)
        if len(used) == 2:
            w.put(used[1], 8)

    def write_normal(self, w, max_symbol, counts):
        L = [self.lengths.get(s, 0) for s in range(self.alphabet)]
        toks, i, prev = [], 0, 8
        while i < len(L):
            v, run = L[i], 1
            while i + run < len(L) and L[i + run] == v:
                run += 1
            i += run
            if v == 0:
                while run >= 11:
                    t = min(run, 138)
                    toks.append((18, t - 11))
                    run -= t
                if run >= 3:
                    toks.append((17, run - 3))
                    run = 0
                toks += [(0, 0)] * run
            else:
                if prev != v:
                    toks.append((v, 0))
                    prev, run = v, run - 1
                while run >= 3:
                    t = min(run, 6)
                    toks.append((16, t - 3))
                    counts["repeat_16"] = counts.get("repeat_16", 0) + 1
                    run -= t
                toks += [(v, 0)] * run
        if max_symbol:
            while len(toks) > 2 and toks[-1][0] in (0, 17, 18):
                toks.pop()
            counts["max_symbol"] = counts.get("max_symbol", 0) + 1
        used = sorted({t[0] for t in toks})
        cl = Code(19, {used[0]: 1} if len(used) == 1 else dict(zip(used, shape_lengths(len(used), False))))
        n = max(4, 1 + max(CODE_LENGTH_ORDER.index(s) for s in used))
        w.put(0, 1)
        w.put(n - 4, 4)
        for k in range(n):
            w.put(cl.lengths.get(CODE_LENGTH_ORDER[k], 0), 3)
        if max_symbol:
            k = 0
            while len(toks) - 2 >= 1 << (2 + 2 * k):
                k += 1
            w.put(1, 1)
            w.put(k, 3)
            w.put(len(toks) - 2, 2 + 2 * k)
        else:
            w.put(0, 1)
        for s, extra in toks:
            cl.emit(w, s)
            if s >= 16:
                w.put(extra, {16: 2, 17: 3, 18: 7}[s])


def prefix_symbol(value):
    """(symbol, extra bits, extra value) of a length or a distance code >= 1"""
    if value <= 4:
        return value - 1, 0, 0
    d = value - 1
    high = d.bit_length() - 1
    extra = high - 1
    return 2 * high + ((d >> extra) & 1), extra, d & ((1 << extra) - 1)


def distance_of(code, xsize):
    if code > 120:
        return code - 120
    dx, dy = DISTANCE_MAP[code - 1]
    return max(1, dx + dy * xsize)


def make_code(alphabet, used, rng, opts, counts):
    used = sorted(used) or [0]
    if len(used) == 1:
        if opts.get("lone_long"):
            counts["lone_long"] = counts.get("lone_long", 0) + 1
            return Code(alphabet, {used[0]: 3}), "normal"
        return Code(alphabet, {used[0]: 1}), ("simple" if used[0] < 256 else "normal")
    if len(used) == 2 and used[1] < 256 and not opts.get("no_simple"):
        return Code(alphabet, {used[0]: 1, used[1]: 1}), "simple"
    shape = shape_lengths(len(used), bool(opts.get("deep")))
    if shape[-1] == 15:
        counts["len15"] = counts.get("len15", 0) + 1
    order = list(used)
    rng.shuffle(order)
    return Code(alphabet, dict(zip(order, shape))), "normal"


def write_image(w, rng, xsize, ysize, tokens, opts, counts, main=False, cache_bits=0, prefix_bits=0, entropy=None):
    """tokens: ("lit", argb) | ("copy", length, distance code) | ("cache", index); they cover xsize * ysize pixels (a damaged
    stream's may not)"""
    if cache_bits:
        w.put(1, 1)
        w.put(cache_bits, 4)
    else:
        w.put(0, 1)
    ent_x = 0
    if main:
        if entropy is not None:
            ent_x, ent_y = (xsize + (1 << prefix_bits) - 1) >> prefix_bits, (ysize + (1 << prefix_bits) - 1) >> prefix_bits
            assert len(entropy) == ent_x * ent_y
            w.put(1, 1)
            w.put(prefix_bits - 2, 3)
            write_image(w, rng, ent_x, ent_y, [("lit", g << 8) for g in entropy], {}, {})
        else:
            w.put(0, 1)
    n_groups = max(entropy) + 1 if entropy is not None else 1
    alphabets = (256 + 24 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)

    def walk(visit):
        pos = 0
        for t in tokens:
            x, y = pos % xsize, pos // xsize
            g = entropy[(y >> prefix_bits) * ent_x + (x >> prefix_bits)] if entropy is not None and pos < xsize * ysize else 0
            visit(g, t, pos)
            pos += t[1] if t[0] == "copy" else 1

    used = [[set() for _ in range(5)] for _ in range(n_groups)]

    def count(g, t, pos):
        if t[0] == "lit":
            v = t[1]
            for slot, s in enumerate(((v >> 8) & 255, (v >> 16) & 255, v & 255, v >> 24)):
                used[g][slot].add(s)
        elif t[0] == "copy":
            used[g][0].add(256 + prefix_symbol(t[1])[0])
            used[g][4].add(prefix_symbol(t[2])[0])
        else:
            used[g][0].add(280 + t[1])
    walk(count)
    codes, legal = [], True
    for g in range(n_groups):
        five = []
        for slot in range(5):
            code, form = make_code(alphabets[slot], used[g][slot], rng, opts, counts)
            if slot == 4 and opts.get("distance_simple"):          # a simple code that names these symbols, in or beyond the alphabet of 40
                code, form = Code(256, {s: 1 for s in opts["distance_simple"]}), "simple"
            bad = opts.get("bad_code")
            if bad and g == 0 and slot == 1:
                code, form, legal = Code(256, bad), "normal", False
            if form == "simple":
                code.write_simple(w)
            else:
                code.write_normal(w, bool(opts.get("max_symbol")) and slot == 0, counts)
            five.append(code)
        codes.append(five)
    if not legal:
        w.put(0, 32)                                             # (the reader never comes here)
        return
    state = {"g": None}

    def emit(g, t, pos):
        c = codes[g]
        if t[0] == "lit":
            v = t[1]
            for slot, s in enumerate(((v >> 8) & 255, (v >> 16) & 255, v & 255, v >> 24)):
                c[slot].emit(w, s)
        elif t[0] == "copy":
            s, nb, ev = prefix_symbol(t[1])
            c[0].emit(w, 256 + s)
            w.put(ev, nb)
            s, nb, ev = prefix_symbol(t[2])
            c[4].emit(w, s)
            w.put(ev, nb)
            end = pos + t[1]
            if entropy is not None and end < xsize * ysize:
                g2 = entropy[((end // xsize) >> prefix_bits) * ent_x + ((end % xsize) >> prefix_bits)]
                if g2 != g and (end % xsize) & ((1 << prefix_bits) - 1):      # (no tile starts there: the group is looked up behind the copy)
                    counts["copy_into_other_group_mid_tile"] = counts.get("copy_into_other_group_mid_tile", 0) + 1
                if g2 != g:
                    counts["copy_into_other_group"] = counts.get("copy_into_other_group", 0) + 1
        else:
            c[0].emit(w, 280 + t[1])
        state["g"] = g
    walk(emit)


def random_tokens(rng, xsize, ysize, opts, counts, cache_bits=0):
    """a token list that covers the image: literals from small per-channel sets, copies, cache symbols; opts["forced"] is a
    list of (position at or after which, token) placed as soon as they are legal"""
    n, pos, toks = xsize * ysize, 0, []
    greens = rng.integers(0, 256, opts.get("greens", 20))
    others = rng.integers(0, 256, (3, opts.get("others", 5)))
    forced = list(opts.get("forced", []))
    every_code = list(range(1, 121)) if opts.get("every_distance_code") else []
    while pos < n:
        tok = None
        if forced and pos >= forced[0][0]:
            t = forced[0][1]
            if distance_of(t[2], xsize) <= pos and pos + t[1] <= n:
                tok = forced.pop(0)[1]
        if tok is None and every_code and distance_of(every_code[0], xsize) <= pos and pos + 2 <= n:
            tok = ("copy", int(rng.integers(1, min(9, n - pos) + 1)), every_code.pop(0))
        if tok is None:
            r = rng.random()
            if r < opts.get("p_copy", 0.2) and pos > 0:
                length = int(min(n - pos, rng.choice(opts.get("lengths", [1, 2, 3, 5, 8, 17, 64, 65, 130, 700]))))
                if rng.random() < 0.5:
                    code = int(rng.integers(1, 121))
                    if distance_of(code, xsize) > pos:
                        code = 121
                else:
                    code = 120 + int(rng.integers(1, min(pos, 3000) + 1))
                tok = ("copy", length, code)
            elif cache_bits and r < opts.get("p_copy", 0.2) + opts.get("p_cache", 0.2):
                tok = ("cache", int(rng.integers(0, 1 << cache_bits)))
            else:
                a = 0xFF if not opts.get("alpha") else int(others[2][rng.integers(0, others.shape[1])])
                tok = ("lit", a << 24 | int(others[0][rng.integers(0, others.shape[1])]) << 16 | int(greens[rng.integers(0, len(greens))]) << 8 |
                       int(others[1][rng.integers(0, others.shape[1])]))
        if tok[0] == "copy":
            d = distance_of(tok[2], xsize)
            counts.setdefault("distance_codes", set()).add(min(tok[2], 121))
            if tok[2] <= 120 and sum(DISTANCE_MAP[tok[2] - 1][k] * (1, xsize)[k] for k in (0, 1)) < 1:
                counts["clamped"] = counts.get("clamped", 0) + 1
            if d == 1 and tok[1] == 4096:
                counts["distance_1_length_4096"] = counts.get("distance_1_length_4096", 0) + 1
            if d < tok[1]:
                counts["overlapping"] = counts.get("overlapping", 0) + 1
        toks.append(tok)
        pos += tok[1] if tok[0] == "copy" else 1
    return toks


def write_payload(seed, w, h, transforms=(), alpha=1, cache_bits=0, prefix_bits=0, groups=1, opts=None, damage=None):
    """-> (the VP8L payload, counts).  transforms: (kind, tile bits or palette size) in file order."""
    rng = np.random.default_rng(seed)
    opts, counts = dict(opts or {}), {}
    b = Bits()
    b.put(0x2F, 8)
    b.put(w - 1, 14)
    b.put(h - 1, 14)
    b.put(alpha, 1)
    b.put(0, 3)
    xsize = w
    counts["transforms"] = [t[0] for t in transforms]
    for kind, arg in transforms:
        b.put(1, 1)
        b.put(kind, 2)
        if kind in (PREDICTOR, CROSS_COLOR):
            tx, ty = (xsize + (1 << arg) - 1) >> arg, (h + (1 << arg) - 1) >> arg
            b.put(arg - 2, 3)
            if kind == PREDICTOR:
                modes = [(k + int(seed)) % 14 for k in range(tx * ty)]
                counts.setdefault("modes", set()).update(modes)
                counts.setdefault("predictor_bits", []).append(arg)
                if xsize != w:
                    counts["predictor_after_indexing"] = 1
                sub = [("lit", int(rng.integers(0, 256)) << 24 | int(rng.integers(0, 256)) << 16 | m << 8 | int(rng.integers(0, 4))) for m in modes]
            else:
                sub = [("lit", 0xFF000000 | int(rng.integers(0, 1 << 24))) for _ in range(tx * ty)]
            write_image(b, rng, tx, ty, sub, {}, {})
        elif kind == COLOR_INDEXING:
            b.put(arg - 1, 8)
            write_image(b, rng, arg, 1, [("lit", int(rng.integers(0, 1 << 32))) for _ in range(arg)], {}, {})
            bits = 3 if arg <= 2 else 2 if arg <= 4 else 1 if arg <= 16 else 0
            xsize = (xsize + (1 << bits) - 1) >> bits
    if damage == "transform_twice":
        b.put(1, 1)
        b.put(transforms[-1][0], 2)
        b.put(0, 16)
    b.put(0, 1)
    entropy = None
    if prefix_bits:
        ent = ((xsize + (1 << prefix_bits) - 1) >> prefix_bits) * ((h + (1 << prefix_bits) - 1) >> prefix_bits)
        entropy = [int(g) for g in rng.integers(0, groups, ent)]
        entropy[0] = groups - 1
    tokens = random_tokens(rng, xsize, h, opts, counts, cache_bits)
    if damage == "distance":
        tokens[0] = ("copy", 1, 121)
    elif damage == "copy_end":
        pos, keep = 0, 0
        while pos + (tokens[keep][1] if tokens[keep][0] == "copy" else 1) <= xsize * h - 10:
            pos += tokens[keep][1] if tokens[keep][0] == "copy" else 1
            keep += 1
        tokens = tokens[:keep] + [("copy", xsize * h - pos + 3, 121)]
    elif damage == "oversubscribed":
        opts["bad_code"] = {0: 1, 1: 1, 2: 1}
    elif damage == "incomplete":
        opts["bad_code"] = {0: 1, 1: 2}
    write_image(b, rng, xsize, h, tokens, opts, counts, main=True, cache_bits=cache_bits, prefix_bits=prefix_bits, entropy=entropy)
    counts["cache_bits"], counts["groups"] = cache_bits, groups
    return b.bytes(), counts


def chunk(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def riff(payload, before=(), after=(), vp8x=None, riff_delta=0, payload_tag=b"VP8L"):
    """a .webp file around a payload; vp8x: (flags, width, height) for an extended file; before / after: (tag, body) chunks"""
    body = b"WEBP"
    if vp8x is not None:
        flags, w, h = vp8x
        body += chunk(b"VP8X", bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little"))
    for tag, data in before:
        body += chunk(tag, data)
    body += chunk(payload_tag, payload)
    for tag, data in after:
        body += chunk(tag, data)
    return b"RIFF" + struct.pack("<I", len(body) + riff_delta) + body


def legal_files():
    """name -> (file, counts)"""
    if "legal" in _CACHE:
        return _CACHE["legal"]
    files = {}

    def add(name, *a, wrap=riff, **k):
        payload, counts = write_payload(*a, **k)
        files[name] = (wrap(payload), counts)
    add("predictor_after_indexing", 1, 45, 37, transforms=((COLOR_INDEXING, 13), (PREDICTOR, 2), (CROSS_COLOR, 3), (SUBTRACT_GREEN, 0)), opts={"greens": 40})
    add("indexing_last", 2, 33, 70, transforms=((SUBTRACT_GREEN, 0), (PREDICTOR, 3), (COLOR_INDEXING, 3)), opts={"greens": 30, "alpha": 1})
    add("tile_bits_9_cache_11", 3, 70, 66, transforms=((SUBTRACT_GREEN, 0), (CROSS_COLOR, 2), (PREDICTOR, 9)), cache_bits=11, opts={"greens": 60, "others": 9, "alpha": 1})
    add("codes", 4, 100, 90, opts={"greens": 50, "deep": 1, "lone_long": 1, "max_symbol": 1, "no_simple": 1, "forced": [(10, ("copy", 4096, 121)), (5000, ("copy", 4096, 2))]})
    add("distance_map_w3", 5, 3, 400, opts={"every_distance_code": 1, "p_copy": 0.3})
    add("distance_map_w1", 6, 1, 900, opts={"every_distance_code": 1, "p_copy": 0.3})
    add("distance_map_w23", 7, 23, 120, transforms=((PREDICTOR, 2),), opts={"every_distance_code": 1, "p_copy": 0.05})
    add("meta_groups", 8, 21, 19, transforms=((PREDICTOR, 2),), cache_bits=3, prefix_bits=2, groups=7, opts={"p_copy": 0.35, "alpha": 1, "lengths": [1, 2, 3, 5, 7, 11]})
    add("meta_groups_cache_11", 9, 40, 30, cache_bits=11, prefix_bits=3, groups=9, opts={"p_copy": 0.3, "greens": 90, "others": 30})
    add("vp8x_wrapped", 10, 19, 130, transforms=((PREDICTOR, 4),), opts={"alpha": 1},
        wrap=lambda p: riff(p, vp8x=(0x18, 19, 130), before=((b"ABCD", b"\1\2\3"),), after=((b"EXIF", b"Exif\0\0II*\0\x08\0\0\0\0\0\0"), (b"XMP ", b"<x/>"))))
    _CACHE["legal"] = files
    return files


def files_beyond_the_reader():
    """name -> (file, counts): legal for libwebp, but tests/vp8l_reader.py does not read them -- Pillow alone is their yardstick
    (alpha_is_used is set, so Pillow hands out all four channels)"""
    if "beyond" not in _CACHE:
        # a simple distance code of two symbols, one of them beyond the alphabet of 40: libwebp counts symbol 5 alone
        payload, counts = write_payload(11, 9, 7, alpha=1, opts={"p_copy": 0.0, "alpha": 1, "distance_simple": (5, 200)})
        _CACHE["beyond"] = {"simple_code_symbol_beyond_the_alphabet": (riff(payload), counts)}
    return _CACHE["beyond"]


def damaged_files():
    """name -> (file, the status word of csrc/webp_decode_core.hpp)"""
    if "damaged" in _CACHE:
        return _CACHE["damaged"]
    files = {}
    for k, (damage, status) in enumerate((("oversubscribed", 2), ("incomplete", 2), ("distance", 4), ("copy_end", 5), ("transform_twice", 7))):
        payload, _ = write_payload(50 + k, 30, 20, transforms=((SUBTRACT_GREEN, 0),), opts={"p_copy": 0.1}, damage=damage)
        files[damage] = (riff(payload), status)
    payload, _ = write_payload(60, 1, 1, opts={"p_copy": 0.0, "distance_simple": (255,)})     # the distance code's only symbol lies beyond its alphabet
    files["simple_code_only_symbol_beyond_the_alphabet"] = (riff(payload), 2)
    _CACHE["damaged"] = files
    return files
