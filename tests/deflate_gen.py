"""A seeded writer of legal deflate streams (RFC 1950 / 1951) that zlib's ENCODER never writes -- test infrastructure, and no
product code: nothing here is shared with csrc/png_encode_core.hpp.  zlib's DECODER accepts all of RFC 1951 and is the
yardstick: every stream made here inflates with zlib.decompress to the bytes its tokens define.

What the writer can do that zlib's encoder does not: matches at any distance up to 32768 (the far end of the window
included) and of any legal length, not the nearest and not the longest; length 258 as symbol 284 with extra 31; stored blocks
of any length that start at any bit offset; empty blocks of every type; dynamic blocks whose code lengths come from a
Huffman build on distorted frequencies (15-bit codes that the tokens really use, unused symbols with codes, HLIT / HDIST /
HCLEN padded, a one-code distance set, a distance set with no code), whose length sequence is run-length coded with random
splits, runs across the HLIT boundary included.

`stats` counts what a stream contains, so that coverage is asserted and not hoped for.  The flush threshold, the ring and the
staged-input size are the decoder's constants (csrc/png_decode_core.hpp): the writer follows the decoder's flush rule to know
where a match ends on a threshold.

    random_stream(rng, size)  -> (data, zlib stream, stats)     made-up tokens define the data; the first byte is 0
    reencode(data, rng)       -> (zlib stream, stats)           a random legal parse of given bytes
    names() / entry(name)     the corpus: fixed seeds, every stream rebuilt from its seed, at most 128 KiB inflated each
    damaged()                 name -> (stream, cap, status): derived from generator blocks by rule
    device_cases()            every (stream, cap, status) that tests send to a GPU; the sanitizer build sees them first
"""
import functools
import heapq
import random
import struct
import zlib
from bisect import bisect_right
from collections import Counter

import numpy as np

from tests import png_decode_oracle as O

RING, FLUSH, STAGE_IN, FAST_BITS = 32768, 8192, 4096, 10              # kInfRing, kInfFlush, kInfIn, kInfFastBits
OK, TRUNCATED, CODE_LENGTHS, ADLER = 0, 1, 4, 8
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
STORED_LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 65535)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0) + tuple(e for e in range(1, 14) for _ in (0, 1))
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
ALT_258 = (284, 5, 31)


def _length_symbols():
    t = [None] * 259
    for i, (base, e) in enumerate(zip(LEN_BASE, LEN_EXTRA)):
        for v in range(1 << e):
            if base + v <= 258:
                t[base + v] = (257 + i, e, v)                              # (258 ends as symbol 285: the later entry wins)
    return t


LEN_SYM = _length_symbols()


class BitSink:
    """the Bits writer of tests/test_png_decode_core.py, restated with a byte buffer behind it: values low bit first, Huffman
    codes high bit first"""
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits
        if self.n >= 512:
            self._spill()

    def _spill(self):
        k = self.n >> 3
        self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def align(self):
        self.n += (-self.n) & 7

    def raw(self, data):
        assert self.n & 7 == 0
        self._spill()
        self.out += data

    def bytes(self):
        self.align()
        self._spill()
        return bytes(self.out)


def reverse(code, bits):
    r = 0
    for _ in range(bits):
        r = r << 1 | (code & 1)
        code >>= 1
    return r


def canonical(lens):
    """code lengths -> [(the code bit-reversed, as the stream holds it; its length)] per symbol (RFC 1951 3.2.2)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l:
            out.append((reverse(nxt[l] & ((1 << l) - 1), l), l))
            nxt[l] += 1
        else:
            out.append((0, 0))
    return out


def limited_lengths(weights, limit):
    """{symbol: weight > 0} -> {symbol: length <= limit} of a COMPLETE prefix code (one symbol alone: one bit, the incomplete
    set zlib allows): Huffman's tree, clipped at `limit`, then the Kraft sum mended a length at a time"""
    syms = sorted(weights)
    if len(syms) == 1:
        return {syms[0]: 1}
    heap = [(weights[s], i) for i, s in enumerate(syms)]
    heapq.heapify(heap)
    parent, nid = {}, len(syms)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        parent[a[1]] = parent[b[1]] = nid
        heapq.heappush(heap, (a[0] + b[0], nid))
        nid += 1
    depth = {nid - 1: 0}
    for i in range(nid - 2, -1, -1):
        depth[i] = depth[parent[i]] + 1
    lens = [min(depth[i], limit) for i in range(len(syms))]
    full = 1 << limit
    kraft = sum(1 << (limit - l) for l in lens)
    order = sorted(range(len(syms)), key=lambda i: (-lens[i], i))
    while kraft > full:                                                    # over-subscribed by the clip: lengthen the deepest below the limit
        i = max((j for j in range(len(syms)) if lens[j] < limit), key=lambda j: (lens[j], j))
        lens[i] += 1
        kraft -= 1 << (limit - lens[i])
    while kraft < full:                                                    # what is left over: shorten, deepest first
        for i in order:
            while lens[i] > 1 and (1 << (limit - lens[i])) <= full - kraft:
                kraft += 1 << (limit - lens[i])
                lens[i] -= 1
        order.sort(key=lambda i: (-lens[i], i))
    return {s: lens[i] for i, s in enumerate(syms)}


def _fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def distorted_lengths(rng, freq, universe, limit, power, deep, unused):
    """code lengths for the symbols of `freq` (all get a code) out of range(universe): the frequencies raised to `power`;
    deep: the rarest (deep == "common": the commonest) 16..22 of them get Fibonacci weights below everybody else's (a chain as deep as the limit, which the
    tokens really use); unused: symbols that do not occur get codes too"""
    w = {s: float(f) ** power for s, f in freq.items()}
    if unused or (deep and len(w) < 18):
        spare = [s for s in range(universe) if s not in w]
        rng.shuffle(spare)
        take = spare[:rng.randint(1, max(1, len(spare)))] if unused else spare[:18 - len(w)]
        low = min(w.values()) if w else 1.0
        for s in take:
            w[s] = low * rng.choice((0.01, 0.5, 1.0))
    if deep and len(w) >= 3:
        k = min(len(w), rng.randint(16, 22))
        sign = -1 if deep == "common" else 1                                # the tokens' own rarest symbols go deepest -- or their commonest
        used = sorted(freq, key=lambda s: (sign * freq[s], rng.random()))
        chain = (used + [s for s in w if s not in freq])[:k]
        fib = _fib(k)
        top = float(fib[-1])
        w = {s: top * (1.0 + v / (1.0 + max(w.values()))) for s, v in w.items()}
        for s, f in zip(chain, fib):
            w[s] = float(f)
    return limited_lengths(w, limit)


def new_stats():
    return {"blocks": Counter(), "empty_blocks": Counter(), "stored_bit_offsets": Counter(), "stored_lengths": Counter(),
            "matches": Counter(), "headers": Counter(), "max_ll_code_used": 0, "max_d_code_used": 0, "walk_uses": 0,
            "runs_across_hlit": 0, "first_block_empty": False, "final_pad_bits": None, "inside_match": None, "inside_stored": None,
            "cuts": [], "compressed": 0, "inflated": 0}


def merge_stats(all_stats):
    out = new_stats()
    for s in all_stats:
        for k, v in s.items():
            if isinstance(v, Counter):
                out[k].update(v)
            elif k in ("max_ll_code_used", "max_d_code_used"):
                out[k] = max(out[k], v)
            elif k in ("walk_uses", "runs_across_hlit", "compressed", "inflated"):
                out[k] += v
    return out


class Writer:
    """one zlib stream, block by block; the tokens written so far define `data`"""
    def __init__(self, rng):
        self.rng, self.bits, self.data, self.stats = rng, BitSink(), bytearray(), new_stats()
        self.flushed, self.spans, self.done = 0, [], False                  # spans: (start, end, type) of every block
        self.bits.raw(b"\x78" + bytes([rng.choice((0x01, 0x5E, 0x9C, 0xDA))]))

    # -- what the decoder does with its window, restated: a flush whenever 8192 new bytes have gathered, down to a multiple of 16
    def _gathered(self):
        if len(self.data) - self.flushed >= FLUSH:
            self.flushed = len(self.data) & ~15

    def _crosses(self, a, b):
        """do the bits [a, b) lie on both sides of a multiple of 4096 bytes of the stream"""
        return b > a and a // (8 * STAGE_IN) != (b - 1) // (8 * STAGE_IN)

    def _open(self, kind, empty, last):
        st = self.stats
        assert not self.done
        if not self.spans:
            st["first_block_empty"] = empty
        st["blocks"][kind] += 1
        if empty:
            st["empty_blocks"][(kind, "last" if last else "not last")] += 1
        self.done = last

    def stored(self, payload, last=False):
        st, bits = self.stats, self.bits
        payload = bytes(payload)
        assert len(payload) <= 65535
        self._open("stored", not payload, last)
        a = bits.bitpos
        st["stored_bit_offsets"][a & 7] += 1
        st["stored_lengths"][len(payload)] += 1
        bits.put(1 if last else 0, 1)
        bits.put(0, 2)
        bits.align()
        bits.put(len(payload), 16)
        bits.put(len(payload) ^ 0xFFFF, 16)
        if self._crosses(a, bits.bitpos):
            st["headers"]["stored header across an input boundary"] += 1
        bits.raw(payload)
        start = len(self.data)
        if len(payload) >= 2:
            st["inside_stored"] = start + len(payload) // 2
        for i in range(0, len(payload), 4096):                             # the decoder copies 4096 at a time and looks after each
            self.data += payload[i:i + 4096]
            self._gathered()
        self.spans.append((start, len(self.data), "stored"))
        st["cuts"].append(bits.bitpos)

    def block(self, tokens, kind, last=False, **opt):
        """tokens: a literal is an int, a match (length, distance) or (length, distance, as symbol 284 + 31).  kind: "fixed" or
        "dynamic"; opt: plan_dynamic's"""
        rng, st, bits, data = self.rng, self.stats, self.bits, self.data
        res, llf, df = [], {256: 1}, {}
        for t in tokens:
            if isinstance(t, int):
                res.append(t)
                llf[t] = llf.get(t, 0) + 1
            else:
                n, dist = t[0], t[1]
                assert 3 <= n <= 258 and 1 <= dist <= RING
                alt = n == 258 and (t[2] if len(t) > 2 else rng.random() < 0.5)
                ls, le, lv = ALT_258 if alt else LEN_SYM[n]
                ds = bisect_right(DIST_BASE, dist) - 1
                res.append((n, dist, ls, le, lv, ds, DIST_EXTRA[ds], dist - DIST_BASE[ds]))
                llf[ls] = llf.get(ls, 0) + 1
                df[ds] = df.get(ds, 0) + 1
        self._open(kind, not res, last)
        a = bits.bitpos
        bits.put(1 if last else 0, 1)
        if kind == "fixed":
            bits.put(1, 2)
            ll_lens, d_lens = FIXED_LL, FIXED_D
        else:
            bits.put(2, 2)
            plan = plan_dynamic(rng, llf, df, **opt)
            write_dynamic_header(bits, plan)
            ll_lens, d_lens = plan["ll"], plan["d"]
            st["runs_across_hlit"] += plan["runs_across_hlit"]
            for k in plan["shape"]:
                st["headers"][k] += 1
            if self._crosses(a, bits.bitpos):
                st["headers"]["dynamic header across an input boundary"] += 1
        st["cuts"].append(bits.bitpos)
        llc, dc = canonical(ll_lens), canonical(d_lens)
        m = st["matches"]
        start, my = len(data), kind
        for i, t in enumerate(res):
            if isinstance(t, int):
                c, l = llc[t]
                bits.put(c, l)
                data.append(t)
                if l > st["max_ll_code_used"]:
                    st["max_ll_code_used"] = l
                if l > FAST_BITS:
                    st["walk_uses"] += 1
            else:
                n, dist, ls, le, lv, ds, de, dv = t
                pos = len(data)
                assert dist <= pos, "a distance that reaches before the stream's start"
                ta = bits.bitpos
                c, l = llc[ls]
                c2, l2 = dc[ds]
                bits.put(c, l)
                bits.put(lv, le)
                bits.put(c2, l2)
                bits.put(dv, de)
                if l > st["max_ll_code_used"]:
                    st["max_ll_code_used"] = l
                if l2 > st["max_d_code_used"]:
                    st["max_d_code_used"] = l2
                st["walk_uses"] += (l > FAST_BITS) + (l2 > FAST_BITS)
                if self._crosses(ta, bits.bitpos):
                    m["token across an input boundary"] += 1
                src = pos - dist
                if dist >= n:
                    data += data[src:src + n]
                else:
                    data += (bytes(data[src:pos]) * (n // dist + 1))[:n]
                    m["dist 1..63, n > dist" if dist < 64 else "dist 64..257, n > dist"] += 1
                if dist == n:
                    m["dist == n"] += 1
                elif dist == n + 1:
                    m["dist == n + 1"] += 1
                if n == 258:
                    m["258 as symbol 284 + 31" if ls == 284 else "258 as symbol 285"] += 1
                if src // RING != (src + min(n, dist) - 1) // RING:
                    m["source wraps the ring"] += 1
                if pos // RING != (pos + n - 1) // RING:
                    m["destination wraps the ring"] += 1
                if dist + n > RING:
                    m["dist + n > 32768"] += 1
                    if pos > RING:
                        m["dist + n > 32768 above 32768"] += 1
                gathered = pos + n - self.flushed
                if gathered == FLUSH:
                    m["ends on a flush threshold"] += 1
                elif gathered > FLUSH:
                    m["crosses a flush threshold"] += 1
                if src < start:                                             # the source begins in an earlier block
                    between = False
                    for s0, s1, typ in reversed(self.spans):
                        if s1 <= src:
                            break
                        if typ == "stored" and s0 < min(s1, src + min(n, dist)):
                            m["into a stored block"] += 1
                        if s0 > src and s1 > s0 and typ != my:
                            between = True
                    if between:
                        m["across a block of another type"] += 1
                if n >= 4 and (st["inside_match"] is None or rng.random() < 0.02):
                    st["inside_match"] = pos + n // 2
            self._gathered()
            if i == len(res) // 2:
                st["cuts"].append(bits.bitpos)
        c, l = llc[256]
        bits.put(c, l)
        self.spans.append((start, len(data), kind))

    def finish(self):
        """-> (data, zlib stream, stats)"""
        assert self.done, "the last block must say that it is"
        st = self.stats
        st["final_pad_bits"] = (-self.bits.bitpos) & 7
        self.bits.align()
        self.bits.raw(struct.pack(">I", zlib.adler32(bytes(self.data))))
        z = self.bits.bytes()
        st["compressed"], st["inflated"] = len(z), len(self.data)
        return bytes(self.data), z, st


# ---- dynamic headers ------------------------------------------------------------------------------------------------------------------
def run_length_code(rng, seq, hlit, mode):
    """the code lengths as (symbol, extra value, extra bits) items; mode: "none", "greedy" (the longest repeat every time) or
    "random" (a literal, or a repeat of any legal count, wherever one is possible) -> (items, runs that cross hlit)"""
    items, i, across = [], 0, 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        pick = (lambda lo, hi: hi) if mode == "greedy" else rng.randint
        rep = 0
        if mode != "none" and (mode == "greedy" or rng.random() < 0.75):
            if v == 0 and run >= 11 and (mode == "greedy" or rng.random() < 0.7):
                rep = pick(11, min(138, run))
                items.append((18, rep - 11, 7))
            elif v == 0 and run >= 3:
                rep = pick(3, min(10, run))
                items.append((17, rep - 3, 3))
            elif i > 0 and seq[i - 1] == v and run >= 3:
                rep = pick(3, min(6, run))
                items.append((16, rep - 3, 2))
        if rep:
            across += i < hlit < i + rep
            i += rep
        else:
            items.append((v, 0, 0))
            i += 1
    return items, across


def plan_dynamic(rng, llf, df, power=None, deep=None, unused=None, pad_hlit=None, pad_hdist=None, pad_hclen=None, rle=None,
                 edit_lens=None, edit_items=None, edit_cl=None, hlit_field=None, hdist_field=None):
    """everything a dynamic block's header holds, from the frequencies of its tokens.  The edit_* hooks and *_field overrides
    are for damaged(): they make the one change that the refusal under test needs."""
    def choose(v, options):
        return rng.choice(options) if v is None else v
    power = choose(power, (0.0, 0.35, 0.7, 1.0, 1.0, 1.5, 3.0))
    deep = choose(deep, (False, False, True))
    unused = choose(unused, (False, False, True))
    rle = choose(rle, ("none", "greedy", "random", "random", "random"))
    shape = []
    lens = distorted_lengths(rng, llf, 286, 15, power, deep, unused)
    ll = [lens.get(s, 0) for s in range(286)]
    if not df and not unused:
        d = [0] * 30
        shape.append("no distance code")
    else:
        if not df:
            df = {rng.randrange(30): 1}
        lens = distorted_lengths(rng, df, 30, 15, power, deep, unused and rng.random() < 0.7)
        d = [lens.get(s, 0) for s in range(30)]
        if sum(1 for l in d if l) == 1:
            shape.append("one distance code of one bit")
    if edit_lens:
        edit_lens(ll, d)
    hlit = max(257, max(s for s in range(286) if ll[s] or s == 256) + 1)
    hdist = max(1, max([s + 1 for s in range(30) if d[s]] or [1]))
    if choose(pad_hlit, (False, False, True)) and hlit < 286:
        hlit = rng.choice((286, rng.randint(hlit + 1, 286)))
        shape.append("HLIT padded")
    if choose(pad_hdist, (False, False, True)) and hdist < 30:
        hdist = rng.choice((30, rng.randint(hdist + 1, 30)))
        shape.append("HDIST padded")
    items, across = run_length_code(rng, ll[:hlit] + d[:hdist], hlit, rle)
    if edit_items:
        edit_items(items)
    clf = dict(Counter(it[0] for it in items))
    while len(clf) < 2:                                                     # (the code-length code may not be incomplete)
        clf.setdefault(rng.randrange(19), 1)
    lens = distorted_lengths(rng, clf, 19, 7, power, deep and rng.random() < 0.5, unused and rng.random() < 0.5)
    cl = [lens.get(s, 0) for s in range(19)]
    if edit_cl:
        edit_cl(cl)
    hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl[s]))
    if choose(pad_hclen, (False, True)) and hclen < 19:
        hclen = rng.randint(hclen + 1, 19)
        shape.append("HCLEN padded")
    shape.append("HCLEN %d" % hclen)
    if max(ll) == 15:
        shape.append("literal/length code of 15 bits")
    if max(d) == 15:
        shape.append("distance code of 15 bits")
    return {"ll": ll, "d": d, "hlit": hlit, "hdist": hdist, "items": items, "cl": cl, "hclen": hclen, "runs_across_hlit": across, "shape": shape,
            "hlit_field": hlit - 257 if hlit_field is None else hlit_field, "hdist_field": hdist - 1 if hdist_field is None else hdist_field}


def write_dynamic_header(bits, plan):
    bits.put(plan["hlit_field"], 5)
    bits.put(plan["hdist_field"], 5)
    bits.put(plan["hclen"] - 4, 4)
    for s in CL_ORDER[:plan["hclen"]]:
        bits.put(plan["cl"][s], 3)
    codes = canonical(plan["cl"])
    for sym, extra, ebits in plan["items"]:
        bits.put(*codes[sym])
        bits.put(extra, ebits)


# ---- token sources --------------------------------------------------------------------------------------------------------------------
def random_bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


def random_tokens(rng, pos, budget, count=None, p_literal=0.2, alphabet=256):
    """made-up tokens from output position `pos` on that produce at most `budget` bytes (exactly, with count None): a literal,
    or a match of any legal length at any distance -- short repeating patterns, dist == n, the window's far end"""
    out, made = [], 0
    while made < budget and (count is None or len(out) < count):
        left = budget - made
        if pos == 0:
            out.append(0)                                                   # (the stream's first byte: a filter type 0)
        elif left < 3 or rng.random() < p_literal:
            out.append(rng.randrange(alphabet))
        else:
            r = rng.random()
            n = 258 if r < 0.15 else 3 if r < 0.25 else rng.randint(4, 10) if r < 0.4 else rng.randint(3, 258)
            n = min(n, left)
            r, far = rng.random(), min(pos, RING)
            if r < 0.15:
                dist = rng.randint(1, 63)
            elif r < 0.3:
                dist = rng.randint(64, 257)
            elif r < 0.4:
                dist = n
            elif r < 0.5:
                dist = n + 1
            elif r < 0.7:
                dist = RING - rng.randint(0, 300)
            elif r < 0.85:
                dist = rng.randint(1, far)
            else:
                dist = 1 << rng.randint(0, 15)
            dist = max(1, min(dist, far))
            out.append((n, dist))
            pos += n
            made += n
            continue
        pos += 1
        made += 1
    return out


def common_prefix(a, b):
    """the number of leading bytes two equally long byte strings share"""
    if a == b:
        return len(a)
    lo, hi = 0, len(a)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[:mid] == b[:mid]:
            lo = mid
        else:
            hi = mid
    return lo


class Parser:
    """a random legal parse of given bytes: at each position a literal, or a match to SOME earlier occurrence found through a
    3-byte index -- any within 32768, not the nearest -- of any legal length, not the longest"""
    def __init__(self, data, rng):
        self.data, self.rng, self.index, self.indexed = bytes(data), rng, {}, 0

    def _index_to(self, pos):
        d = self.data
        for i in range(self.indexed, min(pos, len(d) - 2)):
            self.index.setdefault(d[i:i + 3], []).append(i)
        self.indexed = max(self.indexed, pos)

    def tokens(self, pos, count, p_literal):
        d, rng, out = self.data, self.rng, []
        while pos < len(d) and len(out) < count:
            self._index_to(pos)
            at = self.index.get(d[pos:pos + 3]) if pos + 3 <= len(d) else None
            if at and at[0] < pos - RING:
                at[:] = [i for i in at if i >= pos - RING]
            if not at or rng.random() < p_literal:
                out.append(d[pos])
                pos += 1
                continue
            src = at[-1] if rng.random() < 0.3 else rng.choice(at)
            span = min(258, len(d) - pos)
            longest = common_prefix(d[src:src + span], d[pos:pos + span])   # (the source may run into the match itself)
            n = longest if rng.random() < 0.4 else rng.randint(3, longest)
            out.append((n, pos - src))
            pos += n
        return out, pos


def reencode(data, rng, p_stored=0.15, **opt):
    """-> (zlib stream, stats): a random legal parse of `data`, cut into blocks of random type and size"""
    w, p, pos = Writer(rng), Parser(data, rng), 0
    while not w.done:
        r = rng.random()
        if r < p_stored:
            n = min(len(data) - pos, rng.choice(STORED_LENGTHS + (rng.randint(0, 3000),) * 4))
            pos += n
            w.stored(data[pos - n:pos], last=pos == len(data) and rng.random() < 0.8)
        else:
            tokens, pos = p.tokens(pos, rng.choice((0, 1, 50, 400, 2000, 10 ** 6)), rng.choice((0.02, 0.2, 0.6)))
            w.block(tokens, "fixed" if r < p_stored + 0.25 else "dynamic", last=pos == len(data) and rng.random() < 0.8, **opt)
    got, z, stats = w.finish()
    assert got == bytes(data)
    return z, stats


def random_stream(rng, size, p_stored=0.2, p_fixed=0.25, **opt):
    """-> (data, zlib stream, stats): at most `size` bytes (and nearly that many) defined by made-up tokens and stored bytes;
    the first byte is 0, so the data is one gray-8 row of filter type 0"""
    w = Writer(rng)
    while not w.done:
        pos = len(w.data)
        left = size - pos
        r = rng.random()
        if r < p_stored:
            n = rng.choice(STORED_LENGTHS + (rng.randint(0, 70000),) * 3 + (rng.randint(0, 600),) * 3)
            if n > min(left, 65535):
                n = rng.randint(0, min(left, 65535))
            payload = random_bytes(rng, n)
            if pos == 0 and n:
                payload = b"\0" + payload[1:]
            w.stored(payload, last=n == left and rng.random() < 0.7)
        else:
            count = rng.choice((0, 1, 2, 30, 100, 300, 800))
            tokens = random_tokens(rng, pos, left, count, rng.choice((0.02, 0.1, 0.3, 0.8, 1.0)), rng.choice((2, 16, 256)))
            made = sum(1 if isinstance(t, int) else t[0] for t in tokens)
            w.block(tokens, "fixed" if r < p_stored + p_fixed else "dynamic", last=made == left and rng.random() < 0.7, **opt)
    return w.finish()


# ---- the named constructions: at least one of everything the random streams could miss -------------------------------------------------
def _fill(w, target, kind="dynamic", **kw):
    """a block of made-up tokens that ends exactly at output position `target`"""
    assert target >= len(w.data)
    w.block(random_tokens(w.rng, len(w.data), target - len(w.data), None, **kw), kind)


def c_overlaps(rng):
    """short repeating patterns: dist in 1..63 and 64..257 with n > dist, dist == n, dist == n + 1, lengths around the 64 lanes"""
    w = Writer(rng)
    head = [0] + [rng.randrange(256) for _ in range(300)]
    for kind in ("fixed", "dynamic"):
        t = list(head)
        for dist in (1, 2, 3, 7, 31, 32, 33, 62, 63):
            for n in (dist + 1, 64, 65, 127, 129, 258):
                if n > dist and n >= 3:
                    t += [(n, dist), rng.randrange(256)]
        for dist in (64, 65, 100, 127, 128, 129, 191, 193, 256, 257):
            for n in (dist + 1, 2 * dist, 2 * dist + 1, 258):
                if dist < n <= 258:
                    t += [(n, dist), rng.randrange(256)]
        for n in (3, 4, 63, 64, 65, 128, 129, 257, 258):
            t += [(n, n), rng.randrange(256), (n, n + 1), rng.randrange(256)]
        w.block(t, kind, last=kind == "dynamic")
    return w.finish()


def c_ring_wraps(rng):
    """sources and destinations that wrap the 32 KiB ring, and matches through the staging row (dist + n > 32768) at output
    positions above 32768 -- also one that does all three at once"""
    w = Writer(rng)
    _fill(w, RING - 100, p_literal=0.3)
    w.block([(258, 5000), 7, (258, 227)], "fixed")                          # the destination wraps; then the source (32700..) does
    _fill(w, RING + 1000)
    w.block([(200, 1100), 9], "dynamic")                                    # source 32668..32868
    _fill(w, 40000, p_literal=0.5)
    t = []
    for dist, n in ((32700, 258), (32768, 258), (32767, 258), (32511, 258), (32510, 258), (32767, 3), (32705, 65), (32704, 65), (32768, 3)):
        t += [(n, dist), rng.randrange(256)]
    w.block(t, "dynamic", deep=True)
    _fill(w, 2 * RING - 100)
    w.block([(258, 32700), 1, 2, 3], "fixed")                               # staged, and the destination wraps
    _fill(w, 3 * RING - 120, "fixed", p_literal=0.1)
    w.block([(258, 32650, True), 4], "dynamic", last=True)                  # staged; source and destination both wrap
    return w.finish()


def _fill_to_threshold(w, n, kind="dynamic", **kw):
    """made-up tokens up to n bytes below the point where the decoder flushes next"""
    if w.flushed + FLUSH - n < len(w.data):
        _fill(w, w.flushed + FLUSH + 16, kind, **kw)
    _fill(w, w.flushed + FLUSH - n, kind, **kw)


def c_flush_thresholds(rng):
    """a match that ends exactly where 8192 new bytes have gathered, one that crosses that point, in both block types; the
    staging row at the threshold too"""
    w = Writer(rng)
    _fill(w, FLUSH - 100, "fixed", p_literal=0.4)
    w.block([(100, 200)], "fixed")
    assert w.flushed == FLUSH
    _fill(w, 2 * FLUSH - 50)
    w.block([(120, 64)], "dynamic")
    _fill_to_threshold(w, 258)
    w.block([(258, 1)], "dynamic")
    _fill(w, 5 * FLUSH)
    _fill_to_threshold(w, 258, p_literal=0.6)
    w.block([(258, 32768)], "fixed")                                        # staged, ends on the threshold
    _fill_to_threshold(w, 10, "fixed")
    w.block([(258, 32600), 5], "fixed", last=True)                          # staged, crosses it
    return w.finish()


def c_across_blocks(rng):
    """matches that reach back into a stored block, and across a block of another type"""
    w = Writer(rng)
    w.stored(b"\0" + random_bytes(rng, 999))
    w.block([(100, 500), 1, (258, 1001), (3, 3)], "fixed")
    w.block([rng.randrange(256) for _ in range(200)], "dynamic")
    w.stored(random_bytes(rng, 300))
    w.block([(50, 400), (258, 700), 6], "fixed")                            # into the dynamic block, across the stored one
    w.stored(b"")
    w.block([(258, len(w.data) - 10), 7, (40, 20)], "dynamic", last=True)   # into the first stored block, across everything
    return w.finish()


def c_stored_bit_offsets(rng):
    """a stored block's header at every bit offset 0..7, with the lengths where a copy of 4096 at a time can go wrong; the
    largest stored block at bit offset 5"""
    w = Writer(rng)
    for target, n in zip((0, 1, 2, 3, 4, 5, 6, 7, 5), (1, 0, 15, 16, 17, 4095, 4096, 4097, 65535)):
        while w.bits.bitpos & 7 != target:
            w.block([rng.randrange(144, 256)] if w.data else [], "fixed")   # 3 + 9 + 7 bits (empty: 3 + 7) move the offset
        payload = random_bytes(rng, n)
        w.stored(payload if w.data else b"\0" + payload[1:])
    w.stored(b"", last=True)
    return w.finish()


def c_input_boundaries(rng):
    """a stored header, a dynamic header and a match token whose bits lie on both sides of a 4096-byte boundary of the stream"""
    w = Writer(rng)

    def literals_until(lo, hi):                                             # the block ends (7 bits of end-of-block) at a bit in [lo, hi]
        t = [] if w.data else [0]
        while not lo <= w.bits.bitpos + 3 + 8 * len(t) + 7 <= hi:
            t.append(rng.randrange(144))
        w.block(t, "fixed")
    literals_until(8 * 4096 - 20, 8 * 4096 - 4)
    w.stored(random_bytes(rng, 10))
    literals_until(8 * 8192 - 40, 8 * 8192 - 10)
    w.block([(258, 4000), (3, 1)] + [rng.randrange(256) for _ in range(400)], "dynamic", rle="random")
    t = []
    while not 8 * 12288 - 14 <= w.bits.bitpos + 3 + 8 * len(t) <= 8 * 12288 - 7:
        t.append(rng.randrange(144))
    w.block(t + [(258, 11000 + rng.randrange(100), False), 8], "fixed", last=True)
    return w.finish()


def c_final_padding(rng, pad):
    """the last block ends `pad` bits short of a byte boundary: where the Adler-32 is read from"""
    for nine in range(8):
        w = Writer(random.Random(1000 + pad))
        w.block(random_tokens(w.rng, 0, 600, None, 0.3), "dynamic")
        w.block([65] + [200] * nine, "fixed", last=True)
        data, z, stats = w.finish()
        if stats["final_pad_bits"] == pad:
            return data, z, stats
    raise AssertionError(pad)


def c_empty_blocks(rng, last_kind):
    """every empty block type not last, the first block empty, and an empty last block of `last_kind`"""
    w = Writer(rng)
    kinds = ["stored", "fixed", "dynamic"]
    kinds = kinds[kinds.index(last_kind):] + kinds[:kinds.index(last_kind)]

    def empty(kind, last=False):
        if kind == "stored":
            w.stored(b"", last)
        else:
            w.block([], kind, last, unused=False if rng.random() < 0.5 else None)
    for k in kinds:
        empty(k)
    w.block(random_tokens(rng, 0, 500, None, 0.3), "dynamic")
    for k in reversed(kinds):
        empty(k)
        empty(k)
    w.stored(random_bytes(rng, 40))
    empty(last_kind, True)
    return w.finish()


def c_deep_codes(rng):
    """15-bit literal/length and distance codes that the tokens use: every look-up beyond the 10-bit table is a canonical walk"""
    w = Writer(rng)
    for i in range(6):
        t = random_tokens(rng, len(w.data), 12000, None, 0.7, 24 if i in (1, 4) else 256)
        w.block(t, "dynamic", last=i == 5, deep="common" if i in (1, 4) else True, power=rng.choice((0.35, 1.0)), unused=i % 2 == 1)
    return w.finish()


def c_header_shapes(rng):
    """dynamic headers: one distance code of one bit, no distance code, HLIT / HDIST / HCLEN padded to the full, runs that
    cross from the literal/length lengths into the distance lengths, 258 written both ways"""
    w = Writer(rng)
    w.block([0] + [rng.randrange(256) for _ in range(300)], "dynamic", unused=False, pad_hdist=False)            # no distance code
    w.block([(258, 1), 1, (3, 1), (100, 1)], "dynamic", unused=False, deep=False)                                                # one distance code
    for i in range(6):                                                      # no short distance: the distance lengths begin with zeros
        t = [(100 + i, 300 - i), rng.randrange(200)] * 20 + [(7, 290)]
        w.block(t, "dynamic", unused=False, deep=False, pad_hlit=True, pad_hdist=bool(i & 1), pad_hclen=bool(i & 2), rle=("greedy", "random")[i % 2])
    t = list(range(255))                                                    # 256 codes of 8 bits: the code-length code needs 8 and 0 only
    rng.shuffle(t)
    w.block(t, "dynamic", power=0.0, deep=False, unused=False, pad_hlit=False, pad_hdist=False, pad_hclen=False, rle="greedy")
    for hclen_pad in (False, True):
        w.block(random_tokens(rng, len(w.data), 3000, None, 0.5, 4), "dynamic", unused=True, pad_hlit=True, pad_hdist=True, pad_hclen=hclen_pad)
    w.block([(258, 258, True), (258, 259, False), 3], "fixed", last=True)
    return w.finish()


CONSTRUCTIONS = {
    "overlaps": c_overlaps, "ring_wraps": c_ring_wraps, "flush_thresholds": c_flush_thresholds, "across_blocks": c_across_blocks,
    "stored_bit_offsets": c_stored_bit_offsets, "input_boundaries": c_input_boundaries, "deep_codes": c_deep_codes,
    "header_shapes": c_header_shapes,
}
CONSTRUCTIONS.update({"final_padding_%d" % p: functools.partial(c_final_padding, pad=p) for p in range(8)})
CONSTRUCTIONS.update({"empty_last_%s" % k: functools.partial(c_empty_blocks, last_kind=k) for k in ("stored", "fixed", "dynamic")})

RANDOM_SIZES = (45000, 70000, 131072, 98304 + 17, 66000, 131071, 41000, 120000)
N_RANDOM = 64
# (colour type, depth, width, height, interlaced): the filtered streams of real images, re-encoded
IMAGES = {"image_rgba8": (6, 8, 37, 65, False), "image_rgb16_adam7": (2, 16, 37, 65, True), "image_palette4": (3, 4, 300, 140, False),
          "image_gray1_adam7": (0, 1, 300, 140, True), "image_gray_alpha8": (4, 8, 300, 140, False)}


def names():
    return sorted(CONSTRUCTIONS) + ["random_%02d" % i for i in range(N_RANDOM)] + sorted(IMAGES)


def _seed(name):
    return zlib.crc32(name.encode())


def image_samples(name):
    """-> (samples, palette or None): smooth ramps with a little noise, the kind of rows whose filtered bytes repeat"""
    ct, depth, w, h, _ = IMAGES[name]
    rng = np.random.default_rng(_seed(name))
    s = O.random_samples(rng, w, h, ct, depth, smooth=True)
    if depth < 8:
        yy, xx = np.mgrid[0:h, 0:w]
        s = (((xx // 7 + yy // 5)[..., None] + (rng.integers(0, 100, (h, w, 1)) == 0)) % (1 << depth)).astype(np.uint32)
    return s, (rng.integers(0, 256, (1 << depth, 3), dtype=np.uint8) if ct == 3 else None)


@functools.lru_cache(maxsize=None)
def entry(name):
    """-> (data, zlib stream, stats) of a corpus stream"""
    rng = random.Random(_seed(name))
    if name in CONSTRUCTIONS:
        out = CONSTRUCTIONS[name](rng)
    elif name in IMAGES:
        ct, depth, w, h, inter = IMAGES[name]
        data = O.filtered_stream(image_samples(name)[0], ct, depth, [4, 0, 3, 1, 2, 4, 4, 3, 1], inter)
        z, stats = reencode(data, rng)
        out = data, z, stats
    else:
        out = random_stream(rng, RANDOM_SIZES[int(name[-2:]) % len(RANDOM_SIZES)])
    assert 2 <= len(out[0]) <= 131072 and (name in IMAGES or out[0][0] == 0)
    return out


def gray_row_file(z, n):
    """a PNG of one gray-8 row whose image data is n bytes (the filter byte and n - 1 pixels), with `z` as its IDAT stream"""
    return O.write_png(np.zeros((1, n - 1, 1), np.uint32), 0, 8, z=z)


def image_file(name):
    ct, depth, w, h, inter = IMAGES[name]
    s, palette = image_samples(name)
    return O.write_png(s, ct, depth, interlace=inter, palette=palette, z=entry(name)[1])


# ---- damaged streams: by rule, not by chance -----------------------------------------------------------------------------------------
def _one_dynamic_block(rng, **opt):
    w = Writer(rng)
    w.block(random_tokens(rng, 0, 4000, None, 0.3, 64), "dynamic", last=True, unused=False, deep=False, rle="random", **opt)
    return w.finish()


def _shorten_longest(lens):
    s = max(range(len(lens)), key=lambda i: (lens[i], i))
    assert lens[s] >= 2
    lens[s] -= 1


def _lengthen_shortest(lens):
    s = min((i for i in range(len(lens)) if lens[i]), key=lambda i: (lens[i], i))
    lens[s] += 1


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> (stream, cap, the status it must give): every refusal that a dynamic header can meet in png_build_huff and in the
    length loop, each made by ONE edit of a generator block that inflates without it; and corpus streams cut at token boundaries"""
    edits = {
        "oversubscribed_literal_length_set": dict(edit_lens=lambda ll, d: _shorten_longest(ll)),
        "incomplete_literal_length_set": dict(edit_lens=lambda ll, d: _lengthen_shortest(ll)),
        "oversubscribed_distance_set": dict(edit_lens=lambda ll, d: _shorten_longest(d)),
        "incomplete_distance_set": dict(edit_lens=lambda ll, d: _lengthen_shortest(d)),
        "oversubscribed_code_length_set": dict(edit_cl=_shorten_longest),
        "incomplete_code_length_set": dict(edit_cl=_lengthen_shortest),
        "repeat_with_nothing_before_it": dict(edit_items=lambda items: items.insert(0, (16, 0, 2))),
        "run_past_hlit_plus_hdist": dict(edit_items=lambda items: items.__setitem__(-1, (18, 127, 7))),
        "missing_end_of_block_code": dict(edit_lens=lambda ll, d: ll.__setitem__(256, 0)),
        "hlit_287": dict(hlit_field=30),
        "hdist_31": dict(hdist_field=30),
    }
    out = {}
    data, z, _ = _one_dynamic_block(random.Random(5))
    assert zlib.decompress(z) == data                                       # the block that the edits start from is a good one
    for name, opt in edits.items():
        bad = _one_dynamic_block(random.Random(5), **opt)[1]
        assert bad != z
        out[name] = (bad, len(data), CODE_LENGTHS)
    for name in ("random_03", "deep_codes", "stored_bit_offsets"):
        data, z, stats = entry(name)
        cuts = sorted(set(b // 8 for b in stats["cuts"] if 2 < b // 8 < len(z) - 4))
        for k in (0, len(cuts) // 2, len(cuts) - 1):
            out["%s_cut_at_%d" % (name, cuts[k])] = (z[:cuts[k]], len(data), TRUNCATED)
    return out


# ---- surplus data: the same stream under an IHDR that needs less -------------------------------------------------------------------
SURPLUS = ("random_05", "ring_wraps", "stored_bit_offsets", "flush_thresholds")


def surplus_caps(name):
    data, z, stats = entry(name)
    caps = [len(data) - 1, len(data) // 2]
    caps += [c for c in (stats["inside_match"], stats["inside_stored"]) if c is not None and c >= 2]
    return caps


def wrong_adler(name):
    """-> (stream, data): a good stream with a wrong checksum"""
    data, z, _ = entry(name)
    return z[:-1] + bytes([z[-1] ^ 0x40]), data


def with_filter_byte(z, data):
    """-> (zlib stream, data) with one stored byte 0 in front: any stream becomes one gray-8 row of filter type 0.  The stored block
    ends on a byte boundary, so every bit of the stream's own blocks stays as its encoder wrote it."""
    assert z[0] & 15 == 8 and not z[1] & 0x20
    return z[:2] + b"\x00\x01\x00\xfe\xff\x00" + z[2:-4] + struct.pack(">I", zlib.adler32(b"\0" + data)), b"\0" + data


@functools.lru_cache(maxsize=None)
def zlibs_own_streams():
    """name -> (zlib stream, data): the GOOD streams of tests/test_png_decode_core.py (zlib's encoder at every strategy, this
    project's own coder, the hand-written far distances) as gray-8 rows"""
    from tests.test_png_decode_core import GOOD
    return {name: with_filter_byte(z, data) for name, (data, z) in sorted(GOOD.items()) if len(data) >= 2}


@functools.lru_cache(maxsize=None)
def device_cases():
    """[(name, stream, cap, status)]: everything that tests/test_gpu_png_inflate_streams.py sends to the device, with the status it
    expects there.  tests/test_deflate_gen.py takes this list through the ASan + UBSan build of the emulation first."""
    out = []
    for name in names():
        data, z, _ = entry(name)
        out.append((name, z, len(data), OK))
    for name in SURPLUS:
        for cap in surplus_caps(name):
            out.append(("%s under %d" % (name, cap), entry(name)[1], cap, OK))
    z, data = wrong_adler("random_05")
    out.append(("wrong adler, exact size", z, len(data), ADLER))
    out.append(("wrong adler, one surplus byte", z, len(data) - 1, OK))
    for name, (z, cap, status) in sorted(damaged().items()):
        out.append((name, z, cap, status))
    for name, (z, data) in zlibs_own_streams().items():
        out.append(("zlib's own: " + name, z, len(data), OK))
    return out
