"""A seeded writer of legal baseline JPEG files (ITU-T T.81, sequential Huffman) that no ENCODER writes -- test infrastructure,
and no product code: nothing here is shared with csrc/jpeg_write.cpp, codecs/mozjpeg.py or oracle/jpeg_oracle.c.  The writer
chooses the coefficient planes itself, so the expected result of every decode is known without a second decoder.

What the writer can do that libjpeg's encoder does not: Huffman tables of any legal shape (every code 16 bits long; codes at
every length 10..16; the maximal table whose last code is the 16-bit 1111111111111110; under-subscribed tables; 255 values at
one length and one more, all a DHT's count byte holds), any table id 0..3 per component, tables spread over several DHT /
DQT segments or defined twice (the last definition holds), 16-bit DQT entries, SOF1, any component ids, any restart interval
with 0..3 fill bytes before each RSTn, pad bits of ones, zeros or noise, blocks of 1 665 bits, blocks without an EOB, chains
of ZRLs, a ZRL directly before an EOB.

`stats` records what a file contains, so that coverage is asserted and not hoped for (tests/test_jpeg_gen.py).  1 024 bits
is the decoder's sub-sequence (csrc/jpeg_parse.hpp kSubBits); its restart segments start on that grid, and `seg_first_sub`
follows that rule.

    names() / entry(name)   the corpus: fixed seeds, every file rebuilt from its seed, cached per process
                            entry -> (file bytes, coefficient planes [bh][bw][64] int16 natural order, qt [ncomp][64], stats)
    device_cases()          the names a GPU test may use: set by tests/test_jpeg_gen.py's checks (see there)

Left out on purpose:
  * tables with Kraft sum exactly 1: T.81 forbids the all-ones code and libjpeg refuses such a DHT (jdhuff.c
    jpeg_make_d_derived_tbl, "no code is allowed to be all ones"), so they are not legal streams.  The corpus carries the
    maximal legal tables instead: Kraft sum 1 - 2^-16 (`maximal`), and every code of a length but the all-ones one (`fixed12`);
  * a coefficient whose run carries the zigzag index past 63: libjpeg stores it at index 63 without an error, the device
    decoder reports the file as corrupt -- the expected result is undecided, nothing of the kind goes to a GPU.  (A ZRL that
    carries the index past 63 just ends the block in all three decoders and is in the corpus: `silent_zrl_past_63`.)
"""
import functools

import numpy as np

SUB_BITS = 1024
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
SAMPLING = {"gray": ((1,), (1,)), "444": ((1, 1, 1), (1, 1, 1)), "422": ((2, 1, 1), (1, 1, 1)),
            "440": ((1, 1, 1), (2, 1, 1)), "420": ((2, 1, 1), (2, 1, 1))}
EOB, ZRL = 0x00, 0xF0

# ---- Huffman tables: (bits[1..16] as a 16-tuple, vals) ----------------------------------------------------------------------
# T.81 Annex K.3 luminance tables
STD_DC = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
STD_AC = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), tuple(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_SYMBOLS = tuple(sorted(STD_AC[1]))                 # EOB, ZRL and every (run, size 1..10)
assert len(AC_SYMBOLS) == 162


def table(lengths):
    """[(symbol, code length)] -> (bits, vals); symbols of one length keep their order"""
    bits = [0] * 17
    for _, l in lengths:
        bits[l] += 1
    vals = [s for l in range(1, 17) for s, k in lengths if k == l]
    kraft = sum(bits[l] << (16 - l) for l in range(1, 17))
    assert kraft < 1 << 16 and len(vals) <= 256, "not a legal JPEG table (the all-ones code is reserved)"
    return tuple(bits[1:]), tuple(vals)


def all16(vals):
    return table([(s, 16) for s in vals])


def rotated(vals, k):
    vals = list(vals)
    return vals[k % len(vals):] + vals[:k % len(vals)]


def spread(vals):
    """two 2-bit codes, the rest at every length 10..16"""
    vals = list(vals)
    n = len(vals) - 2
    per = [max(1, n // 8)] * 6
    lens = [2, 2] + [10 + i for i, c in enumerate(per) for _ in range(c)]
    lens += [16] * (len(vals) - len(lens))
    return table(list(zip(vals, lens)))


def maximal(vals16):
    """one code of every length 1..16: 0, 10, 110, ... and 1111111111111110 for the LAST symbol; Kraft sum 1 - 2^-16"""
    assert len(vals16) == 16
    return table([(s, i + 1) for i, s in enumerate(vals16)])


def gappy(vals):
    """under-subscribed, with lengths that have no code between lengths that do: 3, 3, then 11 x 7, 13 x 3, 16 for the rest"""
    vals = list(vals)
    lens = ([3, 3] + [11] * 7 + [13] * 3 + [16] * 256)[:len(vals)]
    return table(list(zip(vals, lens)))


def flat(vals, length):
    """every value at one length -- but a DHT counts the codes of a length in ONE byte: the 256th value gets the next length"""
    vals = list(vals)
    return table([(s, length) for s in vals[:255]] + [(s, length + 1) for s in vals[255:]])


DC12 = tuple(range(12))
# every symbol 12 bits long with its magnitude bits: DC category c behind a (12 - c)-bit code, AC (run r, size 8) behind 4 bits
FIXED12_DC = table(sorted(((c, 12 - c) for c in range(12)), key=lambda t: t[1]))
FIXED12_AC = flat([(r << 4) | 8 for r in range(15)], 4)
AC256 = tuple(AC_SYMBOLS) + tuple(s for s in range(256) if s not in AC_SYMBOLS)     # the 162 real symbols, then filler


def codes_of(tab):
    """symbol -> (code, length), canonical (T.81 Annex C)"""
    bits, vals = tab
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


# ---- the scan ------------------------------------------------------------------------------------------------------------
class _Segment:
    """bits of one restart segment, high bit first, through an integer accumulator that is spilled every 4 096 bits"""
    def __init__(self):
        self.out, self.acc, self.n, self.pos = bytearray(), 0, 0, 0

    def put(self, value, bits):
        self.acc = (self.acc << bits) | value
        self.n += bits
        self.pos += bits
        if self.n >= 4096:
            k = self.n & 7
            self.out += (self.acc >> k).to_bytes(self.n >> 3, "big")
            self.acc &= (1 << k) - 1
            self.n = k

    def close(self, pad, rng):
        k = -self.n & 7
        if k:
            fill = {"ones": (1 << k) - 1, "zeros": 0}.get(pad)
            self.put(int(rng.integers(0, 1 << k)) if fill is None else fill, k)
            self.pos -= k
        self.out += self.acc.to_bytes(self.n >> 3, "big")
        return bytes(self.out)


def _encode_block(zz, pred, dc, ac, seg, st, zrl_tail):
    """one block (zigzag order, python ints) into seg; zrl_tail: ZRLs written between the last coefficient and the EOB
    (-1: as many as it takes to carry the index past 63, and no EOB -- libjpeg's silent case)"""
    acc, n = 0, 0
    diff = zz[0] - pred
    cat = abs(diff).bit_length()
    code, l = dc[cat]
    st["longest_code"] = max(st["longest_code"], l)
    st["long_symbols"] += l > 9
    acc, n = (code << cat) | (diff if diff >= 0 else diff + (1 << cat) - 1), l + cat
    k = 0                                                     # zigzag index of the last coefficient written
    for i in [i for i in range(1, 64) if zz[i]]:
        run = i - k - 1
        while run >= 16:
            code, l = ac[ZRL]
            acc, n = (acc << l) | code, n + l
            st["longest_code"] = max(st["longest_code"], l)
            st["long_symbols"] += l > 9
            st["zrl"] += 1
            run -= 16
        v = zz[i]
        size = abs(v).bit_length()
        code, l = ac[(run << 4) | size]
        acc, n = (((acc << l) | code) << size) | (v if v >= 0 else v + (1 << size) - 1), n + l + size
        st["longest_code"] = max(st["longest_code"], l)
        st["long_symbols"] += l > 9
        k = i
    if k < 63:
        code, l = ac[ZRL]
        extra = zrl_tail if zrl_tail >= 0 else (63 - k + 15) // 16
        if zrl_tail >= 0:
            extra = min(extra, (62 - k) // 16)                # the index stays at or below 63: another symbol follows
        for _ in range(extra):
            acc, n = (acc << l) | code, n + l
            st["long_symbols"] += l > 9
            st["zrl"] += 1
        if extra:
            st["longest_code"] = max(st["longest_code"], l)
        if zrl_tail >= 0:
            code, l = ac[EOB]
            acc, n = (acc << l) | code, n + l
            st["longest_code"] = max(st["longest_code"], l)
            st["long_symbols"] += l > 9
            st["zrl_before_eob"] += extra > 0
            st["dc_and_eob_blocks"] += k == 0 and extra == 0
        else:
            st["zrl_past_63"] += 1
    else:
        st["blocks_without_eob"] += 1
    seg.put(acc, n)
    st["longest_block"] = max(st["longest_block"], n)


def encode_scan(planes, hs, vs, mcus_w, mcus_h, dc_codes, ac_codes, ri, fill, pad, rng, zrl_tails=None):
    """-> (entropy-coded bytes behind the SOS header, stats).  planes[c]: [bh][bw][64] natural order; dc_codes / ac_codes: per
    component; ri: restart interval in MCUs (0: none); fill: None or (lo, hi) 0xFF fill bytes before each RSTn; zrl_tails: None
    or a function block number -> zrl_tail of _encode_block."""
    st = dict(longest_code=0, long_symbols=0, longest_block=0, zrl=0, zrl_before_eob=0, zrl_past_63=0, blocks_without_eob=0, dc_and_eob_blocks=0,
              blocks=0, block_starts=[], seg_bits=[], fill_bytes=0, stuffed=0)
    zz = [p[..., ZIGZAG].astype(np.int64) for p in planes]
    order = [(c, dy, dx) for c in range(len(planes)) for dy in range(vs[c]) for dx in range(hs[c])]
    out = bytearray()
    total = mcus_w * mcus_h
    per = ri if ri else total
    n_rst = 0
    for m0 in range(0, total, per):
        seg, starts, pred = _Segment(), [], [0] * len(planes)
        for m in range(m0, min(m0 + per, total)):
            my, mx = divmod(m, mcus_w)
            for c, dy, dx in order:
                blk = zz[c][my * vs[c] + dy, mx * hs[c] + dx].tolist()
                starts.append(seg.pos)
                _encode_block(blk, pred[c], dc_codes[c], ac_codes[c], seg, st, zrl_tails(st["blocks"]) if zrl_tails else 0)
                pred[c] = blk[0]
                st["blocks"] += 1
        st["seg_bits"].append(seg.pos)
        st["block_starts"].append(starts)
        raw = seg.close(pad, rng)
        st["stuffed"] += raw.count(b"\xff")
        out += raw.replace(b"\xff", b"\xff\x00")
        if m0 + per < total:
            k = int(rng.integers(fill[0], fill[1] + 1)) if fill else 0
            st["fill_bytes"] += k
            out += b"\xff" * k + bytes([0xFF, 0xD0 + (n_rst & 7)])
            n_rst += 1
    # the decoder's layout: every segment starts on a sub-sequence boundary and takes at least one
    first, firsts, empty = 0, [], []
    for bits, starts in zip(st["seg_bits"], st["block_starts"]):
        n_sub = max(1, -(-(8 * -(-bits // 8)) // SUB_BITS))
        firsts.append(first)
        empty.append(n_sub - len({s // SUB_BITS for s in starts}))
        first += n_sub
    st.update(seg_first_sub=firsts, n_sub=first, subs_without_block_start=empty, segments=len(firsts))
    return bytes(out), st


def straddles(st, sub):
    """does a block start in front of bit sub * 1 024 of the whole scan (the decoder's layout) and end behind it?"""
    for first, bits, starts in zip(st["seg_first_sub"], st["seg_bits"], st["block_starts"]):
        at = (sub - first) * SUB_BITS
        if 0 < at < bits:
            return all(s != at for s in starts)
    return False


# ---- the file ------------------------------------------------------------------------------------------------------------
def _marker(m, payload):
    return bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, "big") + payload


def _dqt(tid, q, wide):
    zq = np.asarray(q)[ZIGZAG]
    return bytes([(16 if wide else 0) | tid]) + (zq.astype(">u2").tobytes() if wide else zq.astype(np.uint8).tobytes())


def _dht(tc, th, tab):
    return bytes([(tc << 4) | th]) + bytes(tab[0]) + bytes(tab[1])


def write_file(width, height, sampling, planes, qts, tq, dht, td, ta, rng, ri=0, fill=None, pad="ones", sof=0xC0, comp_ids=None,
               split_tables=False, decoys=(), decoy_qts=None, wide_qt=(), tail=b"\xff\xd9", zrl_tails=None):
    """qts: {id: [64] natural order}; dht: {(class, id): table}; decoys: [(class, id, table)] written in front of the real
    definitions; wide_qt: quantisation table ids written with 16-bit entries; tail: what follows the scan"""
    hs, vs = SAMPLING[sampling]
    n = len(hs)
    comp_ids = comp_ids or tuple(range(1, n + 1))
    mcus_w, mcus_h = -(-width // (8 * max(hs))), -(-height // (8 * max(vs)))
    for c in range(n):
        assert planes[c].shape == (mcus_h * vs[c], mcus_w * hs[c], 64), (planes[c].shape, c)
    out = bytearray(b"\xff\xd8")
    dq = [_dqt(t, q, False) for t, q in sorted((decoy_qts or {}).items())]
    dq += [_dqt(t, q, t in wide_qt or max(q) > 255) for t, q in sorted(qts.items())]
    out += b"".join(_marker(0xDB, p) for p in dq) if split_tables else _marker(0xDB, b"".join(dq))
    out += _marker(sof, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([n])
                   + b"".join(bytes([comp_ids[c], (hs[c] << 4) | vs[c], tq[c]]) for c in range(n)))
    dh = [_dht(tc, th, tab) for tc, th, tab in decoys] + [_dht(tc, th, tab) for (tc, th), tab in sorted(dht.items())]
    out += b"".join(_marker(0xC4, p) for p in dh) if split_tables else _marker(0xC4, b"".join(dh))
    if ri:
        out += _marker(0xDD, ri.to_bytes(2, "big"))
    out += _marker(0xDA, bytes([n]) + b"".join(bytes([comp_ids[c], (td[c] << 4) | ta[c]]) for c in range(n)) + bytes([0, 63, 0]))
    dc_codes = [codes_of(dht[(0, td[c])]) for c in range(n)]
    ac_codes = [codes_of(dht[(1, ta[c])]) for c in range(n)]
    scan, st = encode_scan(planes, hs, vs, mcus_w, mcus_h, dc_codes, ac_codes, ri, fill, pad, rng, zrl_tails)
    st.update(sampling=sampling, ri=ri, mcus=mcus_w * mcus_h, mcus_w=mcus_w, pad=pad, sof=sof, tail=tail)
    return bytes(out) + scan + tail, st


# ---- coefficient planes ----------------------------------------------------------------------------------------------------
def plane_shapes(width, height, sampling):
    hs, vs = SAMPLING[sampling]
    mw, mh = -(-width // (8 * max(hs))), -(-height // (8 * max(vs)))
    return [(mh * vs[c], mw * hs[c]) for c in range(len(hs))]


def _long_block(rng, amp_lo=512):
    """63 AC coefficients of +-amp_lo..1023 (category 10 at 512): with 16-bit codes 16 + 11 + 63 x 26 = 1 665 bits"""
    b = rng.integers(amp_lo, 1024, 64) * rng.choice([-1, 1], 64)
    b[0] = 0
    return b


def make_planes(width, height, sampling, style, rng):
    """style: small (in range for the pixel stage), long, mixed, tiny, limits, fixed12"""
    planes = []
    for bh, bw in plane_shapes(width, height, sampling):
        p = np.zeros((bh, bw, 64), np.int64)
        nb = bh * bw
        flat = p.reshape(nb, 64)                              # zigzag order while it is filled
        if style == "small":
            flat[:, 0] = rng.integers(-60, 61, nb)
            for b in range(nb):
                k = int(rng.integers(0, 7))
                flat[b, rng.integers(1, 64, k)] = rng.integers(-6, 7, k)
        elif style == "tiny":
            flat[:, 0] = 5                                     # every difference behind the first is 0: DC code + EOB
        elif style == "long":
            for b in range(nb):
                flat[b] = _long_block(rng)
            flat[:, 0] = np.where(np.arange(nb) % 2 == 0, 1000, -1000)          # differences of +-2 000: category 11
        elif style == "limits":
            for b in range(nb):
                flat[b] = _long_block(rng, 1)
                flat[b, rng.integers(1, 64, 8)] = rng.choice([-1023, 1023, -512, 512, 1, -1], 8)
            flat[:, 0] = np.where(np.arange(nb) % 2 == 0, 1023, -1024)           # differences of +-2 047
        elif style == "mixed":
            dc = 0
            for b in range(nb):
                kind = int(rng.integers(0, 7))
                if kind <= 1:
                    flat[b] = _long_block(rng)
                elif kind == 2:                                                   # DC and EOB only, the difference 0 or small
                    pass
                elif kind == 3:                                                   # no EOB: coefficient 63 is there
                    flat[b, 63] = rng.integers(1, 1024)
                    flat[b, rng.integers(1, 63, 3)] = rng.integers(-1023, 1024, 3)
                elif kind == 4:                                                   # three ZRLs in a row (run of 48..61 zeros)
                    flat[b, 1] = -3
                    flat[b, int(rng.integers(50, 64))] = rng.integers(1, 1024)
                elif kind == 5:                                                   # ends early: room for ZRLs before the EOB
                    flat[b, 1:int(rng.integers(2, 14))] = rng.integers(1, 1024)
                else:                                                             # ZRL chain to the very last coefficient
                    flat[b, 63] = -1
                dc = int(rng.integers(-1000, 1001)) if kind != 2 or rng.integers(0, 2) else dc
                flat[b, 0] = dc
        elif style == "fixed12":
            # every AC symbol is (run 0, size 8): nibbles of the magnitude bits never 1111, so a decoder that is 4 or 8 bits
            # off the 12-bit symbol grid never meets the one pattern that is no code and stays off the grid
            hi = rng.integers(0, 15, (nb, 64))
            lo = rng.integers(0, 15, (nb, 64))
            raw = hi * 16 + lo                                                    # the 8 magnitude bits as written
            flat[:] = np.where(raw >= 128, raw, raw - 255)
            flat[:, 0] = np.where(np.arange(nb) % 2 == 0, 750, -750)              # +-1 500: "0" + 11 bits without a 1111 nibble
            flat[0, 1] = 0                                                        # block 0 is one symbol short: no later block starts
                                                                                  # on a sub-sequence boundary (756 + 768 k != 1 024 t)
        else:
            raise ValueError(style)
        nat = np.zeros_like(p).reshape(nb, 64)
        nat[:, ZIGZAG] = flat
        planes.append(nat.reshape(bh, bw, 64).astype(np.int16))
    return planes


# ---- the corpus ------------------------------------------------------------------------------------------------------------
Q1 = [1] * 64
Q_SMALL = [2 + (i % 3) for i in range(64)]
Q_WIDE = [0] * 64                                             # 256..969 in the upper half of the zigzag: only a 16-bit DQT holds them
for _i in range(64):
    Q_WIDE[int(ZIGZAG[_i])] = 3 if _i < 32 else 256 + 23 * (_i - 32)


def _tables(kind, n=3):
    """-> dht dict for table ids 0..n-1 of one kind"""
    d = {}
    for t in range(n):
        if kind == "std":
            d[(0, t)], d[(1, t)] = STD_DC, STD_AC
        elif kind == "all16":                                  # six different tables: the symbol order is rotated per id
            d[(0, t)], d[(1, t)] = all16(rotated(DC12, 5 * t)), all16(rotated(AC_SYMBOLS, 37 * t))
        elif kind == "spread":
            d[(0, t)], d[(1, t)] = spread(rotated(DC12, 3 * t)), spread(rotated(AC_SYMBOLS, 11 * t + 1))
        elif kind == "gappy":
            d[(0, t)], d[(1, t)] = gappy(rotated(DC12, t)), gappy(rotated(AC_SYMBOLS, 5 * t))
        elif kind == "flat256":
            d[(0, t)], d[(1, t)] = all16(DC12), flat(rotated(AC256, 3 * t), 10)
        elif kind == "ac256x16":
            d[(0, t)], d[(1, t)] = all16(DC12), table([(s, 16 if i else 15) for i, s in enumerate(rotated(AC256, 100 + t))])
        else:
            raise ValueError(kind)
    return d


# name -> parameters.  style / tables / geometry as above; `in_range`: the pixel stage stays inside 0..255 (small amplitudes),
# so libjpeg's pixels are comparable; everything else is checked coefficient for coefficient only.
def _corpus():
    C = {}

    def add(name, w, h, sampling, style, tables, seed, **kw):
        assert name not in C
        C[name] = dict(w=w, h=h, sampling=sampling, style=style, tables=tables, seed=seed, **kw)

    # a. long codes -- and, for reference, the standard tables through this writer
    for s, (w, h) in (("gray", (40, 24)), ("444", (33, 17)), ("422", (40, 24)), ("440", (24, 40)), ("420", (50, 35))):
        add(f"std_{s}", w, h, s, "small", "std", 1, in_range=True)
        add(f"all16_{s}", w, h, s, "small", "all16", 2, in_range=True, td=(0, 1, 1), ta=(0, 1, 1))
    add("spread_420", 72, 40, "420", "small", "spread", 3, in_range=True, td=(0, 1, 2), ta=(2, 0, 1), sof=0xC1)
    add("spread_limits_gray", 48, 32, "gray", "limits", "spread", 4)
    add("gappy_444", 41, 23, "444", "small", "gappy", 5, in_range=True, td=(0, 1, 0), ta=(1, 0, 1))
    add("flat256_422", 56, 24, "422", "small", "flat256", 6, in_range=True)
    add("ac256x16_gray", 40, 24, "gray", "mixed", "ac256x16", 7)
    add("maximal_gray", 64, 40, "gray", "maximal", "maximal", 8)
    add("limits_all16_gray", 40, 24, "gray", "limits", "all16", 9)
    # b. the second-level pool overflows: 3 x (128 + 2 x 128) entries wanted, 768 there
    add("pool_six_tables_444", 48, 32, "444", "small", "all16", 10, in_range=True, td=(0, 1, 2), ta=(0, 1, 2), sof=0xC1)
    add("pool_six_tables_long_444", 32, 24, "444", "mixed", "all16", 11, td=(0, 1, 2), ta=(0, 1, 2), sof=0xC1)
    add("pool_last_ac_444", 48, 32, "444", "small", "all16", 12, in_range=True, td=(0, 1, 0), ta=(0, 1, 2), sof=0xC1)
    add("mix_std_444", 48, 32, "444", "small", "std", 38, in_range=True)                # the same geometry with other tables:
    add("mix_all16_444", 48, 32, "444", "small", "all16", 39, in_range=True, td=(0, 1, 1), ta=(0, 1, 1))   # for mixed batches
    # c. long blocks
    add("long_gray", 40, 24, "gray", "long", "all16", 13)
    add("mixed_gray", 96, 64, "gray", "mixed", "all16", 14, zrl_tail=True)
    add("mixed_420", 48, 32, "420", "mixed", "all16", 15, td=(0, 1, 1), ta=(0, 1, 1), zrl_tail=True, pad="random")
    add("mixed_spread_444", 40, 24, "444", "mixed", "spread", 16, td=(0, 1, 2), ta=(0, 1, 2), sof=0xC1, zrl_tail=True, pad="zeros")
    # d. the write pass's chunk of 512 sub-sequences and a synchronisation workgroup's own 1 008
    add("bound_512_gray", 208, 208, "gray", "long", "all16", 17)
    add("bound_1008_gray", 208, 208, "gray", "mixed_long", "all16", 18)
    add("bound_restart_gray", 208, 208, "gray", "long", "all16", 19, ri=5, fill=(0, 3))
    add("bound_restart_mixed_gray", 208, 208, "gray", "mixed_long", "all16", 121, ri=9, pad="random")
    # e. a decoder off the symbol grid stays off it
    add("slow_sync_gray", 184, 184, "gray", "fixed12", "fixed12", 21)
    # f. restart variety
    add("ri1_long_420", 48, 32, "420", "long", "all16", 22, ri=1, fill=(0, 3), td=(0, 1, 1), ta=(0, 1, 1))
    add("ri1_fill3_long_gray", 40, 24, "gray", "long", "all16", 23, ri=1, fill=(3, 3))
    add("ri1_tiny_gray", 160, 128, "gray", "tiny", "std", 24, ri=1, in_range=True)
    add("ri1_tiny_444", 88, 64, "444", "tiny", "all16", 25, ri=1, in_range=True, fill=(0, 2), pad="zeros")
    add("ri7_of_5_wide_420", 80, 48, "420", "small", "spread", 26, ri=7, in_range=True, td=(0, 1, 1), ta=(0, 1, 1))
    add("ri7_of_5_wide_long_422", 80, 24, "422", "mixed", "all16", 27, ri=7, fill=(1, 2), zrl_tail=True)
    add("ri60000_440", 24, 40, "440", "small", "gappy", 28, ri=60000, in_range=True)
    add("ri4_random_pad_gray", 40, 24, "gray", "long", "all16", 29, ri=4, pad="random")
    # g. header variety
    add("sof1_ids23_420", 34, 18, "420", "small", "std4", 30, in_range=True, sof=0xC1, td=(2, 3, 3), ta=(3, 2, 2), tq=(2, 3, 3))
    add("wide_dqt_444", 24, 16, "444", "small_lowfreq", "std", 31, in_range=True, qt="wide", tq=(0, 1, 1))
    add("comp_ids_012_444", 24, 16, "444", "small", "all16", 32, in_range=True, comp_ids=(0, 1, 2))
    add("comp_ids_102030_420", 40, 24, "420", "small", "spread", 33, in_range=True, comp_ids=(10, 20, 30), split_tables=True)
    add("junk_after_eoi_gray", 40, 24, "gray", "small", "all16", 34, in_range=True, tail=b"\xff\xd9" + bytes(range(200, 256)) * 3)
    add("no_eoi_422", 40, 24, "422", "small", "gappy", 35, in_range=True, tail=b"")
    add("redefined_tables_444", 40, 24, "444", "small", "all16", 36, in_range=True, decoy=True, split_tables=True,
        td=(0, 1, 1), ta=(0, 1, 1))
    # h. outside the standard, decoded by libjpeg without a word: a ZRL that carries the index past 63 ends the block
    add("silent_zrl_past_63_gray", 40, 24, "gray", "small", "all16", 37, in_range=True, zrl_tail=-1)
    return C


CORPUS = _corpus()


def names():
    return list(CORPUS)


@functools.lru_cache(maxsize=None)
def entry(name):
    """-> (file bytes, planes, qt [ncomp][64] uint16 natural order, stats)"""
    p = dict(CORPUS[name])
    rng = np.random.default_rng(p["seed"])
    sampling, w, h = p["sampling"], p["w"], p["h"]
    n = len(SAMPLING[sampling][0])
    style, kind = p["style"], p["tables"]
    if style == "maximal":
        # 16 AC symbols: EOB, ZRL, (0, size 1..10), (1, 1), (1, 2), (2, 1), (3, 1); 1111111111111110 belongs to (0, 1), the commonest
        planes = make_planes(w, h, sampling, "small", rng)
        dht = {(0, 0): table([(c, c + 1) for c in range(11)] + [(11, 16)]),
               (1, 0): maximal([EOB, 0x02, 0x03, 0x11, 0x21, ZRL, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0x31, 0x12, 0x01])}
        for pl in planes:                                       # coefficients 1..5 only, coefficient 1 of every size, DC steps of +-2 047
            z = pl[..., ZIGZAG]
            z[..., 6:] = 0
            z[..., 1:6] = rng.integers(-3, 4, z[..., 1:6].shape) * (rng.integers(0, 3, z[..., 1:6].shape) > 0)
            z[..., 1] = rng.choice([1, -1, 1, -1, 2, 5, -9, 17, -40, 100, -300, 600, -1023], z[..., 1].shape)
            z[..., 0] = np.cumsum(np.resize([2047, -2047, 1, 0, 300, -301], z[..., 0].size)).reshape(z[..., 0].shape) - 1024
            for b in z.reshape(-1, 64):                         # (run, size) pairs the table has: (0, s), (1, 1), (1, 2), (2, 1), (3, 1)
                run = 0
                for i in range(1, 6):
                    if b[i] == 0:
                        run += 1
                        continue
                    size = abs(int(b[i])).bit_length()
                    if run and (run, size) not in ((1, 1), (1, 2), (2, 1), (3, 1)):
                        b[i - run:i] = 1
                    run = 0
            pl[..., ZIGZAG] = z
    else:
        base = {"mixed_long": "mixed", "small_lowfreq": "small"}.get(style, style)
        planes = make_planes(w, h, sampling, base, rng)
        if style == "mixed_long":                               # mostly long blocks, some of a handful of bits between them
            for pl in planes:
                flat = pl.reshape(-1, 64)
                for b in np.flatnonzero(rng.integers(0, 16, len(flat)) > 0):
                    z = _long_block(rng)
                    z[0] = flat[b, 0]
                    flat[b, ZIGZAG] = z
        if style == "small_lowfreq":
            for pl in planes:
                z = pl[..., ZIGZAG]
                z[..., 32:] = 0
                pl[..., ZIGZAG] = z
        if kind == "fixed12":
            dht = {(0, 0): FIXED12_DC, (1, 0): FIXED12_AC}
        elif kind == "std4":
            dht = {(0, 2): STD_DC, (1, 3): STD_AC, (0, 3): all16(DC12), (1, 2): spread(AC_SYMBOLS)}
        else:
            dht = _tables(kind, 1 if n == 1 else 3)
    td, ta = p.get("td", (0,) * n)[:n], p.get("ta", (0,) * n)[:n]
    tq = p.get("tq", (0, 1, 1))[:n]
    dht = {k: v for k, v in dht.items() if (k[0] == 0 and k[1] in td) or (k[0] == 1 and k[1] in ta)}
    if p.get("qt") == "wide":
        qts = {0: Q_SMALL, 1: Q_WIDE}
    elif p.get("in_range"):
        qts = {t: [1 + ((i + t) % 3) for i in range(64)] for t in set(tq)}
    else:
        qts = {t: Q1 for t in set(tq)}
    decoys = [(tc, th, STD_AC if tc else STD_DC) for (tc, th) in sorted(dht)] if p.get("decoy") else []
    decoy_qts = {t: [9 + t] * 64 for t in qts} if p.get("decoy") else None
    zt = p.get("zrl_tail")
    tails = None
    if zt is True:
        picks = np.random.default_rng(p["seed"] + 1000).integers(0, 4, 1 << 16)
        tails = lambda b: int(picks[b & 0xffff])
    elif zt == -1:
        picks = np.random.default_rng(p["seed"] + 1000).integers(0, 2, 1 << 16)
        tails = lambda b: -int(picks[b & 0xffff])
    data, st = write_file(w, h, sampling, planes, qts, tq, dht, td, ta, rng, ri=p.get("ri", 0), fill=p.get("fill"),
                          pad=p.get("pad", "ones"), sof=p.get("sof", 0xC0), comp_ids=p.get("comp_ids"),
                          split_tables=p.get("split_tables", False), decoys=decoys, decoy_qts=decoy_qts,
                          wide_qt=(1,) if p.get("qt") == "wide" else (), tail=p.get("tail", b"\xff\xd9"), zrl_tails=tails)
    qt = np.array([qts[tq[c]] for c in range(n)], np.uint16)
    st.update(in_range=bool(p.get("in_range")), td=td, ta=ta, tq=tq, tables=kind, width=w, height=h)
    for pl in planes:
        pl.setflags(write=False)
    return data, planes, qt, st


_DEVICE_CASES = None


def device_cases():
    """The entries a GPU test may use: exactly those that tests/test_jpeg_gen.py's per-entry checks accept (the generator's
    planes read back by the serial decoder, libjpeg's pixels where comparable, the host scan report clean).  Evaluated once
    per process; an entry that fails there fails the CPU test and never reaches a device."""
    global _DEVICE_CASES
    if _DEVICE_CASES is None:
        from tests import test_jpeg_gen as T
        _DEVICE_CASES = [n for n in names() if T.accepts(n)]
    return list(_DEVICE_CASES)
