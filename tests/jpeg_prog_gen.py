"""A seeded writer of legal PROGRESSIVE JPEG files (ITU-T T.81 Annex G, Huffman) that no encoder writes -- test infrastructure
in the manner of tests/jpeg_gen.py (whose table helpers it uses), and no product code: nothing here is shared with
csrc/jpeg_write.cpp or csrc/jpeg_progressive_read.cpp.  The writer chooses the coefficients itself and follows its own scan
script, so the expected planes of every decode are known without a second decoder: a coefficient stands at the precision the
last scan that covered its block left it at, and a block no scan covered (the padding of a plane under one-component scans)
stays zero.

What the scripts hold that libjpeg's encoder does not write: one-component DC scans in a three-component file, DC point
transforms up to 3 with chains of refinements, bands of one index and bands cut anywhere, a component with DC only, successive
approximation three deep, restart intervals in all four scan kinds (interval 1 included) with a DRI that changes between
scans, 0..3 fill bytes before each RSTn, pad bits of ones, zeros or noise, tables whose every code is 16 bits long, a table id
redefined in front of every scan, an end-of-band run of 2^14 blocks, and refinement blocks with 63 correction bits.

`stats` records what a file contains, so that coverage is asserted and not hoped for (tests/test_jpeg_prog_gen.py).

    names() / entry(name)   the accepted corpus -> (file bytes, planes [bh][bw][64] int16 natural order, qt [ncomp][64], stats)
    refused() -> {name: bytes}   files the device path's front end must refuse (the host reader decodes or refuses them itself)
    damaged(name, k)        seeded damage inside the scans of a corpus file: k even a byte flip, k odd a cut
"""
import functools

import numpy as np

from tests.jpeg_gen import SAMPLING, ZIGZAG, codes_of, table

STAGE_BITS = 1024 * 32          # csrc/jpeg_progressive_core.hpp kProgStageWords, in bits (asserted by the tests against the library's)


def geometry(w, h, samp):
    hs, vs = SAMPLING[samp]
    hmax, vmax = max(hs), max(vs)
    mw, mh = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    bw = [mw * a for a in hs]
    bh = [mh * a for a in vs]
    wb = [-(-w * a // (8 * hmax)) for a in hs]
    hb = [-(-h * a // (8 * vmax)) for a in vs]
    return dict(hs=hs, vs=vs, mw=mw, mh=mh, bw=bw, bh=bh, wb=wb, hb=hb, ncomp=len(hs))


def nbits(v):
    return int(v).bit_length()


class Bits:
    """a restart interval's bit string"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):
        if n:
            self.acc = (self.acc << n) | (int(v) & ((1 << n) - 1))
            self.n += n

    def bytes(self, pad, rng):
        padn = (-self.n) % 8
        fill = {"ones": (1 << padn) - 1, "zeros": 0, "noise": int(rng.integers(0, 1 << padn)) if padn else 0}[pad]
        acc, n = (self.acc << padn) | fill, self.n + padn
        raw = acc.to_bytes(n // 8, "big") if n else b""
        return raw.replace(b"\xff", b"\xff\x00")


def shaped_table(symbols, shape):
    """a legal table over `symbols` (<= 255): flat (all 8 bits), all16 (every code 16 bits), skew (1, 2, 3 .. 15, then 16)"""
    symbols = sorted(symbols) or [0]
    assert len(symbols) <= 255
    if shape == "all16":
        return table([(s, 16) for s in symbols])
    if shape == "skew":
        return table([(s, min(i + 1, 16)) for i, s in enumerate(symbols)]) if len(symbols) <= 15 else \
            table([(s, i + 2) if i < 7 else (s, 16) for i, s in enumerate(symbols)])
    return table([(s, 8) for s in symbols])


# ---- one scan: tokens per restart interval ------------------------------------------------------------------------------------
class ScanCoder:
    def __init__(self, G, truth, scan, ri, stats):
        self.G, self.truth, self.s, self.ri, self.stats = G, truth, scan, ri, stats
        self.intervals, self.cur = [], []
        self.eobrun, self.be = 0, []              # pending end-of-band run and its buffered correction bits

    def sym(self, cls_slot, s):
        self.cur.append(("s", cls_slot, s))

    def bits(self, v, n):
        if n:
            self.cur.append(("b", v, n))

    def flush_eobrun(self, slot):
        if self.eobrun:
            r = nbits(self.eobrun) - 1
            self.sym(slot, r << 4)
            self.bits(self.eobrun - (1 << r), r)
            st = self.stats
            st["max_eobrun"] = max(st["max_eobrun"], self.eobrun)
            st["eob0"] += self.eobrun == 1
            if self.be:
                st["eobrun_with_corrections"] += 1
            self.eobrun = 0
        for b in self.be:
            self.bits(b, 1)
        self.be = []

    def blocks_of_mcu(self, m):
        """[(scan slot, ci, by, bx)] in coding order"""
        G, comps = self.G, self.s["comps"]
        if len(comps) == 1:
            ci = comps[0]
            return [(0, ci, m // G["wb"][ci], m % G["wb"][ci])]
        my, mx = divmod(m, G["mw"])
        return [(k, ci, my * G["vs"][ci] + dy, mx * G["hs"][ci] + dx) for k, ci in enumerate(comps)
                for dy in range(G["vs"][ci]) for dx in range(G["hs"][ci])]

    def run(self):
        G, s = self.G, self.s
        comps = s["comps"]
        total = G["wb"][comps[0]] * G["hb"][comps[0]] if len(comps) == 1 else G["mw"] * G["mh"]
        Ss, Se, Ah, Al = s["Ss"], s["Se"], s["Ah"], s["Al"]
        pred = {ci: 0 for ci in comps}
        covered = []
        row_w = G["wb"][comps[0]] if len(comps) == 1 else G["mw"]
        for m in range(total):
            if self.ri and m and m % self.ri == 0:
                if self.eobrun:
                    self.stats["eobrun_cut_by_restart"] += 1
                self.flush_eobrun(("ac", s["ta"]))
                self.intervals.append(self.cur)
                self.cur = []
                pred = {ci: 0 for ci in comps}
            if self.eobrun and m % row_w == 0:
                self.stats["eobrun_spans_rows"] += 1
            for slot, ci, by, bx in self.blocks_of_mcu(m):
                blk = self.truth[ci][by, bx]
                covered.append((ci, by, bx))
                if Ss == 0 and Ah == 0:
                    v = int(blk[0]) >> Al
                    d = v - pred[ci]
                    pred[ci] = v
                    n = nbits(abs(d))
                    self.sym(("dc", s["td"][slot]), n)
                    self.bits(d if d >= 0 else d - 1, n)
                elif Ss == 0:
                    self.bits((int(blk[0]) >> Al) & 1, 1)
                elif Ah == 0:
                    self.ac_first(blk, Ss, Se, Al)
                else:
                    self.ac_refine(blk, Ss, Se, Al)
        self.flush_eobrun(("ac", s["ta"]))
        self.intervals.append(self.cur)
        return covered

    def ac_first(self, blk, Ss, Se, Al):
        slot, r = ("ac", self.s["ta"]), 0
        for k in range(Ss, Se + 1):
            v = int(blk[ZIGZAG[k]])
            t = abs(v) >> Al
            if t == 0:
                r += 1
                continue
            self.flush_eobrun(slot)
            while r > 15:
                self.sym(slot, 0xF0)
                r -= 16
            n = nbits(t)
            self.sym(slot, (r << 4) | n)
            self.bits(t if v >= 0 else ~t, n)
            r = 0
        if r > 0:
            self.eobrun += 1
            if self.eobrun == 0x7FFF:
                self.flush_eobrun(slot)

    def ac_refine(self, blk, Ss, Se, Al):
        slot, r, br, st = ("ac", self.s["ta"]), 0, [], self.stats
        absv = [abs(int(blk[ZIGZAG[k]])) >> Al for k in range(64)]
        eob = max([k for k in range(Ss, Se + 1) if absv[k] == 1], default=-1)
        history = sum(1 for k in range(Ss, Se + 1) if absv[k] > 1)
        st["max_corrections_in_block"] = max(st["max_corrections_in_block"], history)
        if eob < 0 and history:
            st["all_correction_blocks"] += 1
            if self.eobrun:
                st["corrections_inside_eobrun"] += 1
        for k in range(Ss, Se + 1):
            t = absv[k]
            if t == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                self.flush_eobrun(slot)
                self.sym(slot, 0xF0)
                r -= 16
                if br:
                    st["zrl_over_history"] += 1
                for b in br:
                    self.bits(b, 1)
                br = []
            if t > 1:
                br.append(t & 1)
                continue
            self.flush_eobrun(slot)
            self.sym(slot, (r << 4) | 1)
            self.bits(0 if blk[ZIGZAG[k]] < 0 else 1, 1)
            for b in br:
                self.bits(b, 1)
            br, r = [], 0
            if k == 63:
                st["new_coefficient_at_63"] += 1
        if r > 0 or br:
            self.eobrun += 1
            self.be += br
            if self.eobrun == 0x7FFF or len(self.be) > 937:
                self.flush_eobrun(slot)


def seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def dht(cls, slot, tab):
    bits, vals = tab
    return seg(0xC4, bytes([(cls << 4) | slot]) + bytes(bits) + bytes(vals))


def new_stats():
    return dict(kinds=set(), intervals=set(), max_eobrun=0, eob0=0, eobrun_with_corrections=0, eobrun_cut_by_restart=0,
                eobrun_spans_rows=0, max_corrections_in_block=0, all_correction_blocks=0, corrections_inside_eobrun=0,
                zrl_over_history=0, new_coefficient_at_63=0, fill_bytes=0, pads=set(), max_code_len=0, min_code_len=16,
                max_stream_bits=0, dri_changes=0, table_redefinitions=0, levels=0, scans=0, dc_only_components=0,
                one_component_dc_in_color=0, max_dc_al=0, refinement_depth=0, single_index_bands=0, first_scans_at_level0=0,
                padded_blocks_coded=0, padded_blocks_skipped=0, restart_kinds=set())


# jcparam.c jpeg_set_quality: the Annex K tables scaled (natural order) -- what ifhip_jpeg_write gives a baseline twin of a file
K_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
QUALITY = 75


def quality_tables(q):
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.array([min(max((v * scale + 50) // 100, 1), 255) for v in t], np.uint16) for t in (K_LUMA, K_CHROMA)]


def truth_planes(G, rng, density, dense_blocks=False, amp=255):
    planes = []
    for c in range(G["ncomp"]):
        p = np.zeros((G["bh"][c], G["bw"][c], 64), np.int16)
        p[:, :, 0] = rng.integers(-900, 900, p.shape[:2])
        mask = rng.random(p.shape) < density
        mask[:, :, 0] = False
        mags = np.where(rng.random(p.shape) < 0.5, rng.integers(1, 4, p.shape), rng.integers(1, amp + 1, p.shape))
        sign = np.where(rng.random(p.shape) < 0.5, -1, 1)
        p[mask] = (mags * sign)[mask].astype(np.int16)
        if dense_blocks:                                   # every AC coefficient of some blocks nonzero at every precision
            flat = p.reshape(-1, 64)
            for b in range(0, flat.shape[0], 3):
                flat[b, 1:] = (rng.integers(8, 64, 63) * np.where(rng.random(63) < 0.5, -1, 1)).astype(np.int16)
        planes.append(p)
    return planes


def write(w, h, samp, scans, seed, density=0.2, dense_blocks=False, truth=None, sof=0xC2, flat=()):
    """scans: dicts comps, Ss, Se, Ah, Al and optionally dri (a DRI in front of the scan), shape, pad, fill, td / ta.
    flat: components whose blocks all hold one DC value and no AC (a component the script gives DC scans only: libjpeg's
    block smoothing, which fills in AC coefficients a file never sent from the DC values around, then predicts zeros)"""
    rng = np.random.default_rng(seed)
    G = geometry(w, h, samp)
    n = G["ncomp"]
    truth = truth if truth is not None else truth_planes(G, rng, density, dense_blocks)
    for c in flat:
        truth[c][:] = 0
        truth[c][:, :, 0] = 37 * (c + 1)
    tabs = quality_tables(QUALITY)
    qt = np.stack([tabs[min(c, 1)] for c in range(n)])
    st = new_stats()
    out = bytearray(b"\xff\xd8")
    for c in range(n):
        out += seg(0xDB, bytes([c]) + bytes(int(qt[c][ZIGZAG[k]]) for k in range(64)))
    sof_body = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([n])
    for c in range(n):
        sof_body += bytes([c + 1, (G["hs"][c] << 4) | G["vs"][c], c])
    out += seg(sof, sof_body)
    expected = [np.zeros_like(p) for p in truth]
    level = [[-1] * 64 for _ in range(n)]
    first_al = {}
    ri, seen_dri = 0, False
    defined = set()
    for s in scans:
        s = dict(s)
        comps = s["comps"]
        s.setdefault("td", [min(ci, 1) for ci in comps])
        s.setdefault("ta", min(comps[0], 1))
        if "dri" in s:
            st["dri_changes"] += seen_dri and s["dri"] != ri
            ri, seen_dri = s["dri"], True
            out += seg(0xDD, ri.to_bytes(2, "big"))
        coder = ScanCoder(G, truth, s, ri, st)
        covered = coder.run()
        kind = ("dc" if s["Ss"] == 0 else "ac") + ("_refine" if s["Ah"] else "_first")
        st["kinds"].add(kind)
        st["scans"] += 1
        if ri:
            st["restart_kinds"].add(kind)
            st["intervals"].add(ri)
        # the tables this scan uses, from the symbols it holds
        used = {}
        for iv in coder.intervals:
            for t in iv:
                if t[0] == "s":
                    used.setdefault(t[1], set()).add(t[2])
        codes = {}
        for key, symbols in sorted(used.items()):
            tab = shaped_table(symbols, s.get("shape", "flat"))
            st["table_redefinitions"] += key in defined
            defined.add(key)
            out += dht(0 if key[0] == "dc" else 1, key[1], tab)
            codes[key] = codes_of(tab)
            for _, l in codes[key].values():
                st["max_code_len"], st["min_code_len"] = max(st["max_code_len"], l), min(st["min_code_len"], l)
        hdr = bytes([len(comps)])
        for k, ci in enumerate(comps):
            hdr += bytes([ci + 1, (s["td"][k] << 4) | s["ta"]])
        hdr += bytes([s["Ss"], s["Se"], (s["Ah"] << 4) | s["Al"]])
        out += seg(0xDA, hdr)
        pad, fill = s.get("pad", "ones"), s.get("fill", 0)
        st["pads"].add(pad)
        for i, iv in enumerate(coder.intervals):
            b = Bits()
            for t in iv:
                if t[0] == "s":
                    b.put(*codes[t[1]][t[2]])
                else:
                    b.put(t[1], t[2])
            st["max_stream_bits"] = max(st["max_stream_bits"], b.n)
            out += b.bytes(pad, rng)
            if i + 1 < len(coder.intervals):
                out += b"\xff" * fill + bytes([0xFF, 0xD0 + (i & 7)])
                st["fill_bytes"] += fill
        # what a decoder holds behind this scan, and the scan's level
        Al = s["Al"]
        lvl = 0
        for ci in comps:
            for z in range(s["Ss"], s["Se"] + 1):
                lvl = max(lvl, level[ci][z] + 1)
        for ci in comps:
            for z in range(s["Ss"], s["Se"] + 1):
                level[ci][z] = lvl
                if s["Ah"] == 0:
                    first_al[(ci, z)] = Al
        st["levels"] = max(st["levels"], lvl + 1)
        st["first_scans_at_level0"] += lvl == 0 and s["Ah"] == 0
        for ci, by, bx in covered:
            src, dst = truth[ci][by, bx], expected[ci][by, bx]
            pad_block = by >= G["hb"][ci] or bx >= G["wb"][ci]
            st["padded_blocks_coded"] += pad_block
            for z in range(s["Ss"], s["Se"] + 1):
                v = int(src[ZIGZAG[z]])
                if z == 0 and s["Ah"]:                        # a DC refinement ORs its bit into whatever the block holds
                    dst[0] = int(dst[0]) | (((v >> Al) & 1) << Al)
                else:
                    dst[ZIGZAG[z]] = (v >> Al) << Al if z == 0 else (1 if v >= 0 else -1) * ((abs(v) >> Al) << Al)
        if len(comps) == 1:
            ci = comps[0]
            st["padded_blocks_skipped"] += G["bw"][ci] * G["bh"][ci] - G["wb"][ci] * G["hb"][ci]
            st["one_component_dc_in_color"] += n == 3 and s["Ss"] == 0 and s["Ah"] == 0
        if s["Ss"] == 0:
            st["max_dc_al"] = max(st["max_dc_al"], Al)
        st["single_index_bands"] += s["Ss"] == s["Se"] and s["Ss"] > 0
    out += b"\xff\xd9"
    st["dc_only_components"] = sum(1 for c in range(n) if all(level[c][z] < 0 for z in range(1, 64)))
    st["refinement_depth"] = max(first_al.values(), default=0)
    return bytes(out), expected, qt, st


# ---- scripts ------------------------------------------------------------------------------------------------------------------
def S(comps, Ss, Se, Ah, Al, **kw):
    return dict(comps=list(comps), Ss=Ss, Se=Se, Ah=Ah, Al=Al, **kw)


def script_like_an_encoder(n):
    if n == 1:
        return [S([0], 0, 0, 0, 1), S([0], 1, 63, 0, 1), S([0], 0, 0, 1, 0), S([0], 1, 63, 1, 0)]
    return [S([0, 1, 2], 0, 0, 0, 1), S([0], 1, 5, 0, 2), S([2], 1, 63, 0, 1), S([1], 1, 63, 0, 1), S([0], 6, 63, 0, 2),
            S([0], 1, 63, 2, 1), S([0, 1, 2], 0, 0, 1, 0), S([2], 1, 63, 1, 0), S([1], 1, 63, 1, 0), S([0], 1, 63, 1, 0)]


def script_no_encoder_writes():
    """one-component DC scans (two first scans of level 0 and more), DC Al 3 refined 3 -> 2 -> 1 -> 0 through interleaved and
    one-component scans, bands of one index, bands cut anywhere, Cr with DC only, the band 3..20 of Y three deep"""
    return [S([0], 0, 0, 0, 3), S([1], 0, 0, 0, 2), S([2], 0, 0, 0, 0),
            S([0], 1, 1, 0, 0), S([0], 2, 2, 0, 1), S([0], 3, 20, 0, 3), S([0], 21, 22, 0, 0), S([0], 23, 63, 0, 1),
            S([1], 1, 9, 0, 0), S([1], 10, 63, 0, 1),
            S([0], 0, 0, 3, 2), S([0, 1], 0, 0, 2, 1), S([0], 3, 20, 3, 2), S([0], 3, 20, 2, 1), S([0], 0, 0, 1, 0),
            S([0], 3, 20, 1, 0), S([0], 2, 2, 1, 0), S([1], 0, 0, 1, 0), S([0], 23, 63, 1, 0), S([1], 10, 63, 1, 0)]


def script_restarts(n):
    """a restart interval in every scan kind, interval 1 included, a DRI that changes between scans and goes back to 0"""
    c = [0, 1, 2][:n]
    sc = [S(c, 0, 0, 0, 1, dri=1, fill=1, pad="noise"), S([0], 1, 63, 0, 1, dri=2, fill=3, pad="zeros"),
          S(c, 0, 0, 1, 0, dri=3, fill=2, pad="noise"), S([0], 1, 63, 1, 0, dri=1, pad="ones", fill=1)]
    if n == 3:
        sc += [S([1], 1, 63, 0, 0, dri=5, pad="noise"), S([2], 1, 63, 0, 1, dri=0), S([2], 1, 63, 1, 0, dri=4, fill=1, pad="zeros")]
    return sc


def with_shape(scans, shape):
    return [dict(s, shape=shape) for s in scans]


def same_slot(scans):
    """every scan's tables in slot 0: the id is redefined in front of every scan"""
    return [dict(s, td=[0] * len(s["comps"]), ta=0) for s in scans]


CORPUS = {}


def _add(name, *a, **kw):
    CORPUS[name] = (a, kw)


_add("gray_8x8", 8, 8, "gray", script_like_an_encoder(1), 1, density=0.4)
_add("mcu_16x16_420", 16, 16, "420", script_like_an_encoder(3), 2, density=0.3)
for _i, _samp in enumerate(("420", "422", "440", "444")):
    _add("enc_24x24_%s" % _samp, 24, 24, _samp, script_like_an_encoder(3), 10 + _i, density=0.25)
    _add("odd_17x9_%s" % _samp, 17, 9, _samp, same_slot(script_no_encoder_writes()), 20 + _i, density=0.3, flat=(2,))
    _add("odd_24x24_%s" % _samp, 24, 24, _samp, with_shape(script_no_encoder_writes(), "skew"), 30 + _i, density=0.15, flat=(2,))
    _add("restarts_17x9_%s" % _samp, 17, 9, _samp, script_restarts(3), 40 + _i, density=0.3)
_add("restarts_gray_40x24", 40, 24, "gray", script_restarts(1), 50, density=0.05)
_add("all16_24x24_420", 24, 24, "420", with_shape(same_slot(script_like_an_encoder(3)), "all16"), 60, density=0.3)
_add("all16_restarts_17x9_444", 17, 9, "444", with_shape(script_restarts(3), "all16"), 61, density=0.4)
_add("dense_refine_64x48_444", 64, 48, "444", script_like_an_encoder(3), 70, density=0.08, dense_blocks=True)
_add("dense_refine_restarts_32x16_gray", 32, 16, "gray", script_restarts(1), 71, density=0.1, dense_blocks=True)
_add("sparse_rows_64x48_gray", 64, 48, "gray", script_like_an_encoder(1), 72, density=0.004)
_add("long_stream_64x48_444", 64, 48, "444", with_shape(script_like_an_encoder(3), "all16"), 73, density=0.9)


def _eob_big():
    G = geometry(1024, 1024, "gray")
    truth = [np.zeros((G["bh"][0], G["bw"][0], 64), np.int16)]
    truth[0][:, :, 0] = 64
    return write(1024, 1024, "gray", [S([0], 0, 0, 0, 0), S([0], 1, 63, 0, 0)], 80, truth=truth)


@functools.lru_cache(maxsize=None)
def entry(name):
    if name == "eob_run_1024x1024_gray":
        return _eob_big()
    a, kw = CORPUS[name]
    return write(*a, **kw)


def names(big=True):
    return sorted(CORPUS) + (["eob_run_1024x1024_gray"] if big else [])


@functools.lru_cache(maxsize=None)
def refused():
    """files the front end must refuse; the first three are what libjpeg decodes with JWRN_BOGUS_PROGRESSION"""
    out = {}
    dc, n = S([0, 1, 2], 0, 0, 0, 0), 3
    out["refinement_before_first_scan"] = write(16, 16, "444", [dc, S([0], 1, 63, 1, 0)], 90)[0]
    out["two_first_scans_of_one_band"] = write(16, 16, "444", [dc, S([0], 1, 63, 0, 0), S([0], 1, 63, 0, 0)], 91)[0]
    out["band_over_two_al"] = write(16, 16, "444", [dc, S([0], 1, 5, 0, 1), S([0], 6, 63, 0, 2), S([0], 1, 63, 2, 1)], 92)[0]
    out["ac_before_dc"] = write(16, 16, "444", [S([0], 1, 63, 0, 0), dc], 93)[0]
    out["sequential_two_scans"] = sequential_two_scans()
    assert n == 3
    return out


def sequential_two_scans():
    """SOF0, 4:4:4, scan 1 = Y, scan 2 = Cb Cr interleaved: sequential multi-scan, out of the device path's scope"""
    rng = np.random.default_rng(94)
    G = geometry(16, 16, "444")
    truth = truth_planes(G, rng, 0.2, amp=63)
    out = bytearray(b"\xff\xd8")
    for c in range(3):
        out += seg(0xDB, bytes([c]) + bytes([16] * 64))
    body = bytes([8, 0, 16, 0, 16, 3]) + b"".join(bytes([c + 1, 0x11, c]) for c in range(3))
    out += seg(0xC0, body)
    for comps in ([0], [1, 2]):
        toks, pred = [], {c: 0 for c in comps}
        for m in range(4):
            for ci in comps:
                blk = truth[ci][m // 2, m % 2]
                d = int(blk[0]) - pred[ci]
                pred[ci] = int(blk[0])
                toks += [("s", "dc", nbits(abs(d))), ("b", d if d >= 0 else d - 1, nbits(abs(d)))]
                r = 0
                for k in range(1, 64):
                    v = int(blk[ZIGZAG[k]])
                    if v == 0:
                        r += 1
                        continue
                    while r > 15:
                        toks.append(("s", "ac", 0xF0))
                        r -= 16
                    toks += [("s", "ac", (r << 4) | nbits(abs(v))), ("b", v if v >= 0 else v - 1, nbits(abs(v)))]
                    r = 0
                if r:
                    toks.append(("s", "ac", 0))
        codes = {}
        for cls in ("dc", "ac"):
            tab = shaped_table({t[2] for t in toks if t[0] == "s" and t[1] == cls}, "flat")
            out += dht(0 if cls == "dc" else 1, 0, tab)
            codes[cls] = codes_of(tab)
        out += seg(0xDA, bytes([len(comps)]) + b"".join(bytes([c + 1, 0]) for c in comps) + bytes([0, 63, 0]))
        b = Bits()
        for t in toks:
            b.put(*(codes[t[1]][t[2]] if t[0] == "s" else t[1:]))
        out += b.bytes("ones", rng)
    return bytes(out + b"\xff\xd9")


def scan_spans(data):
    """[(first, last + 1)] of the entropy-coded bytes behind every SOS"""
    spans, i = [], 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF
        if data[i + 1] == 0xD9:
            break
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        i += 2 + n
        if m == 0xDA:
            j = i
            while j + 1 < len(data) and not (data[j] == 0xFF and data[j + 1] not in (0x00, 0xFF) and not 0xD0 <= data[j + 1] <= 0xD7):
                j += 1
            spans.append((i, j))
            i = j
    return spans


def damaged(name, k):
    """seeded damage inside a scan of corpus file `name`: k even -> one byte XORed, k odd -> the file cut there (EOI appended)"""
    data = entry(name)[0]
    rng = np.random.default_rng(1000 + k)
    spans = [s for s in scan_spans(data) if s[1] > s[0]]
    a, b = spans[int(rng.integers(0, len(spans)))]
    at = int(rng.integers(a, b))
    if k % 2 == 0:
        return data[:at] + bytes([data[at] ^ int(rng.integers(1, 256))]) + data[at + 1:]
    return data[:at] + b"\xff\xd9"
