"""The JPEG host front end's answers on a fixed corpus: tests/golden/jpeg_marker_results.json, replayed by
tests/test_jpeg_marker_walk.py.

    python tests/golden/make_jpeg_marker_golden.py            write the file (run at the commit whose behaviour is the record)

The corpus is deterministic: every committed JPEG fixture, the crafted files of tests/jpeg_gen.py, progressive files this
library's writer makes from jpeg_gen's planes, seeded mutations of the smallest of them (byte rewrites in front of the scan
as tests/test_jpeg_headers.py does them, rewrites aimed at segment lengths and at the SOF / SOS / DHT / DQT count fields,
segments inserted, removed and reordered) and hand-made files for the refusals mutations do not reach.  For every case and
every host entry point the record is "rc:digest of the output buffers", or "rc:message" for a refusal.  Digests only: the
file stays small.  REFUSALS lists every refusal text of the two strict marker walks; writing the file asserts that each is
produced (or says why none can be), and that the mutated cases are neither all refused nor all accepted."""
import ctypes as C
import hashlib
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import jpeg_gen as G  # noqa: E402

RESULTS = os.path.join(HERE, "jpeg_marker_results.json")
ENTRY_POINTS = ("parse_headers", "frame_info", "read_coefficients_host", "exif_orientation", "icc_profile_kind", "scan_report")
MAX_BLOCKS = 8192                     # planes and scan reports are asked for only below this many blocks (a mutated size field)

# (entry point, text) of every fail() in the marker part of parse_jpeg, in read_jpeg up to where a scan's bits are read and in
# finish_frame.  UNREACHABLE: texts no input produces, with the reason.
REFUSALS = [
    ("parse_headers", "not a JPEG (no SOI)"), ("parse_headers", "marker expected at byte"), ("parse_headers", "truncated marker segment FF"),
    ("parse_headers", "bad DQT"), ("parse_headers", "bad DHT"), ("parse_headers", "-bit JPEG"), ("parse_headers", "-component JPEG"),
    ("parse_headers", "bad SOF"), ("parse_headers", "(only baseline Huffman)"), ("parse_headers", "SOS before SOF"),
    ("parse_headers", "non-interleaved / multi-scan JPEG"), ("parse_headers", "scan component order"), ("parse_headers", "bad SOS"),
    ("parse_headers", "no frame / scan found"), ("parse_headers", "RGB-coded JPEG"), ("parse_headers", "sampling factor "),
    ("parse_headers", "missing quantisation or Huffman table"), ("parse_headers", "(chroma must be 1x1)"),
    ("frame_info", "not a JPEG (no SOI)"), ("frame_info", "marker expected at byte"), ("frame_info", "truncated marker segment FF"),
    ("frame_info", "bad DQT"), ("frame_info", "bad DHT"), ("frame_info", "two frame headers"), ("frame_info", "-bit JPEG"),
    ("frame_info", "-component JPEG"), ("frame_info", "bad SOF"), ("frame_info", "(Huffman sequential and progressive only)"),
    ("frame_info", "SOS before SOF"), ("frame_info", "no frame found"), ("frame_info", "sampling factor "),
    ("frame_info", "(chroma must be 1x1)"), ("frame_info", "RGB-coded JPEG"),
    ("read_coefficients_host", "bad SOS"), ("read_coefficients_host", "scan names an unknown component"),
    ("read_coefficients_host", "bad progressive scan parameters"), ("read_coefficients_host", "bad sequential scan parameters"),
    ("read_coefficients_host", "missing quantisation table"), ("read_coefficients_host", "missing Huffman table"),
    ("read_coefficients_host", "no scan found"),
]
UNREACHABLE = {
    "parse_jpeg: %u blocks per MCU (limit %u)": "behind the factor range 1..2 and chroma 1x1 an MCU holds at most 4 + 1 + 1 blocks",
    "finish_frame: %d-component JPEG": "read_jpeg refuses the count with the same text before it calls finish_frame",
}


# ---- the library ------------------------------------------------------------------------------------------------------------
class ScanReport(C.Structure):
    _fields_ = ([(n, C.c_uint32) for n in ("segments", "sub_sequences", "scan_complete", "pool_entries", "pool_entries_used",
                                            "prefixes_left_to_search", "pair_entries", "segments_with_wrong_block_count",
                                            "segments_with_invalid_codes", "pair_walk_mismatches", "count_walk_mismatches")]
                + [("_pad", C.c_uint32)] + [(n, C.c_uint64) for n in ("symbols", "table_reads_with_pairs", "blocks")]
                + [("dc_sum", C.c_int32 * 3), ("dc_last_segment", C.c_int32 * 3)])


def library():
    from imageflow_amd import _native
    _native.lib()
    L = C.CDLL(_native.LIB_PATH)                               # a handle of its own: the argument types set here are nobody else's
    L.ifhip_last_error_message.restype = C.c_char_p
    L.ifhip_jpeg_parse_headers.argtypes = [C.c_char_p, C.c_size_t] + [C.c_void_p] * 9
    L.ifhip_jpeg_frame_info.argtypes = [C.c_char_p, C.c_size_t] + [C.c_void_p] * 9
    L.ifhip_jpeg_read_coefficients_host.argtypes = [C.c_char_p, C.c_size_t] + [C.c_void_p] * 4
    L.ifhip_jpeg_exif_orientation.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    L.ifhip_jpeg_icc_profile_kind.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    L.ifhip_jpeg_debug_scan_report.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    L.ifhip_jpeg_write.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                   C.c_size_t, C.POINTER(C.c_size_t)]
    return L


def _answer(L, rc, bufs):
    if rc != 0:
        return f"{rc}:{(L.ifhip_last_error_message() or b'').decode('utf-8', 'replace')}"
    h = hashlib.sha1()
    for b in bufs:
        h.update(b.tobytes())
    return f"0:{h.hexdigest()[:8]}"


def _frame_buffers():
    """w, h, n, hs3, vs3, bw3, bh3, qt3x64, last -- every one filled with a pattern the call must overwrite or leave"""
    return [np.full(1, 0xA5A5A5A5, np.uint32), np.full(1, 0xA5A5A5A5, np.uint32), np.full(1, -1515870811, np.int32), np.full(3, 0xA5, np.uint8),
            np.full(3, 0xA5, np.uint8), np.full(3, 0xA5A5A5A5, np.uint32), np.full(3, 0xA5A5A5A5, np.uint32), np.full(192, 0xA5A5, np.uint16),
            np.full(1, 0xA5A5A5A5, np.uint32)]


def answers(L, data):
    """-> {entry point: answer} of one file"""
    out = {}
    b = _frame_buffers()
    rc = L.ifhip_jpeg_parse_headers(data, len(data), *[x.ctypes.data for x in b])
    out["parse_headers"] = _answer(L, rc, b)
    parsed_blocks = int((b[5].astype(np.uint64) * b[6])[:max(int(b[2][0]), 0)].sum()) if rc == 0 else 0
    if parsed_blocks > MAX_BLOCKS:
        out["scan_report"] = "skipped: too many blocks"
    else:
        r = np.full(C.sizeof(ScanReport), 0xA5, np.uint8)
        out["scan_report"] = _answer(L, L.ifhip_jpeg_debug_scan_report(data, len(data), r.ctypes.data), [r])
    b = _frame_buffers()
    rc = L.ifhip_jpeg_frame_info(data, len(data), *[x.ctypes.data for x in b])
    out["frame_info"] = _answer(L, rc, b)
    n = int(b[2][0]) if rc == 0 else 0
    blocks = [int(b[5][c]) * int(b[6][c]) if c < n else 0 for c in range(3)]
    if sum(blocks) > MAX_BLOCKS:
        out["read_coefficients_host"] = "skipped: too many blocks"
    else:
        planes = [np.full(max(k, 1) * 64, 0x7777, np.int16) for k in blocks]
        qt = np.full(192, 0xA5A5, np.uint16)
        rc = L.ifhip_jpeg_read_coefficients_host(data, len(data), planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, qt.ctypes.data)
        out["read_coefficients_host"] = _answer(L, rc, planes + [qt])
    for name, fn in (("exif_orientation", L.ifhip_jpeg_exif_orientation), ("icc_profile_kind", L.ifhip_jpeg_icc_profile_kind)):
        v = np.full(1, -7, np.int32)
        out[name] = _answer(L, fn(data, len(data), v.ctypes.data), [v])
    return out


# ---- the corpus ---------------------------------------------------------------------------------------------------------------
def fixture_files():
    for name in ("jpeg_cases.npz", "jpeg_encode_cases.npz", "jpeg_entropy_cases.npz"):
        z = np.load(os.path.join(HERE, name))
        for i, n in enumerate(z["names"]):
            yield f"{name}:{n}", z[f"jpg_{i}"].tobytes()
        if "progressive" in z.files:
            yield f"{name}:progressive", z["progressive"].tobytes()


def written_progressive(L):
    """jpeg_gen's planes through this library's writer: progressive (and progressive with restart-free optimised tables) files"""
    for name, flags in (("std_444", 2), ("std_420", 3), ("std_422", 2), ("std_gray", 2), ("std_440", 3)):
        data, planes, qt, st = G.entry(name)
        hs, vs = G.SAMPLING[st["sampling"]]
        n = len(planes)
        coef = [np.ascontiguousarray(planes[c]) if c < n else np.zeros(64, np.int16) for c in range(3)]
        bw = np.array([planes[c].shape[1] if c < n else 0 for c in range(3)], np.uint32)
        bh = np.array([planes[c].shape[0] if c < n else 0 for c in range(3)], np.uint32)
        h3, v3 = np.array(list(hs) + [0] * (3 - n), np.uint8), np.array(list(vs) + [0] * (3 - n), np.uint8)
        out, k = np.zeros(1 << 18, np.uint8), C.c_size_t()
        rc = L.ifhip_jpeg_write(coef[0].ctypes.data, coef[1].ctypes.data, coef[2].ctypes.data, bw.ctypes.data, bh.ctypes.data, n, h3.ctypes.data,
                                v3.ctypes.data, st["width"], st["height"], 85, flags, out.ctypes.data, out.size, C.byref(k))
        assert rc == 0, (name, L.ifhip_last_error_message())
        yield f"written:{name}:flags{flags}", out[:k.value].tobytes()


def segments(data):
    """[(offset of the FF, marker, segment length incl. its two length bytes)] up to and including the first SOS"""
    out, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        m = data[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        if m == 0xD9:
            break
        seg = (data[i + 2] << 8) | data[i + 3]
        if seg < 2 or i + 2 + seg > len(data):
            break
        out.append((i, m, seg))
        if m == 0xDA:
            break
        i += 2 + seg
    return out


def marker(m, payload):
    return bytes([0xFF, m]) + struct.pack(">H", len(payload) + 2) + payload


def adobe(transform):
    return marker(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform]))


def _first(segs, *markers):
    return next(((o, m, s) for o, m, s in segs if m in markers), None)


def _headers_module():
    from tests import test_jpeg_headers as H
    return H


def structural(data, op, rng):
    """one of the segment-level mutations; None when the file has nothing for it to act on"""
    H = _headers_module()
    segs = segments(data)
    sof, sos = _first(segs, 0xC0, 0xC1, 0xC2), _first(segs, 0xDA)
    if not sof or not sos:
        return None
    after_sof = sof[0] + 2 + sof[2]
    if op == "second_sof":
        at = (after_sof, sos[0])[int(rng.integers(0, 2))]
        return data[:at] + data[sof[0]:after_sof] + data[at:]
    if op == "adobe_behind_sof":
        return data[:after_sof] + adobe(int(rng.integers(0, 3))) + data[after_sof:]
    if op == "adobe_in_front_of_sof":
        return data[:sof[0]] + adobe(int(rng.integers(0, 3))) + data[sof[0]:]
    if op == "dqt_between_scans":                              # behind the first scan's data: in front of the next marker that is no RSTn
        i = sos[0] + 2 + sos[2]
        while i + 1 < len(data) and not (data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF) and not 0xD0 <= data[i + 1] <= 0xD7):
            i += 1
        tid = int(rng.integers(0, 5))
        return data[:i] + marker(0xDB, bytes([tid]) + bytes(int(v) for v in rng.integers(1, 255, 64))) + data[i:]
    if op == "fill_bytes":
        o = segs[int(rng.integers(0, len(segs)))][0]
        return data[:o] + b"\xff" * int(rng.integers(1, 5)) + data[o:]
    if op == "dht_tail":                                       # a DHT whose payload is empty, or a table and a tail too short for another
        tail = (b"", bytes(int(v) for v in rng.integers(0, 256, int(rng.integers(1, 17)))))[int(rng.integers(0, 2))]
        dht = _first(segs, 0xC4)
        if tail and dht:
            return data[:dht[0]] + marker(0xC4, data[dht[0] + 4:dht[0] + 2 + dht[2]] + tail) + data[dht[0] + 2 + dht[2]:]
        return data[:sos[0]] + marker(0xC4, tail) + data[sos[0]:]
    if op == "icc_out_of_order":
        chunks = H.icc_app2(H.make_icc(xyz=H.P3_XYZ), pieces=3)
        parts, i = [], 0
        while i < len(chunks):
            n = 2 + ((chunks[i + 2] << 8) | chunks[i + 3])
            parts.append(chunks[i:i + n])
            i += n
        order = [int(v) for v in rng.permutation(3)]
        if order == [0, 1, 2]:
            order = [2, 0, 1]
        return data[:2] + b"".join(parts[k] for k in order) + data[2:]
    if op == "exif":
        return data[:2] + H._exif_app1(int(rng.integers(0, 10)), little=bool(rng.integers(0, 2))) + data[2:]
    if op == "swap_sof_marker":
        b = bytearray(data)
        b[sof[0] + 1] = int(rng.choice([0xC0, 0xC1, 0xC2, 0xC3, 0xC5, 0xC9, 0xCA, 0xCF]))
        return bytes(b)
    if op == "drop_segment":
        o, m, s = segs[int(rng.integers(0, len(segs) - 1))]
        return data[:o] + data[o + 2 + s:]
    if op == "no_payload_markers":
        o = segs[int(rng.integers(0, len(segs)))][0]
        return data[:o] + bytes([0xFF, int(rng.choice([0x01, 0xD0, 0xD7, 0xD8]))]) + data[o:]
    if op == "dri":
        return data[:sos[0]] + marker(0xDD, bytes(int(v) for v in rng.integers(0, 3, int(rng.integers(0, 4))))) + data[sos[0]:]
    if op == "move_sos_forward":                              # the scan header in front of the frame header
        return data[:sof[0]] + data[sos[0]:sos[0] + 2 + sos[2]] + data[sof[0]:]
    raise ValueError(op)


STRUCTURAL = ("second_sof", "adobe_behind_sof", "adobe_in_front_of_sof", "dqt_between_scans", "fill_bytes", "dht_tail", "icc_out_of_order",
              "exif", "swap_sof_marker", "drop_segment", "no_payload_markers", "dri", "move_sos_forward")
REQUIRED_STRUCTURAL = ("second_sof", "adobe_behind_sof", "dqt_between_scans", "fill_bytes", "dht_tail", "icc_out_of_order")


def field_rewrite(data, rng):
    """a rewrite aimed at a segment length or at a count field of SOF / SOS / DHT / DQT"""
    b = bytearray(data)
    segs = segments(data)
    o, m, s = segs[int(rng.integers(0, len(segs)))]
    q = o + 4                                                  # the payload
    kind = int(rng.integers(0, 3))
    if kind == 0 or m not in (0xC0, 0xC1, 0xC2, 0xDA, 0xC4, 0xDB):
        v = int(rng.choice([0, 1, 2, 3, max(s - 1, 0), s + 1, s + int(rng.integers(2, 40)), max(s - int(rng.integers(2, 20)), 0), 0xFFFF,
                            len(data) - o - 2, len(data) - o - 1]))
        b[o + 2], b[o + 3] = (v >> 8) & 255, v & 255
    elif m in (0xC0, 0xC1, 0xC2):
        f = int(rng.integers(0, 5))
        if f == 0:
            b[q + 5] = int(rng.choice([0, 1, 2, 3, 4, 255]))                       # Nf
        elif f == 1:
            b[q] = int(rng.choice([8, 8, 12, 16, 0]))                              # P
        elif f == 2:
            k = int(rng.integers(1, 5))
            b[q + k] = int(rng.choice([0, 0, 1, 255]))                             # a byte of Y / X
        elif f == 3 and s >= 8 + 3:
            c = int(rng.integers(0, (s - 8) // 3))
            b[q + 7 + 3 * c] = int(rng.choice([0x11, 0x21, 0x12, 0x22, 0x31, 0x14, 0x01, 0x10, 0x44]))   # H, V
        elif s >= 8 + 3:
            c = int(rng.integers(0, (s - 8) // 3))
            b[q + 6 + 3 * c + int(rng.choice([0, 2]))] = int(rng.choice([0, 1, 2, 3, 4, ord("R"), ord("G"), ord("B"), 255]))   # C, Tq
    elif m == 0xDA:
        f = int(rng.integers(0, 3))
        if f == 0:
            b[q] = int(rng.choice([0, 1, 2, 3, 4, 255]))                           # Ns
        elif f == 1 and s >= 6:
            b[q + 1 + int(rng.integers(0, s - 5))] = int(rng.choice([0, 1, 2, 3, 0x10, 0x11, 0x33, 0x40, 0x04, 255]))   # Cs / Td, Ta
        else:
            b[q + s - 2 - int(rng.integers(1, 4))] = int(rng.choice([0, 1, 5, 63, 64, 0x10, 0x01, 0x21]))   # Ss, Se, Ah / Al
    elif m == 0xC4:
        f = int(rng.integers(0, 2))
        if f == 0:
            b[q] = int(rng.choice([0x00, 0x10, 0x01, 0x13, 0x03, 0x20, 0x04, 0x14]))  # Tc, Th of the first table
        else:
            b[q + 1 + int(rng.integers(0, min(16, max(s - 3, 1))))] = int(rng.choice([0, 1, 2, 3, 16, 100, 255]))   # a count of its BITS
    else:
        b[q + int(rng.choice([0, 65]) if s > 67 + 2 else 0)] = int(rng.choice([0x00, 0x01, 0x03, 0x04, 0x10, 0x11, 0x13, 0x20, 0x0F]))   # Pq, Tq
    return bytes(b)


def byte_rewrites(data, rng):
    """test_parser_survives_mutated_headers' scheme: 1-3 bytes in front of the SOS plus 14, one time in five a truncation"""
    sos = data.find(b"\xff\xda")
    m = bytearray(data)
    for _ in range(int(rng.integers(1, 4))):
        m[int(rng.integers(2, sos + 14))] = int(rng.integers(0, 256))
    if rng.integers(0, 5) == 0:
        m = m[: int(rng.integers(4, len(m)))]
    return bytes(m)


def mutation_bases(plain):
    """a handful of the smallest files: two of each fixture set, a crafted one with a restart interval, two progressive ones"""
    by_set = {}
    for name, data in plain:
        by_set.setdefault(name.split(":")[0], []).append((len(data), name, data))
    bases = []
    for key in ("jpeg_cases.npz", "jpeg_encode_cases.npz", "jpeg_entropy_cases.npz"):
        bases += [(n, d) for _, n, d in sorted(by_set[key])[:2]]
    want = ("crafted:ri7_of_5_wide_420", "crafted:sof1_ids23_420", "written:std_444:flags2", "written:std_gray:flags2")
    bases += [(n, d) for n, d in plain if n in want]
    assert len(bases) == 10
    return bases


def mutated(plain):
    rng = np.random.default_rng(20)
    for base_name, data in mutation_bases(plain):
        assert data.find(b"\xff\xda") > 0
        for k in range(20):
            yield f"mutated:{base_name}:bytes{k}", byte_rewrites(data, rng)
        for k in range(16):
            yield f"mutated:{base_name}:field{k}", field_rewrite(data, rng)
        for op in STRUCTURAL:
            m = structural(data, op, rng)
            if m is not None:
                yield f"mutated:{base_name}:{op}", m


def hand_made():
    """files for the refusals and the lenient walks' corners; built on the crafted std_444 / std_gray / a progressive file"""
    H = _headers_module()
    base = G.entry("std_444")[0]
    gray = G.entry("std_gray")[0]
    segs = segments(base)
    dqt, sof, dht, sos = (_first(segs, m) for m in (0xDB, 0xC0, 0xC4, 0xDA))
    end = lambda s: s[0] + 2 + s[2]                            # noqa: E731

    def with_sof(payload, marker_byte=0xC0, src=base, s=sof):
        return src[:s[0]] + marker(marker_byte, payload) + src[end(s):]

    def with_sos(payload, src=base):
        s = _first(segments(src), 0xDA)
        return src[:s[0]] + marker(0xDA, payload) + src[end(s):]

    sof_p, sos_p = base[sof[0] + 4:end(sof)], base[sos[0] + 4:end(sos)]

    def sampling(*f):
        p = bytearray(sof_p)
        for c, (h, v) in enumerate(f):
            p[7 + 3 * c] = (h << 4) | v
        return with_sof(bytes(p))

    def ids(*cid):
        p, s = bytearray(sof_p), bytearray(sos_p)
        for c, v in enumerate(cid):
            p[6 + 3 * c] = v
            s[1 + 2 * c] = v
        return with_sos(bytes(s), with_sof(bytes(p)))

    yield "empty", b""
    yield "three_bytes", b"\xff\xd8\xff"
    yield "png", b"\x89PNG\r\n\x1a\n" + bytes(64)
    yield "soi_eoi", b"\xff\xd8\xff\xd9"
    yield "soi_only_fill", b"\xff\xd8" + b"\xff" * 9
    yield "garbage_behind_soi", b"\xff\xd8\x00\x11" + base[2:]
    yield "garbage_behind_dqt", base[:end(dqt)] + b"\x12" + base[end(dqt):]
    yield "truncated_in_tables", base[:end(sof) + 9]
    yield "length_one", base[:dqt[0] + 2] + b"\x00\x01" + base[dqt[0] + 4:]
    yield "length_zero", base[:dqt[0] + 2] + b"\x00\x00" + base[dqt[0] + 4:]
    yield "ends_inside_a_length", base[:sof[0] + 3]
    yield "dqt_id_4", base[:dqt[0] + 4] + b"\x04" + base[dqt[0] + 5:]
    yield "dqt_short", base[:sof[0]] + marker(0xDB, b"\x02" + bytes(40)) + base[sof[0]:]
    yield "dqt_16bit_short", base[:sof[0]] + marker(0xDB, b"\x12" + bytes(100)) + base[sof[0]:]
    yield "dqt_16bit", base[:sof[0]] + marker(0xDB, b"\x13" + bytes(range(128))) + base[sof[0]:]
    yield "dqt_empty", base[:sof[0]] + marker(0xDB, b"") + base[sof[0]:]
    yield "dht_class_2", base[:dht[0] + 4] + b"\x20" + base[dht[0] + 5:]
    yield "dht_id_4", base[:dht[0] + 4] + b"\x04" + base[dht[0] + 5:]
    yield "dht_257_values", base[:sos[0]] + marker(0xC4, b"\x00" + bytes([255, 2] + [0] * 14) + bytes(257)) + base[sos[0]:]
    yield "dht_values_cut", base[:sos[0]] + marker(0xC4, b"\x11" + bytes([0, 3] + [0] * 14) + bytes(2)) + base[sos[0]:]
    yield "dht_empty", base[:sos[0]] + marker(0xC4, b"") + base[sos[0]:]
    yield "dht_tail_16", base[:sos[0]] + marker(0xC4, b"\x00" + bytes([0, 1] + [0] * 14) + b"\x05" + bytes(16)) + base[sos[0]:]
    yield "sof_12bit", with_sof(b"\x0c" + sof_p[1:])
    yield "sof_five_bytes", with_sof(sof_p[:5])
    yield "sof_empty", with_sof(b"")
    yield "sof_4_components", with_sof(sof_p[:5] + b"\x04" + sof_p[6:] + b"\x04\x11\x00")
    yield "sof_2_components", with_sof(sof_p[:5] + b"\x02" + sof_p[6:12])
    yield "sof_0_components", with_sof(sof_p[:5] + b"\x00")
    yield "sof_components_cut", with_sof(sof_p[:-2])
    yield "sof_zero_width", with_sof(sof_p[:3] + b"\x00\x00" + sof_p[5:])
    yield "sof_zero_height", with_sof(sof_p[:1] + b"\x00\x00" + sof_p[3:])
    for m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
        yield f"sof_marker_{m:02X}", with_sof(sof_p, m)
    yield "jpg_marker_C8", with_sof(sof_p, 0xC8)
    yield "dac_marker_CC", base[:sof[0]] + marker(0xCC, b"\x00\x10") + base[sof[0]:]
    yield "two_sofs", base[:end(sof)] + base[sof[0]:]
    yield "two_sofs_second_is_gray", base[:end(sof)] + gray[_first(segments(gray), 0xC0)[0]:][:2 + _first(segments(gray), 0xC0)[2]] + base[end(sof):]
    yield "sos_before_sof", base[:sof[0]] + base[sos[0]:end(sos)] + base[sof[0]:]
    yield "no_sof", base[:sof[0]] + base[end(sof):]
    yield "sof_and_no_sos", base[:sos[0]] + b"\xff\xd9"
    yield "no_sof_no_sos", base[:sof[0]] + b"\xff\xd9"
    yield "sos_empty", with_sos(b"")
    yield "sos_0_components", with_sos(b"\x00" + sos_p[1:])
    yield "sos_1_component", with_sos(b"\x01" + sos_p[1:3] + sos_p[-3:])
    yield "sos_4_components", with_sos(b"\x04" + sos_p[1:7] + b"\x04\x00" + sos_p[-3:])
    yield "sos_cut", with_sos(sos_p[:-2])
    yield "sos_order", with_sos(sos_p[:1] + sos_p[3:5] + sos_p[1:3] + sos_p[5:])
    yield "sos_unknown_component", with_sos(sos_p[:1] + b"\x63" + sos_p[2:])
    yield "sos_dc_table_4", with_sos(sos_p[:2] + b"\x40" + sos_p[3:])
    yield "sos_ac_table_9", with_sos(sos_p[:4] + b"\x19" + sos_p[5:])
    yield "sos_ss_1", with_sos(sos_p[:-3] + b"\x01\x3f\x00")
    yield "sos_se_62", with_sos(sos_p[:-3] + b"\x00\x3e\x00")
    yield "sos_al_1", with_sos(sos_p[:-3] + b"\x00\x3f\x01")
    yield "rgb_ids", ids(ord("R"), ord("G"), ord("B"))
    yield "rgb_ids_adobe_1", ids(ord("R"), ord("G"), ord("B"))[:2] + adobe(1) + ids(ord("R"), ord("G"), ord("B"))[2:]
    for t in (0, 1, 2):
        yield f"adobe_{t}_in_front_of_sof", base[:sof[0]] + adobe(t) + base[sof[0]:]
        yield f"adobe_{t}_behind_sof", base[:end(sof)] + adobe(t) + base[end(sof):]
        yield f"adobe_{t}_gray", gray[:2] + adobe(t) + gray[2:]
    yield "adobe_short", base[:2] + marker(0xEE, b"Adobe" + bytes(6)) + base[2:]
    yield "adobe_0_then_1", base[:2] + adobe(0) + adobe(1) + base[2:]
    for f in ([(3, 1), (1, 1), (1, 1)], [(1, 1), (1, 4), (1, 1)], [(0, 1), (1, 1), (1, 1)], [(2, 2), (2, 2), (2, 2)], [(2, 2), (2, 1), (1, 1)],
              [(1, 1), (2, 2), (2, 2)], [(2, 1), (1, 2), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)], [(1, 1), (1, 1), (2, 1)]):
        yield "sampling_" + "_".join(f"{h}x{v}" for h, v in f), sampling(*f)
    gsof = _first(segments(gray), 0xC0)
    gp = bytearray(gray[gsof[0] + 4:end(gsof)])
    for hv in (0x22, 0x31, 0x12):
        gp[7] = hv
        yield f"gray_sampling_{hv:02x}", with_sof(bytes(gp), src=gray, s=gsof)
    yield "no_dqt", base[:dqt[0]] + base[end(dqt):]
    yield "no_dht", base[:dht[0]] + base[end(dht):]
    yield "tq_3_absent", with_sof(sof_p[:-1] + b"\x03")
    yield "dri_behind_sof", base[:sos[0]] + marker(0xDD, b"\x00\x02") + base[sos[0]:]
    yield "dri_one_byte", base[:sos[0]] + marker(0xDD, b"\x07") + base[sos[0]:]
    yield "dri_twice", base[:sos[0]] + marker(0xDD, b"\x00\x02") + marker(0xDD, b"\x00\x00") + base[sos[0]:]
    yield "fill_bytes_everywhere", b"".join((b"\xff\xff\xff" if o in [s[0] for s in segs] else b"") + base[o:o + 1] for o in range(len(base)))
    yield "tem_rst_soi_between", base[:sof[0]] + b"\xff\x01\xff\xd0\xff\xd7\xff\xd8" + base[sof[0]:]
    yield "eoi_in_front_of_sof", base[:sof[0]] + b"\xff\xd9" + base[sof[0]:]
    yield "scan_cut", base[:end(sos) + 5]
    yield "scan_cut_eoi", base[:end(sos) + 5] + b"\xff\xd9"
    yield "scan_corrupt", base[:end(sos) + 3] + b"\xff\x00" * 6 + base[end(sos) + 15:]
    yield "gray_scan_cut", gray[:len(gray) - 12]
    # several scans: what the writer's progressive files and a non-interleaved sequential file ask of read_jpeg
    prog = next(d for n, d in written_progressive(library()) if n == "written:std_444:flags2")
    ps = segments(prog)
    psos = _first(ps, 0xDA)
    pp = prog[psos[0] + 4:end(psos)]
    yield "progressive_dc_scan_se_5", prog[:psos[0]] + marker(0xDA, pp[:-3] + b"\x00\x05" + pp[-1:]) + prog[end(psos):]
    yield "progressive_al_14", prog[:psos[0]] + marker(0xDA, pp[:-1] + b"\x0e") + prog[end(psos):]
    yield "progressive_ah_3_al_1", prog[:psos[0]] + marker(0xDA, pp[:-1] + b"\x31") + prog[end(psos):]
    yield "progressive_ac_scan_of_3", prog[:psos[0]] + marker(0xDA, pp[:-3] + b"\x01\x05" + pp[-1:]) + prog[end(psos):]
    yield "progressive_first_scan_only", prog[:psos[0]] + prog[psos[0]:].split(b"\xff\xc4")[0] + b"\xff\xd9"
    yield "progressive_no_dqt", prog[:_first(ps, 0xDB)[0]] + prog[end(_first(ps, 0xDB)):]
    pdht = _first(ps, 0xC4)
    yield "progressive_no_first_dht", prog[:pdht[0]] + prog[end(pdht):]
    yield "progressive_marked_sof0", prog[:_first(ps, 0xC2)[0] + 1] + b"\xc0" + prog[_first(ps, 0xC2)[0] + 2:]
    yield "sequential_luma_scan_only", with_sos(b"\x01" + sos_p[1:3] + sos_p[-3:])
    # the lenient walks
    exif, icc = H._exif_app1(6), H.icc_app2(H.make_icc(xyz=H.P3_XYZ), pieces=2)
    srgb = H.icc_app2(H.make_icc())
    yield "exif", base[:2] + exif + base[2:]
    yield "exif_big_endian_3", base[:2] + H._exif_app1(3, little=False) + base[2:]
    yield "exif_in_app2", base[:2] + b"\xff\xe2" + exif[2:] + base[2:]
    yield "exif_behind_fill_bytes", base[:2] + b"\xff\xff" + exif + base[2:]
    yield "exif_behind_garbage", base[:2] + b"\x00" + exif + base[2:]
    yield "exif_behind_truncated_segment", base[:2] + b"\xff\xe0\xff\xff" + exif + base[2:]
    yield "exif_behind_length_1", base[:2] + b"\xff\xe0\x00\x01" + exif + base[2:]
    yield "exif_behind_eoi", base[:2] + b"\xff\xd9" + exif + base[2:]
    yield "exif_behind_sos", base[:-2] + exif + b"\xff\xd9"
    yield "exif_behind_tem_and_rst", base[:2] + b"\xff\x01\xff\xd3" + exif + base[2:]
    yield "exif_cut_by_the_file", (base[:2] + exif)[:30]
    yield "exif_alone", b"\xff\xd8" + exif
    yield "exif_short_then_full", base[:2] + exif[:2] + b"\x00\x1c" + exif[4:30] + exif + base[2:]
    yield "icc_p3_two_chunks", base[:2] + icc + base[2:]
    yield "icc_srgb", base[:2] + srgb + base[2:]
    yield "icc_behind_sof", base[:end(sof)] + srgb + base[end(sof):]
    yield "icc_gray_profile_colour_frame", base[:2] + H.icc_app2(H.make_icc(space=b"GRAY")) + base[2:]
    yield "icc_gray_profile_gray_frame", gray[:2] + H.icc_app2(H.make_icc(space=b"GRAY")) + gray[2:]
    yield "icc_gray_profile_behind_gray_sof", gray[:end(gsof)] + H.icc_app2(H.make_icc(space=b"GRAY")) + gray[end(gsof):]
    gicc = gray[:2] + H.icc_app2(H.make_icc(space=b"GRAY")) + gray[2:]                  # ICC reads the component count from any SOFn
    yield "icc_gray_profile_sof3_one_component", with_sof(gray[gsof[0] + 4:end(gsof)], 0xC3, src=gicc, s=_first(segments(gicc), 0xC0))
    yield "icc_chunk_missing", base[:2] + H.icc_app2(H.make_icc(xyz=H.P3_XYZ), pieces=3, drop=1) + base[2:]
    yield "icc_chunk_twice", base[:2] + H.icc_app2(H.make_icc(xyz=H.P3_XYZ), pieces=2, dup=True) + base[2:]
    yield "icc_counts_differ", base[:2] + icc[:17] + b"\x03" + icc[18:] + base[2:]
    yield "icc_sequence_0", base[:2] + icc[:16] + b"\x00" + icc[17:] + base[2:]
    yield "icc_empty_chunk", base[:2] + b"\xff\xe2\x00\x10ICC_PROFILE\0\x01\x01" + base[2:]
    yield "icc_13_bytes", base[:2] + b"\xff\xe2\x00\x0fICC_PROFILE\0\x01" + base[2:]
    yield "icc_behind_garbage", base[:2] + b"\x07" + srgb + base[2:]
    yield "icc_behind_truncated_segment", base[:2] + b"\xff\xe0\xff\xff" + srgb + base[2:]
    yield "icc_second_chunk_behind_sos", base[:2] + icc[:2 + ((icc[2] << 8) | icc[3])] + base[2:-2] + icc[2 + ((icc[2] << 8) | icc[3]):] + b"\xff\xd9"
    yield "icc_and_exif", base[:2] + exif + srgb + base[2:]


def corpus(L=None):
    """-> [(name, bytes)]: the plain files, then the mutated ones, then the hand-made ones"""
    L = L or library()
    plain = list(fixture_files()) + [(f"crafted:{n}", G.entry(n)[0]) for n in G.names()] + list(written_progressive(L))
    cases = plain + list(mutated(plain)) + [(f"hand:{n}", d) for n, d in hand_made()]
    assert len({n for n, _ in cases}) == len(cases)
    return cases


def plain_cases(cases):
    return [(n, d) for n, d in cases if not n.startswith(("mutated:", "hand:"))]


def write_sanitizer_corpus(path, cases):
    """every case behind a 4-byte little-endian length: what tests/jpeg_markers_sanitize.cpp reads"""
    with open(path, "wb") as f:
        for _, d in cases:
            f.write(struct.pack("<I", len(d)) + d)


def check_conditions(cases, results):
    for ep, text in REFUSALS:
        hit = next((n for n, _ in cases if not results[n][ep].startswith("0:") and text in results[n][ep]), None)
        assert hit, f"no case makes {ep} refuse with {text!r}"
    mut = [n for n, _ in cases if n.startswith("mutated:")]
    for ep in ("parse_headers", "frame_info"):
        refused = sum(not results[n][ep].startswith("0:") for n in mut)
        assert len(mut) / 5 <= refused <= 4 * len(mut) / 5, (ep, refused, len(mut))
        print(f"{ep}: {refused} of {len(mut)} mutated cases refused")
    for op in REQUIRED_STRUCTURAL:
        assert any(f":{op}" in n for n in mut), op
    # the required mutations reach what they are for
    said = lambda ep, text: any(text in results[n][ep] for n in mut)   # noqa: E731
    assert said("frame_info", "two frame headers") and said("frame_info", "RGB-coded")


def _wrapped(items, width=150):
    """JSON texts of `items`, comma separated, packed into lines of about `width` characters"""
    lines, line = [], ""
    for t in (json.dumps(i) for i in items):
        if line and len(line) + len(t) + 2 > width:
            lines.append(line + ",")
            line = t
        else:
            line = line + ", " + t if line else t
    return "\n".join(lines + [line])


def save_recorded(cases, results):
    """The file holds every distinct answer once and, per case in the corpus's order, six indices into that list; the cases'
    names are not stored but digested (the corpus rebuilds them)."""
    seen = [results[n][ep] for n, _ in cases for ep in ENTRY_POINTS]
    answers = sorted(set(seen), key=lambda a: (-seen.count(a), a))            # the commonest first: short indices
    at = {a: i for i, a in enumerate(answers)}
    rows = [" ".join(str(at[results[n][ep]]) for ep in ENTRY_POINTS) for n, _ in cases]
    names = hashlib.sha1("\n".join(n for n, _ in cases).encode()).hexdigest()
    with open(RESULTS, "w") as f:
        f.write('{"entry_points": %s,\n"unreachable": %s,\n"names_sha1": "%s",\n"answers": [\n%s],\n"cases": [\n%s]}\n'
                % (json.dumps(ENTRY_POINTS), json.dumps(UNREACHABLE), names, _wrapped(answers), _wrapped(rows)))


def load_recorded(cases):
    """-> {case name: [answer per entry point]} for the corpus `cases`, which must be the recorded one"""
    with open(RESULTS) as f:
        rec = json.load(f)
    assert tuple(rec["entry_points"]) == ENTRY_POINTS
    assert len(rec["cases"]) == len(cases) and rec["names_sha1"] == hashlib.sha1("\n".join(n for n, _ in cases).encode()).hexdigest(), \
        "the corpus is not the recorded one"
    return {n: [rec["answers"][int(i)] for i in row.split()] for (n, _), row in zip(cases, rec["cases"])}


def main():
    L = library()
    cases = corpus(L)
    results = {n: answers(L, d) for n, d in cases}
    check_conditions(cases, results)
    save_recorded(cases, results)
    print(f"{len(cases)} cases -> {RESULTS} ({os.path.getsize(RESULTS)} bytes)")


if __name__ == "__main__":
    main()
