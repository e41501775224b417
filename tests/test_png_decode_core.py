"""The device PNG decoder's algorithm without a device (csrc/png_decode_core.hpp: bit reader, code tables with zlib's
refusals, the token loop, window copies, flushes, Adler-32, the skewed un-filter, the sample expansion -- what the gfx950
kernels of csrc/png_decode.hip are built from).  tests/png_decode_emulate.cpp runs them lane by lane on the CPU;
zlib.decompress is the yardstick for every good stream, and every damaged stream must give its error status.  The same
cases run a second time in a build with ASan + UBSan, where an access outside the given bounds ends the program."""
import ctypes as C
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from tests import png_decode_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "png_decode_emulate.cpp")
_EMU = {}
OK, TRUNCATED, BLOCK_TYPE, STORED_LENGTH, CODE_LENGTHS, BAD_CODE, DISTANCE, ZLIB_HEADER, ADLER, TOO_LITTLE, FILTER = range(11)


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="png_decode_emulate_")
        so = os.path.join(d, "libpng_decode_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
        lib = C.CDLL(so)
        lib.png_dec_emu_inflate.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.png_dec_emu_inflate.restype = C.c_uint32
        lib.png_dec_emu_inflated_size.argtypes = [C.c_uint32] * 5
        lib.png_dec_emu_inflated_size.restype = C.c_uint64
        lib.png_dec_emu_filter_bpp.argtypes = [C.c_uint32] * 2
        lib.png_dec_emu_filter_bpp.restype = C.c_uint32
        lib.png_dec_emu_unfilter.argtypes = [C.c_void_p] + [C.c_uint32] * 5
        lib.png_dec_emu_unfilter.restype = C.c_uint32
        lib.png_dec_emu_expand.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        lib.png_dec_emu_expand.restype = None
        _EMU["lib"] = lib
    return _EMU["lib"]


def inflate(z, cap):
    """-> (status, the bytes produced)"""
    lib = emulator()
    src = np.frombuffer(bytes(z) + b"\0", np.uint8).copy()
    out, n = np.zeros(max(cap, 1), np.uint8), C.c_uint32(0)
    st = lib.png_dec_emu_inflate(src.ctypes.data, len(z), out.ctypes.data, cap, C.byref(n))
    return st, out[:n.value].tobytes()


class Bits:
    """a deflate bit writer: values low bit first, Huffman codes high bit first"""
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        self.v |= value << self.n
        self.n += bits
        return self

    def code(self, value, bits):
        for i in range(bits - 1, -1, -1):
            self.put((value >> i) & 1, 1)
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def zwrap(raw, data=b""):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data))


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    return O.compress(data, level, strategy)


def photo_like(n, seed=0):
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.integers(-3, 4, n)) & 255
    return walk.astype(np.uint8).tobytes()


def own_coder_stream():
    from tests.test_png_device_coder import deflate as device_deflate
    from tests import png_oracle as P
    stream = P.filter_image(P.photo_frame(200, 60))[1]
    return stream, device_deflate(stream, 3, 1 + 3 * 200)[0]


def far_match_stream(head, dist, length, tail=b"tail"):
    """(data, zlib stream): len(head) <= 65535 stored bytes, one match of `length` at `dist` (>= 24577), literals"""
    data = head + head[len(head) - dist:len(head) - dist + length] + tail
    assert 24577 <= dist <= len(head) and length <= dist
    n = len(head)
    bits = Bits().put(1, 1).put(1, 2)
    if length == 258:
        bits.code(0xC0 + 5, 8)
    elif length == 3:
        bits.code(1, 7)
    else:
        assert length == 65                                          # symbol 276: lengths 59..66, three extra bits
        bits.code(276 - 256, 7).put(65 - 59, 3)
    bits.code(29, 5).put(dist - 24577, 13)
    for ch in tail:
        bits.code(0x30 + ch, 8)
    bits.code(0, 7)
    z = b"\x78\x9c\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + head + bits.bytes() + struct.pack(">I", zlib.adler32(data))
    return data, z


def good_streams():
    rng = np.random.default_rng(11)
    text = (b"the quick brown fox jumps over the lazy dog. " * 400)
    noise = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    photo = photo_like(150000)
    far = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    cases = {
        "stored": (photo[:70000], deflate(photo[:70000], 0)),
        "fixed": (text[:3000], deflate(text[:3000], 6, zlib.Z_FIXED)),
        "level1": (photo, deflate(photo, 1)),
        "level6": (photo, deflate(photo, 6)),
        "level9": (text + photo[:40000], deflate(text + photo[:40000], 9)),
        "rle": (photo, deflate(photo, 6, zlib.Z_RLE)),
        "huffman_only": (photo[:50000], deflate(photo[:50000], 6, zlib.Z_HUFFMAN_ONLY)),
        "filtered": (photo, deflate(photo, 6, zlib.Z_FILTERED)),
        "noise": (noise, deflate(noise, 6)),
        "empty": (b"", deflate(b"")),
        "one_byte": (b"\x07", deflate(b"\x07")),
        "match_258": (b"ab" + b"x" * 600 + b"ab", deflate(b"ab" + b"x" * 600 + b"ab", 9)),
        "distance_1_long": (b"q" + b"\0" * 100000, deflate(b"q" + b"\0" * 100000, 6)),
        "single_distance": (bytes([3, 1, 4, 1, 5, 9, 2]) * 3000, deflate(bytes([3, 1, 4, 1, 5, 9, 2]) * 3000, 6)),
    }
    # Distances zlib never writes (its matches stop 262 bytes short of the window; libdeflate, zopfli and 7-zip use the whole
    # of it), by hand: 32768 stored bytes, then one match.  From 32768 - 258 on, the slots a match reads on the 32 KiB ring are
    # slots the same match writes: 32768 is the one such distance where every byte lands on its own source.
    for dist, length in ((32768, 258), (32767, 258), (32766, 258), (32700, 258), (32600, 258), (32511, 258), (32510, 258), (32767, 3), (32705, 65), (32704, 65)):
        cases["distance_%d_length_%d" % (dist, length)] = far_match_stream(far, dist, length)
    c = zlib.compressobj(6)
    many, z = b"", b""
    for i in range(40):                                               # many blocks: a full flush after every piece, of every block type
        piece = (text[:997] if i % 3 == 0 else noise[i * 500:i * 500 + 700] if i % 3 == 1 else photo[i * 1000:i * 1000 + 3000])
        many += piece
        z += c.compress(piece) + c.flush(zlib.Z_FULL_FLUSH)
    cases["many_blocks"] = (many, z + c.flush())
    cases["own_coder"] = own_coder_stream()
    return cases


def damaged_streams():
    """name -> (stream, cap, the status it must give)"""
    photo = photo_like(40000, 2)
    z = deflate(photo, 6)
    out = {}
    for cut in (0, 1, 2, 3, 10, len(z) // 2, len(z) - 5, len(z) - 1):
        out["truncated_%d" % cut] = (z[:cut], len(photo), TRUNCATED)
    s = deflate(photo[:5000], 0)
    out["truncated_stored"] = (s[:3000], 5000, TRUNCATED)
    out["truncated_stored_header"] = (s[:5], 5000, TRUNCATED)
    out["block_type_3"] = (zwrap(Bits().put(1, 1).put(3, 2).bytes()), 10, BLOCK_TYPE)
    out["len_nlen"] = (zwrap(b"\x01\x05\x00\x05\x00hello", b"hello"), 5, STORED_LENGTH)
    over = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19):
        over.put(1, 3)
    out["oversubscribed_code_lengths"] = (zwrap(over.bytes() + bytes(8)), 10, CODE_LENGTHS)
    inc = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for i in range(19):
        inc.put(2 if i < 3 else 0, 3)                                 # three codes of two bits: incomplete
    out["incomplete_code_lengths"] = (zwrap(inc.bytes() + bytes(8)), 10, CODE_LENGTHS)
    far = Bits().put(1, 1).put(1, 2).code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7)      # 'a', length 3 at distance 2
    out["distance_before_start"] = (zwrap(far.bytes(), b"aaaa"), 4, DISTANCE)
    bad = Bits().put(1, 1).put(1, 2).code(0xC0 + 6, 8).code(0, 7)                               # literal/length symbol 286
    out["symbol_286"] = (zwrap(bad.bytes()), 4, BAD_CODE)
    bad = Bits().put(1, 1).put(1, 2).code(0x30 + 97, 8).code(1, 7).code(30, 5).code(0, 7)       # distance symbol 30
    out["distance_symbol_30"] = (zwrap(bad.bytes()), 4, BAD_CODE)
    out["wrong_adler"] = (z[:-1] + bytes([z[-1] ^ 1]), len(photo), ADLER)
    out["too_little_data"] = (z, len(photo) + 1, TOO_LITTLE)
    out["too_little_data_empty"] = (deflate(b""), 7, TOO_LITTLE)
    out["bad_method"] = (b"\x79\x9c" + z[2:], len(photo), ZLIB_HEADER)
    out["bad_fcheck"] = (b"\x78\x9d" + z[2:], len(photo), ZLIB_HEADER)
    out["preset_dictionary"] = (b"\x78\xbb" + z[2:], len(photo), ZLIB_HEADER)
    return out


GOOD = good_streams()
DAMAGED = damaged_streams()


@pytest.mark.parametrize("name", sorted(GOOD))
def test_good_streams_inflate_to_what_zlib_gives(name):
    data, z = GOOD[name]
    assert zlib.decompress(z) == data
    st, got = inflate(z, len(data))
    assert st == OK and got == data


def test_the_coverage_the_names_promise():
    assert GOOD["stored"][1][2] & 6 == 0                                # BTYPE 0
    assert GOOD["fixed"][1][2] & 6 == 2                                 # BTYPE 1
    assert len(GOOD["distance_1_long"][1]) < 200
    assert len(GOOD["distance_32768_length_258"][1]) < 32768 + 30       # the 258 bytes are one match
    assert sum(name.startswith("distance_327") or name.startswith("distance_326") or name.startswith("distance_325") for name in GOOD) >= 9


@pytest.mark.parametrize("name", sorted(GOOD))
def test_data_beyond_the_expected_size_is_ignored(name):
    data, z = GOOD[name]
    for cap in (0, 1, len(data) // 2, len(data) - 1):
        if 0 <= cap < len(data):
            st, got = inflate(z, cap)
            assert st == OK and got == data[:cap], cap


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damaged_streams_give_their_status(name):
    z, cap, want = DAMAGED[name]
    st, got = inflate(z, cap)
    assert st == want, (name, st)
    if want != TOO_LITTLE:
        with pytest.raises(zlib.error):
            zlib.decompress(z)


def test_every_prefix_of_a_short_stream_is_truncated_and_every_flipped_bit_is_handled():
    data = photo_like(600, 4) + b"abcabcabc" * 20
    for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED):
        z = deflate(data, 9, strategy)
        for cut in range(len(z)):
            assert inflate(z[:cut], len(data))[0] == TRUNCATED, cut
        for bit in range(8 * len(z)):                                   # any status, but never a wrong OK
            bad = bytearray(z)
            bad[bit >> 3] ^= 1 << (bit & 7)
            st, got = inflate(bytes(bad), len(data))
            d = zlib.decompressobj()
            try:                                                        # zlib up to one byte past the expected size: what lies beyond is ignored
                ref = d.decompress(bytes(bad), len(data) + 1)
            except zlib.error:
                ref = None
            if ref is not None and (len(ref) > len(data) or (len(ref) == len(data) and d.eof)):
                assert st == OK and got == ref[:len(data)], (bit, st)
            elif ref is not None and d.eof:
                assert st == TOO_LITTLE, (bit, st)
            elif st == OK:                                              # zlib met an error within one byte past the expected size: a stream that
                more = zlib.decompressobj()                             # holds exactly one byte more is cut before it, and is fine
                assert got == more.decompress(bytes(bad), len(data)) and not more.eof, (bit, st)
                assert inflate(bytes(bad), len(data) + 1)[0] not in (OK, TOO_LITTLE) or inflate(bytes(bad), len(data) + 2)[0] != OK, bit
            elif st == TOO_LITTLE:                                      # the deflate data ended early AND its checksum is wrong: too little is said first
                raw = zlib.decompressobj(-15)
                assert len(raw.decompress(bytes(bad[2:]))) < len(data) and raw.eof, bit


# ---- geometry, un-filter, expansion -------------------------------------------------------------------------------------------------
def test_geometry_equals_the_oracles():
    lib = emulator()
    for ct, depth in O.LEGAL:
        assert lib.png_dec_emu_filter_bpp(ct, depth) == O.filter_bpp(ct, depth)
        for w, h in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (5, 3), (8, 8), (13, 67), (200, 65)):
            for inter in (0, 1):
                assert lib.png_dec_emu_inflated_size(w, h, ct, depth, inter) == O.inflated_size(w, h, ct, depth, inter)


def emu_decode(data):
    """the emulation's BGRA of a file, through inflate, the skewed un-filter and the expansion"""
    lib = emulator()
    info = O.parse(data)
    w, h, ct, depth, inter = info["width"], info["height"], info["color_type"], info["depth"], info["interlace"]
    want = O.inflated_size(w, h, ct, depth, inter)
    st, raw = inflate(info["idat"], want)
    assert st == OK
    buf = np.frombuffer(raw, np.uint8).copy()
    assert lib.png_dec_emu_unfilter(buf.ctypes.data, w, h, ct, depth, inter) == OK
    pal = np.ascontiguousarray(O.palette_table(info)).view(np.uint32).reshape(256).copy()
    key = np.zeros(3, np.uint32)
    has = 0
    if info["trns"] is not None and ct in (0, 2):
        has = 1
        vals = struct.unpack(">H" if ct == 0 else ">HHH", info["trns"][:2 if ct == 0 else 6])
        key[:len(vals)] = vals
    stride = 4 * w + 12
    out = np.full((h, stride), 0xA5, np.uint8)
    lib.png_dec_emu_expand(buf.ctypes.data, w, h, ct, depth, inter, pal.ctypes.data, has, key.ctypes.data, out.ctypes.data, stride)
    assert (out[:, 4 * w:] == 0xA5).all()
    return out[:, :4 * w].reshape(h, w, 4)


@pytest.mark.parametrize("interlace", [False, True])
@pytest.mark.parametrize("ct,depth", O.LEGAL)
def test_emulated_files_equal_the_oracle(ct, depth, interlace):
    rng = np.random.default_rng(ct * 31 + depth)
    for (w, h), filters in (((1, 1), 4), ((1, 70), [1, 3, 4]), ((70, 1), 3), ((13, 67), [0, 1, 2, 3, 4]), ((37, 130), [4, 3, 1, 2, 0, 4, 4])):
        s = O.random_samples(rng, w, h, ct, depth, smooth=True)
        pal = rng.integers(0, 256, (1 << depth, 3), dtype=np.uint8) if ct == 3 else None
        trns = None
        if ct == 3:
            trns = bytes(rng.integers(0, 256, max(1, (1 << depth) // 2), dtype=np.uint8))
        elif ct == 0:
            trns = struct.pack(">H", int(s[0, 0, 0]))
        elif ct == 2:
            trns = struct.pack(">HHH", *[int(v) for v in s[0, 0]])
        data = O.write_png(s, ct, depth, filters=filters, interlace=interlace, palette=pal, trns=trns)
        want, _ = O.decode(data)
        assert np.array_equal(emu_decode(data), want), (w, h)


def test_a_filter_type_above_4_is_reported():
    lib = emulator()
    buf = np.zeros(3 * 5, np.uint8)
    buf[5] = 7
    assert lib.png_dec_emu_unfilter(buf.ctypes.data, 1, 3, 6, 8, 0) == FILTER


# ---- the same cases under ASan + UBSan ---------------------------------------------------------------------------------------------
def sanitizer_executable():
    if "asan" not in _EMU:
        d = tempfile.mkdtemp(prefix="png_decode_asan_")
        exe = os.path.join(d, "png_decode_emulate_asan")
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                            "-DPNG_DEC_EMU_MAIN", SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:                                           # (a toolchain without the static runtime)
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPNG_DEC_EMU_MAIN", SRC, "-o", exe], check=True)
        _EMU["asan"] = exe
    return _EMU["asan"]


def run_under_sanitizers(cases):
    """the packed cases of png_decode_emulate.cpp's main through the ASan + UBSan build -> its lines, "status produced crc32" each"""
    exe = sanitizer_executable()
    path = os.path.join(tempfile.mkdtemp(prefix="png_decode_cases_"), "cases.bin")
    with open(path, "wb") as f:
        f.write(b"".join(cases))
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    return lines


def test_under_sanitizers_no_access_leaves_the_given_bounds():
    cases, want = [], []
    for name in sorted(GOOD):
        data, z = GOOD[name]
        for cap in (len(data), len(data) // 3):
            cases.append(struct.pack("<III", 0, len(z), cap) + z)
            want.append((OK, cap, zlib.crc32(data[:cap])))
    for name in sorted(DAMAGED):
        z, cap, st = DAMAGED[name]
        cases.append(struct.pack("<III", 0, len(z), cap) + z)
        want.append((st, None, None))
    z = deflate(photo_like(300, 9), 9)
    for bit in range(8 * len(z)):
        bad = bytearray(z)
        bad[bit >> 3] ^= 1 << (bit & 7)
        cases.append(struct.pack("<III", 0, len(z), 300) + bytes(bad))
        want.append(None)
    rng = np.random.default_rng(21)
    for ct, depth in O.LEGAL:
        for inter in (False, True):
            s = O.random_samples(rng, 19, 70, ct, depth)
            stream = O.filtered_stream(s, ct, depth, [4, 3, 2, 1, 0], inter)
            cases.append(struct.pack("<IIIIIII", 1, 19, 70, ct, depth, int(inter), len(stream)) + stream)
            want.append((OK, len(stream), None))
    lines = run_under_sanitizers(cases)
    assert len(lines) == len(want)
    for line, w in zip(lines, want):
        st, n, crc = (int(v) for v in line.split())
        if w is None:
            continue
        assert st == w[0], (line, w)
        if w[1] is not None:
            assert n == w[1]
        if w[2] is not None:
            assert crc == w[2]
