"""The files the lossy WebP decoder's tests share.  Good files: libwebp's own encoder through Pillow (every size once, every
setting once at 130 x 90) and tests/vp8_gen.py's legal key frames with the features that encoder never writes.  Flipped files
(one byte of the token data changed) and cut files (the `VP8 ` payload a few bytes short, sizes patched): libwebp through
Pillow says for each whether it still is an image, and which.  Damaged files: each refused by Pillow, with the status word
the core gives (and the one the library call gives, whose container walk refuses a wrong start code before the frame is read).
There is no tolerance anywhere: Pillow's pixels are the yardstick.  Everything is made once per process, seeded."""
import io
import struct

import numpy as np

from tests import vp8_gen as G
from tests import webp_frames as F
from tests.webp_decode_fixtures import pillow_refuses

OK, CONTAINER, NOT_LOSSY, FRAME_HEADER, PARTITIONS, END_OF_MODES, END_OF_TOKENS, ALPHA_HEADER, ALPHA_STREAM = range(9)
SIZES = [(1, 1), (2, 2), (16, 16), (17, 16), (15, 17), (33, 21), (1, 40), (40, 1), (56, 40), (130, 90), (150, 130)]
_CACHE = {}


def pillow_file(bgra, alpha=False, **settings):
    from PIL import Image, features
    assert features.check("webp"), "Pillow without WebP support"
    im = Image.fromarray(F.rgba_of(bgra), "RGBA")
    buf = io.BytesIO()
    (im if alpha else im.convert("RGB")).save(buf, "WEBP", **settings)
    return buf.getvalue()


def good_files():
    """name -> file bytes"""
    if "good" in _CACHE:
        return _CACHE["good"]
    files = {}
    for w, h in SIZES:
        files["size_%dx%d" % (w, h)] = pillow_file(F.photo(w, h, seed=w + h), quality=70, method=4)
    photo, rgba = F.photo(130, 90), F.photo(130, 90, alpha=True)
    for q in (5, 50, 90, 100):
        files["quality_%d" % q] = pillow_file(photo, quality=q, method=4)
    for m in (0, 6):
        files["method_%d" % m] = pillow_file(photo, quality=60, method=m)
    files["noise"] = pillow_file(F.noise(130, 90), quality=30, method=4)
    files["noise_56x40"] = pillow_file(F.noise(56, 40), quality=70, method=4)     # what the flipped and the cut files are made from
    files["rgba_aq100"] = pillow_file(rgba, True, quality=70, method=4, alpha_quality=100)
    files["rgba_aq40"] = pillow_file(rgba, True, quality=70, method=4, alpha_quality=40)
    files["rgba_exact"] = pillow_file(F.garbage_alpha(photo), True, quality=70, method=4, exact=True)
    files["rgba_56x40"] = pillow_file(F.photo(56, 40, alpha=True), True, quality=70, method=4)
    for name, data in G.option_files().items():
        files["gen_" + name] = data
    _CACHE["good"] = files
    return files


def expected(data):
    """BGRA [h, w, 4] as libwebp decodes the file (alpha 255 where Pillow opens it as RGB), or None where Pillow refuses it"""
    if pillow_refuses(data):
        return None
    rgba, mode = F.pillow_decode(data)
    assert mode in ("RGB", "RGBA"), mode
    return np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])


def expected_bgra(name):
    key = ("want", name)
    if key not in _CACHE:
        _CACHE[key] = expected(good_files()[name])
        assert _CACHE[key] is not None, name
    return _CACHE[key]


def parts(data):
    """(the `VP8 ` payload, the `ALPH` payload or None, w, h) of a file"""
    vp8 = G.chunk_body(data, b"VP8 ")
    w, h = struct.unpack_from("<HH", vp8, 6)
    return vp8, G.chunk_body(data, b"ALPH"), w & 0x3FFF, h & 0x3FFF


def rewrap(data, vp8=None, alph=None):
    old_vp8, old_alph, w, h = parts(data)
    return G.riff(old_vp8 if vp8 is None else vp8, old_alph if alph is None else alph, w, h)


def verdict_files():
    """name -> (file bytes, BGRA or None): 20 single-byte flips in the token data of a 56 x 40 quality-70 file, and that file's
    `VP8 ` payload cut by 1..12 bytes.  Pillow's verdict is the expectation either way.  (The picture is noise: behind a flip
    the decoder reads tokens that were never written, and in a file of a few hundred bytes it nearly always runs off the end.)"""
    if "verdict" in _CACHE:
        return _CACHE["verdict"]
    base = good_files()["noise_56x40"]
    vp8 = parts(base)[0]
    tokens = 10 + ((vp8[0] | vp8[1] << 8 | vp8[2] << 16) >> 5)
    rng = np.random.default_rng(77)
    files = {}
    for k in range(20):
        at = int(rng.integers(tokens, len(vp8)))
        flipped = bytearray(vp8)
        flipped[at] ^= int(rng.integers(1, 256))
        data = rewrap(base, vp8=bytes(flipped))
        files["flip_%02d" % k] = (data, expected(data))
    assert sum(want is not None for _, want in files.values()) >= 12
    for cut in range(1, 13):
        data = rewrap(base, vp8=vp8[:len(vp8) - cut])
        files["cut_%02d" % cut] = (data, expected(data))
    _CACHE["verdict"] = files
    return files


def damaged_files():
    """name -> (file bytes, the core's status word, the library's)"""
    if "bad" in _CACHE:
        return _CACHE["bad"]
    base = good_files()["size_56x40"]
    vp8 = parts(base)[0]

    def tagged(change):
        tag = change(vp8[0] | vp8[1] << 8 | vp8[2] << 16)
        return rewrap(base, vp8=struct.pack("<I", tag)[:3] + vp8[3:])
    files = {
        "not_a_key_frame": (tagged(lambda t: t | 1), FRAME_HEADER, FRAME_HEADER),
        "wrong_start_code": (rewrap(base, vp8=vp8[:3] + b"\x9c" + vp8[4:]), FRAME_HEADER, CONTAINER),
        "show_frame_0": (tagged(lambda t: t & ~0x10), FRAME_HEADER, FRAME_HEADER),
        "profile_4": (tagged(lambda t: (t & ~0xE) | 4 << 1), FRAME_HEADER, FRAME_HEADER),
        "first_partition_beyond_the_chunk": (tagged(lambda t: (t & 0x1F) | len(vp8) << 5), PARTITIONS, PARTITIONS),
    }
    eight = parts(good_files()["gen_partitions_8"])[0]
    first = (eight[0] | eight[1] << 8 | eight[2] << 16) >> 5
    files["partition_table_beyond_the_chunk"] = (rewrap(good_files()["gen_partitions_8"], vp8=eight[:10 + first + 5]), PARTITIONS, PARTITIONS)
    rgba = good_files()["rgba_56x40"]
    alph = parts(rgba)[1]
    assert alph[0] & 3 == 1                                                 # VP8L-coded
    files["alph_compression_2"] = (rewrap(rgba, alph=bytes([(alph[0] & ~3) | 2]) + alph[1:]), ALPHA_HEADER, ALPHA_HEADER)
    files["alph_reserved_bit"] = (rewrap(rgba, alph=bytes([alph[0] | 0x80]) + alph[1:]), ALPHA_HEADER, ALPHA_HEADER)
    files["alph_reserved_low_bit"] = (rewrap(rgba, alph=bytes([alph[0] | 0x40]) + alph[1:]), ALPHA_HEADER, ALPHA_HEADER)
    files["alph_pre_processing_2"] = (rewrap(rgba, alph=bytes([alph[0] | 0x20]) + alph[1:]), ALPHA_HEADER, ALPHA_HEADER)
    files["alph_stream_truncated"] = (rewrap(rgba, alph=alph[:len(alph) // 2]), ALPHA_STREAM, ALPHA_STREAM)
    raw = good_files()["gen_alph_raw_f1"]
    files["alph_raw_short"] = (rewrap(raw, alph=parts(raw)[1][:-1]), ALPHA_STREAM, ALPHA_STREAM)
    _CACHE["bad"] = files
    return files
