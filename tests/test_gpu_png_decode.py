"""The device PNG decoder on an MI355X (csrc/png_read.cpp + csrc/png_decode.hip through imageflow_amd.codecs.libpng_decoder
and the shim's `decode`): files are made at test time with zlib and the small writer of tests/png_decode_oracle.py, which
forces the filter type per row and can interlace; every frame is compared byte for byte with the oracle's BGRA, and the
frame's padding, pre-filled with 0xA5, must come back untouched.  There is no tolerance anywhere.

"Pillow's own choice" of filters exists for the types Pillow writes (gray 1 / 8 / 16, gray + alpha 8, RGB 8, RGBA 8, palette
1 / 2 / 4 / 8; never interlaced); for the other pairs the seventh variant is zlib level 9 on Paeth rows.

The damaged streams are the ones of tests/test_png_decode_core.py, green on the CPU emulation first, with the statuses
that the emulation gives.  Streams that zlib's encoder never writes are in tests/test_gpu_png_inflate_streams.py."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import libpng_decoder as D  # noqa: E402
from imageflow_amd.codecs import libpng_encoder as E  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import png_decode_oracle as O  # noqa: E402
from tests import util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIXED = [4, 0, 3, 1, 2, 4, 4, 3, 1]
PILLOW_MODES = {(0, 1): "1", (0, 8): "L", (0, 16): "I;16", (4, 8): "LA", (2, 8): "RGB", (6, 8): "RGBA", (3, 1): "P", (3, 2): "P", (3, 4): "P", (3, 8): "P"}


def make(rng, ct, depth, w, h, filters=MIXED, interlace=False, smooth=True, **kw):
    s = O.random_samples(rng, w, h, ct, depth, smooth=smooth)
    if ct == 3:
        kw.setdefault("palette", rng.integers(0, 256, (int(rng.integers(1, (1 << depth) + 1)), 3), dtype=np.uint8))
        kw.setdefault("trns", bytes(rng.integers(0, 256, max(1, len(kw["palette"]) // 2), dtype=np.uint8)))
    elif ct == 0:
        kw.setdefault("trns", struct.pack(">H", int(s[h // 2, w // 2, 0])))
    elif ct == 2:
        kw.setdefault("trns", struct.pack(">HHH", *[int(v) for v in s[h // 2, w // 2]]))
    return O.write_png(s, ct, depth, filters=filters, interlace=interlace, **kw)


def pillow_file(rng, ct, depth, w, h):
    """the same kind of file written by Pillow with its own filter choice (None where Pillow does not write the type)"""
    mode = PILLOW_MODES.get((ct, depth))
    if mode is None:
        return None
    buf = io.BytesIO()
    if mode == "P":
        im = Image.fromarray(rng.integers(0, 1 << depth, (h, w), dtype=np.uint8), "P")
        im.putpalette(bytes(rng.integers(0, 256, 3 << depth, dtype=np.uint8)))
        im.save(buf, "PNG", bits=depth)
    elif mode == "1":
        Image.fromarray(rng.integers(0, 2, (h, w), dtype=np.uint8) * 255, "L").convert("1", dither=Image.Dither.NONE).save(buf, "PNG")
    elif mode == "I;16":
        Image.fromarray(rng.integers(0, 65536, (h, w), dtype=np.uint16)).save(buf, "PNG")
    else:
        c = O.CHANNELS[ct]
        a = O.random_samples(rng, w, h, ct, 8, smooth=True).astype(np.uint8)
        Image.fromarray(a[..., 0] if c == 1 else a, mode).save(buf, "PNG")
    data = buf.getvalue()
    info = O.parse(data)
    assert (info["color_type"], info["depth"]) == (ct, depth), (mode, info["color_type"], info["depth"])
    return data


def decode_and_check(files, expect_status=None):
    """one batch; every good file against the oracle, its padding untouched; -> (frames as numpy, status)"""
    frames, status = D.decode_png_batch(files, DEV, fill=0xA5)
    torch.cuda.synchronize()
    out = []
    for i, data in enumerate(files):
        want_st = 0 if expect_status is None else expect_status[i]
        assert status[i] == want_st, (i, status[i], want_st)
        if frames[i] is None:
            out.append(None)
            continue
        got = frames[i].to_numpy()[0]
        w = frames[i].w
        if want_st:
            assert (got == 0xA5).all(), ("a damaged file's frame must stay untouched", i)
        else:
            want, info = O.decode(data)
            assert got.shape[0] == want.shape[0] and w == want.shape[1]
            assert np.array_equal(got[:, :4 * w].reshape(want.shape), want), (i, info["color_type"], info["depth"], info["interlace"], want.shape)
            assert (got[:, 4 * w:] == 0xA5).all(), ("padding", i)
            assert frames[i].alpha_meaningful == info["alpha_used"]
        out.append(got)
    return out, status


@pytest.mark.parametrize("ct,depth", O.LEGAL)
def test_every_type_filter_and_interlace(ct, depth):
    """(colour type, depth) x {none, Adam7} x {each filter forced, mixed per row, Pillow's own choice}; 37 columns (not a multiple
    of 8: the low depths end inside a byte) and 65 rows (a band and one row)."""
    rng = np.random.default_rng(1000 + ct * 20 + depth)
    files = []
    for interlace in (False, True):
        for filters in (0, 1, 2, 3, 4, MIXED):
            files.append(make(rng, ct, depth, 37, 65, filters, interlace))
        own = pillow_file(rng, ct, depth, 37, 65) if not interlace else None
        files.append(own if own is not None else make(rng, ct, depth, 37, 65, 4, interlace, level=9))
    decode_and_check(files)


@pytest.mark.parametrize("ct,depth", O.LEGAL)
def test_edge_sizes(ct, depth):
    rng = np.random.default_rng(2000 + ct * 20 + depth)
    files = [make(rng, ct, depth, w, h, MIXED, interlace) for interlace in (False, True)
             for w, h in ((1, 1), (1, 70), (70, 1), (13, 200), (5, 3), (2, 2), (9, 130), (64, 64), (3, 65))]
    decode_and_check(files)


def test_streams_beyond_the_window_and_beyond_a_mebibyte():
    rng = np.random.default_rng(7)
    noise = make(rng, 6, 8, 600, 500, [0, 1, 2], smooth=False)                      # noise: the stream is as large as the image
    smooth = make(rng, 6, 8, 640, 480, [1, 2, 1, 0], smooth=True)
    photo16 = make(rng, 2, 16, 300, 200, [4, 3, 1], interlace=True)
    gray1 = make(rng, 0, 1, 2000, 1500, [0, 2, 1], smooth=False)
    assert len(O.parse(noise)["idat"]) > 1 << 20 and len(O.parse(photo16)["idat"]) > 32768
    assert O.inflated_size(640, 480, 6, 8, False) > 1 << 20
    decode_and_check([noise, smooth, photo16, gray1])


def test_idat_split_into_one_byte_chunks_and_empty_chunks():
    rng = np.random.default_rng(8)
    files = [make(rng, 6, 8, 21, 17, MIXED, split=1), make(rng, 3, 4, 33, 9, MIXED, interlace=True, split=1), make(rng, 2, 16, 40, 30, 4, split=7),
             make(rng, 0, 8, 50, 50, 2, split=4096)]
    assert files[0].count(b"IDAT") > 100
    decode_and_check(files)


def test_matches_that_reach_the_far_end_of_the_window():
    """Distances in (32768 - 258, 32768]: zlib never writes them, libdeflate, zopfli and 7-zip do.  On the decoder's 32 KiB ring
    such a match reads slots that the same match writes; the streams are the hand-written ones of tests/test_png_decode_core.py."""
    from tests.test_png_decode_core import far_match_stream
    rng = np.random.default_rng(77)
    files = []
    for dist, length in ((32768, 258), (32767, 258), (32700, 258), (32600, 258), (32511, 258), (32510, 258), (32767, 3), (32705, 65)):
        head = b"\0" + rng.integers(0, 256, 32767, dtype=np.uint8).tobytes()            # gray 8, one row: the first byte is the filter type
        data, z = far_match_stream(head, dist, length)
        assert zlib.decompress(z) == data
        files.append(O.write_png(np.zeros((1, len(data) - 1, 1), np.uint32), 0, 8, z=z))
    decode_and_check(files)


def test_an_image_beyond_the_size_limit_is_its_own_files_status():
    """A file whose image would inflate beyond 2^31 bytes gets status 11 like a file that does not parse; the call and the
    neighbour are not disturbed."""
    import ctypes as C
    L = D._bind()
    rng = np.random.default_rng(78)
    good = make(rng, 6, 8, 40, 30)
    huge = bytearray(O.write_png(np.zeros((1, 1, 4), np.uint32), 6, 16))
    huge[16:24] = struct.pack(">II", 30000, 30000)
    huge[29:33] = struct.pack(">I", zlib.crc32(bytes(huge[12:29])))
    bufs = [np.frombuffer(bytes(huge), np.uint8), np.frombuffer(good, np.uint8)]
    frame = torch.full((1, 30 * 192), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    rc = L.ifhip_png_decode_batch_device((C.c_void_p * 2)(*[b.ctypes.data for b in bufs]), (C.c_size_t * 2)(*[b.size for b in bufs]), 2,
                                         (C.c_void_p * 2)(None, frame.data_ptr()), (C.c_size_t * 2)(0, 30 * 192), (C.c_uint32 * 2)(0, 192), status.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and status.cpu().tolist() == [11, 0]
    want, _ = O.decode(good)
    assert np.array_equal(frame.cpu().numpy().reshape(30, 192)[:, :160].reshape(30, 40, 4), want)


def damaged_files():
    from tests.test_png_decode_core import DAMAGED
    files, status = [], []
    for name in sorted(DAMAGED):
        z, cap, st = DAMAGED[name]
        if cap < 2:
            continue
        files.append(O.write_png(np.zeros((1, cap - 1, 1), np.uint32), 0, 8, z=z))       # gray 8, one row: inflates to cap bytes
        status.append(st)
    bad_filter = O.filtered_stream(np.zeros((70, 5, 3), np.uint32), 2, 8, 0)
    bad_filter = bad_filter[:16 * 66] + b"\x05" + bad_filter[16 * 66 + 1:]                # row 66's filter byte
    files.append(O.write_png(np.zeros((70, 5, 3), np.uint32), 2, 8, z=zlib.compress(bad_filter)))
    status.append(10)
    crc = bytearray(O.write_png(np.zeros((4, 4, 3), np.uint32), 2, 8))
    crc[29] ^= 1
    files.append(bytes(crc))
    status.append(11)
    return files, status


def test_one_batch_of_mixed_files_with_damaged_neighbours():
    """Mixed geometries and types in one batch; the same file gives the same bytes in every batch position; damaged files report
    their status, leave their frames untouched and their neighbours decode exactly."""
    rng = np.random.default_rng(9)
    good = [make(rng, ct, depth, int(rng.integers(1, 90)), int(rng.integers(1, 90)), MIXED, bool(i & 1)) for i, (ct, depth) in enumerate(O.LEGAL)]
    probe = make(rng, 6, 16, 57, 41, MIXED, interlace=True)
    bad, bad_status = damaged_files()
    files, status = [probe], [0]
    for i, g in enumerate(good):
        files.append(g)
        status.append(0)
        if i < len(bad):
            files.append(bad[i])
            status.append(bad_status[i])
        if i == 7:
            files.append(probe)
            status.append(0)
    for j in range(len(good), len(bad)):
        files.append(bad[j])
        status.append(bad_status[j])
    files.append(probe)
    status.append(0)
    out, _ = decode_and_check(files, status)
    at = [i for i, f in enumerate(files) if f is probe]
    assert len(at) == 3 and all(np.array_equal(out[at[0]], out[k]) for k in at[1:])
    alone, _ = decode_and_check([probe])
    assert np.array_equal(alone[0], out[at[0]])


def test_round_trip_with_the_device_encoder():
    for alpha in (False, True):
        w, h = 211, 97
        fr = U.random_frames(2, w, h, seed0=31, alpha=True)
        if not alpha:
            fr.reshape(2, h, -1)[:, :, 3:4 * w:4] = 255
        bm = Bitmap.from_numpy(fr, w, h, fr.shape[-1], DEV, alpha_meaningful=alpha)
        files = E.encode_png(bm)
        frames, status = D.decode_png_batch(files, DEV)
        assert status == [0, 0]
        for i in range(2):
            assert frames[i].alpha_meaningful == alpha
            assert np.array_equal(frames[i].to_numpy()[0][:, :4 * w], fr.reshape(2, h, -1)[i][:, :4 * w])


def test_host_drop_in_equals_the_device_form_and_keeps_the_padding():
    rng = np.random.default_rng(12)
    data = make(rng, 4, 16, 45, 33, MIXED, interlace=True)
    want, _ = O.decode(data)
    stride = 4 * 45 + 20
    out = np.full((33, stride), 0x5A, np.uint8)
    D.decode_png_host(data, stride, out)
    assert np.array_equal(out[:, :180].reshape(33, 45, 4), want) and (out[:, 180:] == 0x5A).all()
    bad = O.write_png(np.zeros((1, 9, 1), np.uint32), 0, 8, z=zlib.compress(bytes(10))[:-1] + b"\x55")
    with pytest.raises(Exception) as e:
        D.decode_png_host(bad)
    assert "LibPNG error" in str(e.value)


# ---- jobs (csrc/abi_shim.cpp) ------------------------------------------------------------------------------------------------------
def run_job(inputs, steps, outputs=(9,), expect=200, security=None, tell=None):
    with Context() as c:
        for io_id, data in inputs.items():
            c.add_input_buffer(io_id, data)
        for io_id in outputs:
            c.add_output_buffer(io_id)
        if tell is not None:
            assert c.send_json("v1/tell_decoder", {"io_id": tell, "command": "discard_color_profile"})[0] == 200
        msg = {"framewise": {"steps": steps}}
        if security:
            msg["security"] = security
        status, r = c.send_json("v1/execute", msg)
        assert status == expect, (status, r)
        if expect != 200:
            return c.error_code(), r
        return [c.get_output_buffer(o) for o in outputs], r


def test_decode_png_then_encode_libpng_reproduces_the_pixels():
    rng = np.random.default_rng(13)
    for ct, depth, interlace in ((6, 8, False), (2, 8, True), (3, 4, False), (0, 16, True), (6, 16, False)):
        data = make(rng, ct, depth, 83, 61, MIXED, interlace)
        want, info = O.decode(data)
        outs, r = run_job({0: data}, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": {"libpng": {}}}}])
        got, out_info = O.decode(outs[0])
        if not info["alpha_used"]:                                     # a bgr_32 frame is written as RGB: the alpha bytes are dropped
            assert out_info["color_type"] == 2
            want = want.copy()
            want[..., 3] = 255
        assert np.array_equal(got, want), (ct, depth)
        dec = r["data"]["job_result"]["decodes"][0]
        assert (dec["preferred_mime_type"], dec["preferred_extension"], dec["w"], dec["h"]) == ("image/png", "png", 83, 61)


def test_a_png_logo_watermarks_like_the_same_logo_in_the_raw_container():
    rng = np.random.default_rng(14)
    back = U.random_frames(1, 320, 200, seed0=51, alpha=False)[0]
    logo_png = make(rng, 6, 8, 90, 40, MIXED)
    logo, info = O.decode(logo_png)
    rows = np.zeros((40, U.stride_for(90)), np.uint8)
    rows[:, :360] = logo.reshape(40, 360)
    steps = [{"decode": {"io_id": 0}}, {"watermark": {"io_id": 1, "opacity": 0.7, "gravity": {"percentage": {"x": 100, "y": 100}}}}, {"encode": {"io_id": 9, "preset": "gif"}}]
    base = {0: pack_raw_bgra(back, 320, 200, alpha_meaningful=False)}
    a, _ = run_job({**base, 1: logo_png}, steps)
    b, _ = run_job({**base, 1: pack_raw_bgra(rows, 90, 40, alpha_meaningful=True)}, steps)
    assert a[0] == b[0]
    assert a[0] != run_job(base, [steps[0], steps[2]])[0][0]


def test_a_command_string_job_with_a_png_source():
    rng = np.random.default_rng(15)
    data = make(rng, 2, 8, 400, 300, [1, 2, 4])
    outs, r = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=100", "decode": 0, "encode": 9}}])
    rows, w, h, alpha = unpack_raw_bgra(outs[0])                      # no format named: the raw container, as before
    assert (w, h) == (100, 75) and rows[:, :400].std() > 1
    with Context() as c:                                              # format=png in a querystring stays refused
        c.add_input_buffer(0, data)
        c.add_output_buffer(9)
        status, _ = c.send_json("v1/execute", {"framewise": {"steps": [{"command_string": {"kind": "ir4", "value": "width=100&format=png", "decode": 0, "encode": 9}}]}})
        assert status == 400


def test_max_decode_size_is_enforced_from_the_header():
    huge = O.write_png(np.zeros((1, 1, 3), np.uint32), 2, 8)
    huge = bytearray(huge)
    huge[16:24] = struct.pack(">II", 20000, 20000)                     # the header alone: no such image data behind it
    huge[29:33] = struct.pack(">I", zlib.crc32(bytes(huge[12:29])))
    code, r = run_job({0: bytes(huge)}, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": "gif"}}], expect=400)
    assert code == 2 and "max_decode_size" in r["message"]
    rng = np.random.default_rng(16)
    data = make(rng, 6, 8, 120, 80)
    sec = {"max_decode_size": {"w": 100, "h": 100, "megapixels": 1}}
    code, r = run_job({0: data}, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": "gif"}}], expect=400, security=sec)
    assert code == 2 and "max_decode_size" in r["message"]
    sec = {"max_frame_size": {"w": 100, "h": 100, "megapixels": 1}}
    code, r = run_job({0: data}, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": "gif"}}], expect=400, security=sec)
    assert code == 2 and "max_frame_size" in r["message"]


def test_a_non_srgb_iccp_is_refused_and_decodes_after_discard_color_profile():
    from tests.test_jpeg_headers import P3_XYZ, make_icc
    rng = np.random.default_rng(17)
    s = O.random_samples(rng, 60, 40, 2, 8, smooth=True)
    plain = O.write_png(s, 2, 8, filters=MIXED)
    p3 = O.write_png(s, 2, 8, filters=MIXED, ancillary=O.chunk(b"iCCP", b"Display P3\0\0" + zlib.compress(make_icc(xyz=P3_XYZ))))
    srgb = O.write_png(s, 2, 8, filters=MIXED, ancillary=O.chunk(b"iCCP", b"sRGB\0\0" + zlib.compress(make_icc())))
    steps = [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": "gif"}}]
    want = run_job({0: plain}, steps)[0][0]
    code, r = run_job({0: p3}, steps, expect=400)
    assert code == 8 and "ICC profile" in r["message"] and "discard_color_profile" in r["message"]
    assert run_job({0: p3}, steps, tell=0)[0][0] == want
    assert run_job({0: p3}, [{"decode": {"io_id": 0, "commands": ["discard_color_profile"]}}, steps[1]])[0][0] == want
    assert run_job({0: srgb}, steps)[0][0] == want
    # gAMA + cHRM without an sRGB chunk that are not sRGB: refused in their own words; the specification's sRGB values pass
    gama = O.chunk(b"gAMA", struct.pack(">I", 45455))
    p3 = O.write_png(s, 2, 8, filters=MIXED, ancillary=gama + O.chunk(b"cHRM", struct.pack(">8I", 31270, 32900, 68000, 32000, 26500, 69000, 15000, 6000)))
    code, r = run_job({0: p3}, steps, expect=400)
    assert code == 8 and "gAMA and cHRM" in r["message"] and "ICC profile" not in r["message"] and "discard_color_profile" in r["message"]
    assert run_job({0: p3}, steps, tell=0)[0][0] == want
    srgb = O.write_png(s, 2, 8, filters=MIXED, ancillary=gama + O.chunk(b"cHRM", struct.pack(">8I", 31270, 32900, 64000, 33000, 30000, 60000, 15000, 6000)))
    assert run_job({0: srgb}, steps)[0][0] == want
    damaged = O.write_png(s, 2, 8, z=O.compress(O.filtered_stream(s, 2, 8, MIXED))[:-3])
    code, r = run_job({0: damaged}, steps, expect=400)
    assert code == 4 and "LibPNG error" in r["message"]
