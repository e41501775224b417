"""The C ABI of the device WebP decoder without a GPU: the header and the Rust bindings declare ifhip_webp_info,
ifhip_webp_decode_batch_device and ifhip_webp_decode and the library exports them; ifhip_webp_info answers every container
case the way libwebp does through Pillow -- has_alpha pinned to Pillow's mode where the VP8X ALPHA flag and the VP8L header
bit disagree, RIFF sizes beyond and inside the buffer, chunk order, padding -- and reports lossy files, animations and the
ICC verdict; argument and frame checks come before the device check; the kernels stay out of scratch memory and hold the
LDS DESIGN 4.13 states; and through the shim v1/get_image_info answers for a WebP."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd import build as B  # noqa: E402
from imageflow_amd.abi import Context  # noqa: E402
from imageflow_amd.codecs import webp_decoder as W  # noqa: E402
from imageflow_amd.errors import ErrorKind, FlowError  # noqa: E402
from tests import vp8l_gen as G  # noqa: E402
from tests import webp_decode_fixtures as X  # noqa: E402
from tests.test_kernel_resources import resource_usage, _int  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ifhip_webp_info", "ifhip_webp_decode_batch_device", "ifhip_webp_decode"]
INVALID = int(ErrorKind.InvalidArgument)


def payloads():
    with_alpha, _ = G.write_payload(1, 20, 10, alpha=1, opts={"alpha": 1})
    without, _ = G.write_payload(1, 20, 10, alpha=0, opts={"alpha": 1})
    return with_alpha, without


def pillow_mode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im.mode, im.size


def test_header_declares_and_library_exports_the_webp_decode_entries():
    header = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop.rs")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert re.search(r"IFHIP_API [^;]*\b%s\(" % name, header), name
        assert re.search(r"\bfn %s\(" % name, bindings), name
        assert getattr(L, name) is not None
    assert "pub struct ifhip_webp_file_info" in bindings
    for word, value in zip(("TRUNCATED", "CODE_LENGTHS", "BAD_CODE", "DISTANCE", "COPY_END", "CACHE_SYMBOL", "TRANSFORM", "TOO_LITTLE", "CONTAINER"), range(1, 10)):
        assert re.search(r"#define IFHIP_WEBP_DEC_%s %d\b" % (word, value), header), word
        assert W.STATUS[value] == word.lower()


def test_has_alpha_is_pillows_mode_whatever_the_vp8x_flag_says():
    with_alpha, without = payloads()
    for payload, mode in ((with_alpha, "RGBA"), (without, "RGB")):
        for wrap in (lambda p: G.riff(p), lambda p: G.riff(p, vp8x=(0x00, 20, 10)), lambda p: G.riff(p, vp8x=(0x10, 20, 10))):
            data = wrap(payload)
            assert pillow_mode(data) == (mode, (20, 10))
            info = W.webp_info(data)
            assert info["has_alpha"] is (mode == "RGBA") and info["frame_decodes_into"] == ("bgra_32" if mode == "RGBA" else "bgr_32")
            assert (info["width"], info["height"], info["lossless"], info["animated"], info["color_kind"]) == (20, 10, True, False, 0)


def test_every_container_case_goes_the_way_libwebp_goes():
    pa, _ = payloads()
    odd = pa if len(pa) & 1 else pa + b"\0"                            # a payload of odd length: the chunk carries a padding byte
    accepted = {
        "bare": G.riff(pa),
        "odd payload": G.riff(odd),
        "bytes behind the RIFF size": G.riff(pa) + b"xyz",
        "vp8x with unknown chunks around": G.riff(pa, vp8x=(0x10, 20, 10), before=((b"ABCD", b"123"),), after=((b"EXIF", b"Exif\0\0"), (b"XMP ", b"<x/>"), (b"WXYZ", b"1"))),
        "icc flag without a chunk": G.riff(pa, vp8x=(0x30, 20, 10)),
        "iccp behind the image": G.riff(pa, vp8x=(0x30, 20, 10), after=((b"ICCP", b"x" * 200),)),
    }
    refused = {
        "riff size one short": G.riff(pa, riff_delta=-1 - (len(pa) & 1)),
        "riff size cuts the chunk": G.riff(pa, riff_delta=-9),
        "riff size beyond the buffer": G.riff(pa, riff_delta=2),
        "riff size far beyond": G.riff(pa, riff_delta=100),
        "bigger riff size with bytes behind": G.riff(pa, riff_delta=4) + b"xy",
        "padding byte missing": G.riff(odd)[:-1],
        "cut short": G.riff(pa)[:-7],
        "unknown chunk first without vp8x": G.riff(pa, before=((b"ABCD", b"123"),)),
        "two image chunks": G.riff(pa, vp8x=(0x10, 20, 10), after=((b"VP8L", pa),)),
        "canvas of another size": G.riff(pa, vp8x=(0x10, 21, 10)),
        "vp8x without an image": G.riff(pa, vp8x=(0x10, 20, 10), payload_tag=b"ABCD"),
        "signature": G.riff(b"\x2e" + pa[1:]),
        "version": G.riff(pa[:4] + bytes([pa[4] | 0x20]) + pa[5:]),
        "riff only": b"RIFF\x04\0\0\0WEBP",
    }
    for name, data in accepted.items():
        assert not X.pillow_refuses(data), name
        assert W.webp_info(data)["width"] == 20, name
    for name, data in refused.items():
        assert X.pillow_refuses(data), name
        with pytest.raises(FlowError) as e:
            W.webp_info(data)
        assert "ImageMalformed" in str(e.value), name
    with pytest.raises(FlowError):
        W.webp_info(b"\x89PNG\r\n\x1a\n" + bytes(20))


def test_lossy_animated_and_icc_answers():
    from PIL import Image
    from tests.test_jpeg_headers import P3_XYZ, make_icc
    buf = io.BytesIO()
    Image.fromarray(X.smooth_photo(33, 21)).save(buf, "WEBP", quality=60)
    info = W.webp_info(buf.getvalue())
    assert (info["width"], info["height"], info["lossless"], info["animated"], info["has_alpha"]) == (33, 21, False, False, False)
    buf = io.BytesIO()
    Image.fromarray(np.dstack([X.smooth_photo(33, 21), np.arange(33 * 21, dtype=np.uint8).reshape(21, 33)]), "RGBA").save(buf, "WEBP", quality=60)
    info = W.webp_info(buf.getvalue())
    assert b"ALPH" in buf.getvalue() and (info["width"], info["height"], info["lossless"], info["has_alpha"]) == (33, 21, False, True)
    buf = io.BytesIO()
    frames = [Image.fromarray(X.smooth_photo(16, 12, s)) for s in (1, 2)]
    frames[0].save(buf, "WEBP", save_all=True, append_images=frames[1:], lossless=True, duration=50)
    info = W.webp_info(buf.getvalue())
    assert (info["width"], info["height"], info["animated"], info["lossless"]) == (16, 12, True, False)
    pa, _ = payloads()
    for profile, flags, want in ((make_icc(), 0x30, 1), (make_icc(xyz=P3_XYZ), 0x30, 2), (b"x" * 200, 0x30, 2), (make_icc(xyz=P3_XYZ), 0x10, 0)):
        data = G.riff(pa, vp8x=(flags, 20, 10), before=((b"ICCP", profile),))
        assert not X.pillow_refuses(data)
        from PIL import Image as I
        assert bool(I.open(io.BytesIO(data)).info.get("icc_profile")) == (want != 0)      # the demuxer shows a profile only under the flag
        assert W.webp_info(data)["color_kind"] == want, (flags, want)


def test_argument_and_frame_checks_come_before_the_device_check():
    """Without a GPU: a bad stride and a short frame are argument errors, a well-formed call reaches the device check.  (The
    pointers are made up, so this must never run where a kernel could be launched.)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present: the made-up pointers below must not reach a kernel")
    L = W._bind()
    data = X.good_files()["w17"]
    buf = np.frombuffer(data, np.uint8)
    WD, H, STRIDE = 17, 40, 4 * 17 + 8
    status = 0x7F0000200000

    def call(frame_bytes, stride, frame=0x7F0000000000, files=None, n=1):
        ptrs, lens = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(buf.size)
        frames, fb, st = (C.c_void_p * 1)(frame), (C.c_size_t * 1)(frame_bytes), (C.c_uint32 * 1)(stride)
        return L.ifhip_webp_decode_batch_device(ptrs if files is None else files, lens, n, frames, fb, st, status, None)
    assert call(H * STRIDE, 4 * WD - 4) == INVALID
    assert call(H * STRIDE, STRIDE + 2) == INVALID
    assert call((H - 1) * STRIDE + 4 * WD - 4, STRIDE) == INVALID
    assert call(H * STRIDE, STRIDE, frame=0x7F0000000002) == INVALID
    assert call(H * STRIDE, STRIDE, frame=None) == INVALID
    assert call(H * STRIDE, STRIDE, files=0) == INVALID
    assert call(H * STRIDE, STRIDE, n=0) == 0
    assert call(H * STRIDE, STRIDE) in (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
    out, st = np.zeros(H * STRIDE, np.uint8), C.c_uint32(0)
    assert L.ifhip_webp_decode(buf.ctypes.data, buf.size, out.ctypes.data, 4 * WD - 4, out.size, C.byref(st)) == INVALID
    assert L.ifhip_webp_decode(buf.ctypes.data, buf.size, out.ctypes.data, STRIDE, H * STRIDE - 200, C.byref(st)) == INVALID
    assert L.ifhip_webp_decode(buf.ctypes.data, 30, out.ctypes.data, STRIDE, out.size, C.byref(st)) == INVALID
    assert b"ImageMalformed" in L.ifhip_last_error_message()
    bad = np.frombuffer(X.damaged_files()["transform_twice"][0], np.uint8)          # what the host prepare finds needs no device either
    big = np.zeros(1 << 16, np.uint8)
    assert L.ifhip_webp_decode(bad.ctypes.data, bad.size, big.ctypes.data, 4 * 30, big.size, C.byref(st)) == INVALID and st.value == X.TRANSFORM
    assert L.ifhip_webp_decode(buf.ctypes.data, buf.size, out.ctypes.data, STRIDE, out.size, C.byref(st)) in (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))


def test_webp_decode_kernels_use_no_scratch_and_hold_the_lds_of_the_design_table():
    rows = resource_usage(os.path.join(B.CSRC, "webp_decode.hip"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("webp_pixels_kernel", "webp_transform_kernel"):
        r = rows[name]
        assert _int(r, "ScratchSize [bytes/lane]") == 0, (name, r)
        assert _int(r, "LDS Size [bytes/block]") <= 160 * 1024, (name, r)
        assert _int(r, "VGPRs") <= 512, (name, r)
        m = re.search(r"\| `%s` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|" % name, design)      # lanes, VGPRs, LDS bytes, scratch
        assert m, name
        assert int(m.group(3)) == _int(r, "LDS Size [bytes/block]") and int(m.group(4)) == 0, (name, m.groups(), r)
    assert _int(rows["webp_pixels_kernel"], "LDS Size [bytes/block]") <= 32 * 1024          # five waves per CU
    assert _int(rows["webp_transform_kernel"], "LDS Size [bytes/block]") == 0


def test_shim_get_image_info_on_a_webp():
    with_alpha, without = payloads()
    for data, fmt in ((G.riff(with_alpha), "bgra_32"), (G.riff(without, vp8x=(0x10, 20, 10)), "bgr_32")):
        with Context() as c:
            c.add_input_buffer(0, data)
            for method in ("v1/get_image_info", "v1/get_scaled_image_info"):
                if method.endswith("scaled_image_info"):                # the JPEG hints are accepted and ignored
                    assert c.send_json("v1/tell_decoder", {"io_id": 0, "command": {"jpeg_downscale_hints": {"width": 4, "height": 4}}})[0] == 200
                    assert c.send_json("v1/tell_decoder", {"io_id": 0, "command": {"webp_decoder_hints": {"width": 4, "height": 4}}})[0] == 200
                status, r = c.send_json(method, {"io_id": 0})
                assert status == 200, r
                assert r["data"]["image_info"] == {"preferred_mime_type": "image/webp", "preferred_extension": "webp", "image_width": 20, "image_height": 10,
                                                   "frame_decodes_into": fmt}
    with Context() as c:
        c.add_input_buffer(0, G.riff(with_alpha)[:-7])
        status, r = c.send_json("v1/get_image_info", {"io_id": 0})
        assert status == 400 and c.error_code() == 4
        assert "libwebp decoding error" in c.error_message()[0]
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(X.smooth_photo(33, 21)).save(buf, "WEBP", quality=60)
    with Context() as c:                                              # lossy VP8 is not built: ImageTypeNotSupported, in its own words
        c.add_input_buffer(0, buf.getvalue())
        status, r = c.send_json("v1/get_image_info", {"io_id": 0})
        assert status == 400 and c.error_code() == 5 and "lossy" in c.error_message()[0]
    with Context() as c:                                              # a hint without sizes is accepted and holds nothing, as it always was
        c.add_input_buffer(0, G.riff(with_alpha))
        for command in ({"webp_decoder_hints": {}}, {"webp_decoder_hints": {"width": "x"}}, {"webp_decoder_hints": None}):
            assert c.send_json("v1/tell_decoder", {"io_id": 0, "command": command})[0] == 200
        assert c.send_json("v1/tell_decoder", {"io_id": 0, "command": {"no_such_command": {}}})[0] == 400
    with Context() as c:                                              # GIF input stays ImageTypeNotSupported
        c.add_input_buffer(0, b"GIF89a" + bytes(40))
        status, r = c.send_json("v1/execute", {"framewise": {"steps": [{"decode": {"io_id": 0}}]}})
        assert status == 400 and c.error_code() == 5
