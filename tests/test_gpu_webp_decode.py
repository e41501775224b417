"""The device WebP decoder on an MI355X (csrc/webp_read.cpp + csrc/webp_decode.hip through imageflow_amd.codecs.webp_decoder
and the shim's `decode`): the files of tests/webp_decode_fixtures.py -- Pillow's lossless encoder at the settings that give
each feature, this project's own coder, and the legal streams of tests/vp8l_gen.py that libwebp never writes -- decode byte
for byte to what libwebp (through Pillow) decodes from them, the frame's padding, pre-filled with 0xA5, comes back untouched,
and every damaged file gets its status word and leaves its frame and its neighbours alone.  There is no tolerance anywhere."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import webp_decoder as D  # noqa: E402
from imageflow_amd.codecs import webp_encoder as E  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap, get_stride  # noqa: E402
from tests import png_decode_oracle as PO  # noqa: E402
from tests import util as U  # noqa: E402
from tests import vp8l_gen as G  # noqa: E402
from tests import webp_decode_fixtures as X  # noqa: E402
from tests import webp_frames as F  # noqa: E402
from tests.vp8l_reader import read_vp8l  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOOD = sorted(X.good_files())


def frames_for(files, extra_stride):
    """frames pre-filled with 0xA5 at the default stride plus `extra_stride` bytes (None where the file has no size)"""
    out = []
    for data in files:
        try:
            info = D.webp_info(data)
        except Exception:
            out.append(None)
            continue
        if not info["lossless"]:
            out.append(None)
            continue
        stride = get_stride(info["width"]) + extra_stride
        out.append(Bitmap(torch.full((1, info["height"] * stride), 0xA5, dtype=torch.uint8, device=DEV), info["width"], info["height"], stride,
                          alpha_meaningful=info["has_alpha"]))
    return out


def decode_and_check(names_or_files, extra_stride=0):
    """one batch: (name of a good file | (damaged file, status)) each; good frames against the yardstick, padding untouched"""
    files = [X.good_files()[n] if isinstance(n, str) else n[0] for n in names_or_files]
    frames, status = D.decode_webp_batch(files, DEV, frames=frames_for(files, extra_stride))
    torch.cuda.synchronize()
    for i, n in enumerate(names_or_files):
        if isinstance(n, str):
            want, info = X.expected_bgra(n)
            assert status[i] == 0, (n, status[i])
            got, w = frames[i].to_numpy()[0], frames[i].w
            assert got.shape[0] == want.shape[0] and w == want.shape[1]
            assert np.array_equal(got[:, :4 * w].reshape(want.shape), want), (n, info["transforms"], info["tile_bits"])
            assert (got[:, 4 * w:] == 0xA5).all(), ("padding", n)
            assert frames[i].alpha_meaningful == bool(info["alpha_is_used"])
        else:
            assert status[i] == n[1], (i, status[i], n[1])
            if frames[i] is not None:
                assert (frames[i].to_numpy()[0] == 0xA5).all(), ("a damaged file's frame must stay untouched", i)
    return status


@pytest.mark.parametrize("name", GOOD)
def test_every_good_file_alone(name):
    decode_and_check([name])


@pytest.mark.parametrize("extra_stride", [0, 52])
def test_all_good_files_in_one_batch_of_mixed_sizes_and_transforms(extra_stride):
    decode_and_check(GOOD, extra_stride)


def test_one_batch_of_good_files_with_every_damaged_file_between_them():
    bad = X.damaged_files(library=True)
    for name, (data, _) in bad.items():
        assert X.pillow_refuses(data), name
    batch = []
    for k, name in enumerate(sorted(bad)):
        batch += [GOOD[(3 * k) % len(GOOD)], bad[name]]
    batch.append(GOOD[-1])
    decode_and_check(batch, 12)


def test_host_drop_in_equals_the_batch_form_and_keeps_the_padding():
    for name in ("photo_q100_m6", "gen_predictor_after_indexing", "indexed_4"):
        want = X.expected_bgra(name)[0]
        h, w = want.shape[:2]
        stride = 4 * w + 20
        out = np.full((h, stride), 0x5A, np.uint8)
        D.decode_webp_host(X.good_files()[name], stride, out)
        assert np.array_equal(out[:, :4 * w].reshape(want.shape), want) and (out[:, 4 * w:] == 0x5A).all()
    with pytest.raises(Exception) as e:
        D.decode_webp_host(X.damaged_files()["distance"][0])
    assert "libwebp decoding error" in str(e.value)
    with pytest.raises(Exception) as e:
        D.decode_webp_host(X.damaged_files()["oversubscribed"][0])
    assert "libwebp decoding error" in str(e.value)


def test_round_trip_with_the_device_coder():
    """the webp_frames cases through the device coder and back: the sources, byte for byte (alpha 255 where it means nothing)"""
    files, sources = [], []
    for name, (frame, alpha) in F.cases().items():
        h, w = frame.shape[:2]
        rows = np.zeros((1, h, get_stride(w)), np.uint8)
        rows[0, :, :4 * w] = frame.reshape(h, 4 * w)
        bm = Bitmap.from_numpy(rows, w, h, get_stride(w), DEV, alpha_meaningful=alpha)
        files.append(E.encode_webp_lossless(bm)[0])
        want = frame.copy()
        if not alpha:
            want[..., 3] = 255
        sources.append((name, want, alpha))
    frames, status = D.decode_webp_batch(files, DEV)
    assert status == [0] * len(files)
    for fr, (name, want, alpha) in zip(frames, sources):
        got = fr.to_numpy()[0][:, :4 * fr.w].reshape(want.shape)
        assert np.array_equal(got, want), name
        assert fr.alpha_meaningful == alpha, name


# ---- jobs (csrc/abi_shim.cpp) ------------------------------------------------------------------------------------------------------
def run_job(inputs, steps, outputs=(9,), expect=200, security=None, tell=None):
    with Context() as c:
        for io_id, data in inputs.items():
            c.add_input_buffer(io_id, data)
        for io_id in outputs:
            c.add_output_buffer(io_id)
        for io_id, command in (tell or []):
            assert c.send_json("v1/tell_decoder", {"io_id": io_id, "command": command})[0] == 200
        msg = {"framewise": {"steps": steps}}
        if security:
            msg["security"] = security
        status, r = c.send_json("v1/execute", msg)
        assert status == expect, (status, r)
        if expect != 200:
            return c.error_code(), r
        return [c.get_output_buffer(o) for o in outputs], r


GIF = {"encode": {"io_id": 9, "preset": "gif"}}                      # (the raw BGRA container)


def test_decode_webp_then_encode_libpng_reproduces_the_pixels():
    for name in ("rgba_exact", "photo_q70_m4", "gen_indexing_last"):
        want, info = X.expected_bgra(name)
        outs, r = run_job({0: X.good_files()[name]}, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": {"libpng": {}}}}])
        got, out_info = PO.decode(outs[0])
        if not info["alpha_is_used"]:                                  # a bgr_32 frame is written as RGB: the alpha bytes are dropped
            assert out_info["color_type"] == 2
            want = want.copy()
            want[..., 3] = 255
        assert np.array_equal(got, want), name
        dec = r["data"]["job_result"]["decodes"][0]
        assert (dec["preferred_mime_type"], dec["preferred_extension"], dec["w"], dec["h"]) == ("image/webp", "webp", want.shape[1], want.shape[0])


def test_a_webp_logo_watermarks_like_the_same_logo_in_the_raw_container():
    back = U.random_frames(1, 320, 200, seed0=51, alpha=False)[0]
    logo_webp = X.good_files()["rgba_exact"]
    logo = X.expected_bgra("rgba_exact")[0]
    h, w = logo.shape[:2]
    rows = np.zeros((h, U.stride_for(w)), np.uint8)
    rows[:, :4 * w] = logo.reshape(h, 4 * w)
    steps = [{"decode": {"io_id": 0}}, {"watermark": {"io_id": 1, "opacity": 0.7, "gravity": {"percentage": {"x": 100, "y": 100}}}}, GIF]
    base = {0: pack_raw_bgra(back, 320, 200, alpha_meaningful=False)}
    a, _ = run_job({**base, 1: logo_webp}, steps)
    b, _ = run_job({**base, 1: pack_raw_bgra(rows, w, h, alpha_meaningful=True)}, steps)
    assert a[0] == b[0]
    assert a[0] != run_job(base, [steps[0], steps[2]])[0][0]


def test_a_command_string_job_with_a_webp_source():
    data = X.good_files()["photo_q70_m4"]                              # 150 x 130
    outs, r = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=100", "decode": 0, "encode": 9}}])
    rows, w, h, alpha = unpack_raw_bgra(outs[0])
    assert (w, h) == (100, 87) and rows[:, :400].std() > 1
    code, r = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=100&format=webp", "decode": 0, "encode": 9}}], expect=400)
    assert "ActionNotSupported" in r["message"]
    # the reference hands libwebp's rescaler a size when down.colorspace=srgb and the pre-shrink ratio is below 1: not built
    code, r = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=30&down.colorspace=srgb", "decode": 0, "encode": 9}}], expect=400)
    assert code == 8 and "rescaler" in r["message"]
    outs, _ = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=30", "decode": 0, "encode": 9}}])
    assert unpack_raw_bgra(outs[0])[1:3] == (30, 26)


def test_max_decode_size_is_enforced_from_the_header():
    payload = bytearray(X.payload_of(X.good_files()["1x1"]))
    bits = 15999 | 15999 << 14                                         # 14 bits of width - 1, 14 of height - 1
    payload[1:5] = bits.to_bytes(4, "little")
    huge = G.riff(bytes(payload))                                      # the header alone: no such image data behind it
    code, r = run_job({0: huge}, [{"decode": {"io_id": 0}}, GIF], expect=400)
    assert code == 2 and "max_decode_size" in r["message"]
    data = X.good_files()["photo_q70_m4"]
    sec = {"max_decode_size": {"w": 100, "h": 100, "megapixels": 1}}
    code, r = run_job({0: data}, [{"decode": {"io_id": 0}}, GIF], expect=400, security=sec)
    assert code == 2 and "max_decode_size" in r["message"]
    sec = {"max_frame_size": {"w": 100, "h": 100, "megapixels": 1}}
    code, r = run_job({0: data}, [{"decode": {"io_id": 0}}, GIF], expect=400, security=sec)
    assert code == 2 and "max_frame_size" in r["message"]


def test_a_non_srgb_iccp_is_refused_and_decodes_after_discard_color_profile():
    from tests.test_jpeg_headers import P3_XYZ, make_icc
    payload = X.payload_of(X.good_files()["w17"])
    plain = G.riff(payload)
    p3 = G.riff(payload, vp8x=(0x20, 17, 40), before=((b"ICCP", make_icc(xyz=P3_XYZ)),))
    srgb = G.riff(payload, vp8x=(0x20, 17, 40), before=((b"ICCP", make_icc()),))
    for data in (plain, p3, srgb):
        assert not X.pillow_refuses(data)
    steps = [{"decode": {"io_id": 0}}, GIF]
    want = run_job({0: plain}, steps)[0][0]
    code, r = run_job({0: p3}, steps, expect=400)
    assert code == 8 and "ICC profile" in r["message"] and "discard_color_profile" in r["message"]
    assert run_job({0: p3}, steps, tell=[(0, "discard_color_profile")])[0][0] == want
    assert run_job({0: p3}, [{"decode": {"io_id": 0, "commands": ["discard_color_profile"]}}, steps[1]])[0][0] == want
    assert run_job({0: srgb}, steps)[0][0] == want
    code, r = run_job({0: X.damaged_files()["copy_end"][0]}, steps, expect=400)
    assert code == 4 and "libwebp decoding error" in r["message"]


def test_webp_decoder_hints_need_the_rescaler_unless_they_name_the_files_size():
    data = X.good_files()["w17"]                                       # 17 x 40
    steps = [{"decode": {"io_id": 0}}, GIF]
    want = run_job({0: data}, steps)[0][0]
    code, r = run_job({0: data}, steps, expect=400, tell=[(0, {"webp_decoder_hints": {"width": 9, "height": 20}})])
    assert code == 8 and "rescaler" in r["message"]
    code, r = run_job({0: data}, [{"decode": {"io_id": 0, "commands": [{"webp_decoder_hints": {"width": 9, "height": 20}}]}}, GIF], expect=400)
    assert code == 8 and "rescaler" in r["message"]
    assert run_job({0: data}, steps, tell=[(0, {"webp_decoder_hints": {"width": 17, "height": 40}})])[0][0] == want
    assert run_job({0: data}, steps, tell=[(0, {"jpeg_downscale_hints": {"width": 4, "height": 4}})])[0][0] == want     # accepted and ignored
    png = PO.write_png(np.zeros((5, 7, 3), np.uint32), 2, 8)           # a hint told to another kind of input changes nothing
    a = run_job({0: png}, steps)[0][0]
    assert run_job({0: png}, steps, tell=[(0, {"webp_decoder_hints": {"width": 3, "height": 2}})])[0][0] == a


def test_a_lossy_file_is_image_type_not_supported_and_an_animation_is_malformed():
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(X.smooth_photo(32, 24)).save(buf, "WEBP", quality=60)
    code, r = run_job({0: buf.getvalue()}, [{"decode": {"io_id": 0}}, GIF], expect=400)
    assert code == 5 and "ImageTypeNotSupported" in r["message"] and "lossy" in r["message"]
    buf = io.BytesIO()
    frames = [Image.fromarray(X.smooth_photo(16, 12, s)) for s in (1, 2)]
    frames[0].save(buf, "WEBP", save_all=True, append_images=frames[1:], lossless=True, duration=50)
    code, r = run_job({0: buf.getvalue()}, [{"decode": {"io_id": 0}}, GIF], expect=400)
    assert code == 4 and "UNSUPPORTED_FEATURE" in r["message"]
    code, r = run_job({0: b"GIF89a" + bytes(40)}, [{"decode": {"io_id": 0}}, GIF], expect=400)
    assert code == 5


def test_the_alpha_flag_is_carried_into_the_next_node():
    """bgr_32 / bgra_32: a has_alpha = 0 source re-encoded to webplossless says alpha_is_used = 0, a has_alpha = 1 source 1"""
    for name, flag in (("photo_q0_m0", 0), ("rgba_exact", 1)):
        assert X.expected_bgra(name)[1]["alpha_is_used"] == flag
        outs, _ = run_job({0: X.good_files()[name]}, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": "webplossless"}}])
        rgba, info = read_vp8l(outs[0])
        assert info["alpha_is_used"] == flag, name
        want = X.expected_bgra(name)[0]
        assert np.array_equal(rgba[..., :3], want[..., [2, 1, 0]]), name
