"""The device lossy WebP decoder on an MI355X (csrc/vp8_read.cpp + csrc/vp8_decode.hip through
imageflow_amd.codecs.webp_lossy_decoder and, once Context.set_webp_lossy_decoder(True) is told, the shim's `decode`): the files
of tests/webp_lossy_fixtures.py decode byte for byte to what libwebp 1.6.0 (through Pillow) decodes from them, the frame's
padding, pre-filled with 0xA5, comes back untouched, flipped and cut files follow Pillow's verdict either way, and every damaged
file gets its status word and leaves its frame and its neighbours alone.  There is no tolerance anywhere."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import webp_lossy_decoder as D  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap, get_stride  # noqa: E402
from tests import util as U  # noqa: E402
from tests import vp8_gen as G  # noqa: E402
from tests import webp_decode_fixtures as LX  # noqa: E402
from tests import webp_lossy_fixtures as X  # noqa: E402
from tests.vp8l_reader import read_vp8l  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOOD = sorted(X.good_files())


def frames_for(files, extra_stride):
    """frames pre-filled with 0xA5 at the default stride plus `extra_stride` bytes (None where the file gets none)"""
    out = []
    for data in files:
        try:
            info = D.webp_info(data)
        except Exception:
            out.append(None)
            continue
        if info["lossless"] or info["animated"]:
            out.append(None)
            continue
        stride = get_stride(info["width"]) + extra_stride
        out.append(Bitmap(torch.full((1, info["height"] * stride), 0xA5, dtype=torch.uint8, device=DEV), info["width"], info["height"], stride,
                          alpha_meaningful=info["has_alpha"]))
    return out


def decode_and_check(cases, extra_stride=0):
    """one batch of (file, BGRA the yardstick gives | a status word | a tuple of status words): good frames against the
    yardstick with the padding untouched, the others' frames still 0xA5"""
    files = [c[0] for c in cases]
    frames, status = D.decode_webp_lossy_batch(files, DEV, frames=frames_for(files, extra_stride))
    torch.cuda.synchronize()
    for i, (_, want) in enumerate(cases):
        if isinstance(want, np.ndarray):
            assert status[i] == 0, (i, status[i])
            got, w = frames[i].to_numpy()[0], frames[i].w
            assert got.shape[0] == want.shape[0] and w == want.shape[1], i
            assert np.array_equal(got[:, :4 * w].reshape(want.shape), want), i
            assert (got[:, 4 * w:] == 0xA5).all(), ("padding", i)
        else:
            assert status[i] in (want if isinstance(want, tuple) else (want,)), (i, status[i], want)
            if frames[i] is not None:
                assert (frames[i].to_numpy()[0] == 0xA5).all(), ("a damaged file's frame must stay untouched", i)
    return frames, status


def good(name):
    return X.good_files()[name], X.expected_bgra(name)


@pytest.mark.parametrize("name", GOOD)
def test_every_good_file_alone(name):
    frames, _ = decode_and_check([good(name)])
    assert frames[0].alpha_meaningful == (X.parts(X.good_files()[name])[1] is not None)


@pytest.mark.parametrize("extra_stride", [0, 52])
def test_all_good_files_in_one_batch_of_mixed_sizes(extra_stride):
    decode_and_check([good(n) for n in GOOD], extra_stride)


def test_one_batch_with_every_damaged_cut_and_flipped_file_between_good_ones():
    refused = (X.PARTITIONS, X.END_OF_MODES, X.END_OF_TOKENS)
    others = [(data, status) for _, (data, _, status) in sorted(X.damaged_files().items())]
    others += [(data, want if want is not None else refused) for _, (data, want) in sorted(X.verdict_files().items())]
    others.append((LX.good_files()["w17"], X.NOT_LOSSY))                    # a lossless file: not this decoder's, and it gets no frame
    others.append((b"neither RIFF nor WEBP", X.CONTAINER))
    for name, (data, _, _) in X.damaged_files().items():
        assert X.pillow_refuses(data), name
    batch = []
    for k, case in enumerate(others):
        batch += [good(GOOD[(5 * k) % len(GOOD)]), case]
    batch.append(good(GOOD[-1]))
    frames, status = decode_and_check(batch, 12)
    assert frames[2 * len(others) - 3] is None and frames[2 * len(others) - 1] is None     # the lossless file and the one that is no WebP


def test_host_drop_in_equals_the_device_form_and_keeps_the_padding():
    for name in ("size_150x130", "rgba_aq40", "gen_simple_filter", "gen_alph_vp8l_f3", "size_1x1"):
        want = X.expected_bgra(name)
        h, w = want.shape[:2]
        stride = 4 * w + 20
        out = np.full((h, stride), 0x5A, np.uint8)
        D.decode_webp_lossy_host(X.good_files()[name], stride, out)
        assert np.array_equal(out[:, :4 * w].reshape(want.shape), want) and (out[:, 4 * w:] == 0x5A).all(), name
    for name in ("alph_stream_truncated", "show_frame_0", "partition_table_beyond_the_chunk"):
        with pytest.raises(Exception) as e:
            D.decode_webp_lossy_host(X.damaged_files()[name][0])
        assert "libwebp decoding error" in str(e.value), name
    with pytest.raises(Exception) as e:
        D.decode_webp_lossy_host(LX.good_files()["w17"])
    assert "not a lossy WebP" in str(e.value)
    with pytest.raises(Exception) as e:
        D.decode_webp_lossy(X.damaged_files()["profile_4"][0], DEV)
    assert "frame_header" in str(e.value)


# ---- jobs (csrc/abi_shim.cpp) ------------------------------------------------------------------------------------------------------
def run_job(inputs, steps, outputs=(9,), expect=200, tell=None, lossy=True, color=False, security=None):
    with Context() as c:
        if lossy:
            assert c.set_webp_lossy_decoder(True)
        if color:
            assert c.set_color_management(True)
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


RAW = {"encode": {"io_id": 9, "preset": "gif"}}                      # (the raw BGRA container)


def test_get_image_info_answers_for_a_lossy_file_once_switched_on():
    for name, fmt in (("rgba_56x40", "bgra_32"), ("size_56x40", "bgr_32")):
        with Context() as c:
            assert c.set_webp_lossy_decoder(True)
            c.add_input_buffer(0, X.good_files()[name])
            for method in ("v1/get_image_info", "v1/get_scaled_image_info"):
                status, r = c.send_json(method, {"io_id": 0})
                assert status == 200, r
                assert r["data"]["image_info"] == {"preferred_mime_type": "image/webp", "preferred_extension": "webp", "image_width": 56, "image_height": 40,
                                                   "frame_decodes_into": fmt}
        with Context() as c:                                          # off, as it is by default: the refusal and its wording stay
            c.add_input_buffer(0, X.good_files()[name])
            status, r = c.send_json("v1/get_image_info", {"io_id": 0})
            assert status == 400 and c.error_code() == 5 and "lossy" in c.error_message()[0]


def test_decode_then_encode_webplossless_reproduces_libwebps_pixels_and_alpha_flag():
    for name, flag in (("size_150x130", 0), ("rgba_aq40", 1), ("gen_alph_raw_f3", 1), ("gen_segments_delta", 0)):
        want = X.expected_bgra(name)
        outs, r = run_job({0: X.good_files()[name]}, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": "webplossless"}}])
        rgba, info = read_vp8l(outs[0])
        assert info["alpha_is_used"] == flag, name
        assert np.array_equal(rgba[..., :3], want[..., [2, 1, 0]]), name
        if flag:
            assert np.array_equal(rgba[..., 3], want[..., 3]), name
        dec = r["data"]["job_result"]["decodes"][0]
        assert (dec["preferred_mime_type"], dec["preferred_extension"], dec["w"], dec["h"]) == ("image/webp", "webp", want.shape[1], want.shape[0])


def test_a_lossy_logo_watermarks_like_the_same_logo_in_the_raw_container():
    back = U.random_frames(1, 320, 200, seed0=51, alpha=False)[0]
    logo = X.expected_bgra("rgba_56x40")
    h, w = logo.shape[:2]
    rows = np.zeros((h, U.stride_for(w)), np.uint8)
    rows[:, :4 * w] = logo.reshape(h, 4 * w)
    steps = [{"decode": {"io_id": 0}}, {"watermark": {"io_id": 1, "opacity": 0.7, "gravity": {"percentage": {"x": 100, "y": 100}}}}, RAW]
    base = {0: pack_raw_bgra(back, 320, 200, alpha_meaningful=False)}
    a, _ = run_job({**base, 1: X.good_files()["rgba_56x40"]}, steps)
    b, _ = run_job({**base, 1: pack_raw_bgra(rows, w, h, alpha_meaningful=True)}, steps)
    assert a[0] == b[0]
    assert a[0] != run_job(base, [steps[0], steps[2]])[0][0]


def test_a_command_string_job_with_a_lossy_source():
    data = X.good_files()["size_150x130"]
    outs, _ = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=100", "decode": 0, "encode": 9}}])
    rows, w, h, alpha = unpack_raw_bgra(outs[0])
    assert (w, h) == (100, 87) and rows[:, :400].std() > 1
    code, r = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=30&down.colorspace=srgb", "decode": 0, "encode": 9}}], expect=400)
    assert code == 8 and "rescaler" in r["message"]


def test_hints_limits_profiles_and_damage_go_the_lossless_branchs_way():
    from tests.test_jpeg_headers import P3_XYZ, make_icc
    data = X.good_files()["size_33x21"]
    steps = [{"decode": {"io_id": 0}}, RAW]
    want = run_job({0: data}, steps)[0][0]
    rows, w, h, alpha = unpack_raw_bgra(want)
    assert (w, h, alpha) == (33, 21, False) and np.array_equal(rows[:, :4 * w].reshape(h, w, 4)[..., :3], X.expected_bgra("size_33x21")[..., :3])
    code, r = run_job({0: data}, steps, expect=400, tell=[(0, {"webp_decoder_hints": {"width": 9, "height": 20}})])
    assert code == 8 and "rescaler" in r["message"]
    assert run_job({0: data}, steps, tell=[(0, {"webp_decoder_hints": {"width": 33, "height": 21}})])[0][0] == want
    code, r = run_job({0: data}, steps, expect=400, security={"max_decode_size": {"w": 20, "h": 20, "megapixels": 1}})
    assert code == 2 and "max_decode_size" in r["message"]
    vp8 = X.parts(data)[0]
    p3, srgb = G.riff(vp8, None, 33, 21, iccp=make_icc(xyz=P3_XYZ)), G.riff(vp8, None, 33, 21, iccp=make_icc())
    for tagged in (p3, srgb):
        assert not X.pillow_refuses(tagged)
    assert run_job({0: srgb}, steps)[0][0] == want
    code, r = run_job({0: p3}, steps, expect=400)
    assert code == 8 and "ICC profile" in r["message"] and "discard_color_profile" in r["message"]
    assert run_job({0: p3}, steps, tell=[(0, "discard_color_profile")])[0][0] == want
    converted = run_job({0: p3}, steps, color=True)[0][0]
    assert converted != want and unpack_raw_bgra(converted)[1:3] == (33, 21)
    for name in ("alph_stream_truncated", "first_partition_beyond_the_chunk", "not_a_key_frame"):
        code, r = run_job({0: X.damaged_files()[name][0]}, steps, expect=400)
        assert code == 4 and "ImageMalformed: libwebp decoding error" in r["message"], name


def test_with_the_switch_off_a_lossy_file_is_still_image_type_not_supported():
    code, r = run_job({0: X.good_files()["size_33x21"]}, [{"decode": {"io_id": 0}}, RAW], expect=400, lossy=False)
    assert code == 5 and "ImageTypeNotSupported" in r["message"] and "lossy" in r["message"]
