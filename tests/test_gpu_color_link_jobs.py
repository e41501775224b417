"""GRAY and LUT-based profiles through the job interface on an MI355X (csrc/shim_decode.cpp Job::color_plan_for): with colour
management on and ifhip_shim_context_set_color_profile_kinds, a grey JPEG or PNG with a grey profile, and a colour JPEG, PNG or
lossless WebP with a lut16 or lutAToB profile, come out as the CPU emulation of the link (tests/color_link_emulation.py) applied
to the very frame the same job decodes under discard_color_profile -- byte for byte.  With the flags off the jobs get the refusal
they always got; discard_color_profile wins; a malformed LUT profile is a ColorProfileError unless told to ignore it; one context
builds a profile's link once."""
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from tests import color_link_emulation as L  # noqa: E402
from tests import color_link_profiles as W  # noqa: E402
from tests import color_profile_emulation as E  # noqa: E402
from tests import png_decode_oracle as O  # noqa: E402
from tests.test_gpu_color_management_jobs import decode_steps, iccp, jpeg, webp  # noqa: E402
from tests.test_jpeg_headers import icc_app2  # noqa: E402

pytestmark = pytest.mark.gpu
GRAY_ICC = W.gray_profile(W.GRAY_TRCS["dotgain"])
MFT2 = W.mft_profile(5, grid=9, in_entries=256, out_entries=256).icc
MAB = W.mab_profile(12, grid=(9, 7, 5), a_curves="para", matrix=True, m_curves="para").icc


def gray_jpeg(w, h, seed, profile):
    from PIL import Image
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.clip((x + y) * 255 // (w + h - 2) + rng.integers(-12, 13, (h, w)), 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(img, "L").save(b, "JPEG", quality=90, optimize=False)
    data = b.getvalue()
    return data[:2] + icc_app2(profile) + data[2:]


def png_of(color_type, w, h, seed, profile):
    return O.write_png(O.random_samples(np.random.default_rng(seed), w, h, color_type, 8, smooth=True), color_type, 8, ancillary=iccp(profile))


def sources():
    """name -> (the file, its profile, whether its frame is grey, the kinds that convert it)"""
    if not hasattr(sources, "made"):
        sources.made = {
            "gray-jpeg": (gray_jpeg(48, 32, 1, GRAY_ICC), GRAY_ICC, True, {"gray": True}),
            "gray-png": (png_of(0, 17, 9, 2, GRAY_ICC), GRAY_ICC, True, {"gray": True}),
            "gray-alpha-png": (png_of(4, 17, 9, 3, GRAY_ICC), GRAY_ICC, True, {"gray": True}),
            "jpeg-mft2": (jpeg(48, 32, 1, MFT2), MFT2, False, {"lut": True}),
            "png-mft2": (png_of(6, 17, 9, 2, MFT2), MFT2, False, {"lut": True}),
            "webp-mft2": (webp(20, 10, 3, MFT2), MFT2, False, {"lut": True}),
            "jpeg-mab": (jpeg(48, 32, 4, MAB), MAB, False, {"lut": True}),
        }
    return sources.made


def run(inputs, steps, switch=False, kinds=None, tell=(), expect=200):
    with Context() as c:
        for io_id, data in inputs.items():
            c.add_input_buffer(io_id, data)
        c.add_output_buffer(9)
        if switch:
            assert c.set_color_management(True) is True
        if kinds is not None:
            assert c.set_color_profile_kinds(**kinds) is True
        for io_id, command in tell:
            assert c.send_json("v1/tell_decoder", {"io_id": io_id, "command": command})[0] == 200
        status, r = c.send_json("v1/execute", {"framewise": {"steps": steps}})
        assert status == expect, (status, r)
        if expect != 200:
            return c.error_code(), r["message"]
        return c.get_output_buffer(9)


def emulated(raw, icc, gray):
    rows, w, h, alpha = unpack_raw_bgra(raw)
    status, link, why = L.link_from_icc(icc, gray)
    assert status == L.PLANNED, why
    return pack_raw_bgra(L.transform(rows, w, link), w, h, alpha_meaningful=alpha)


@pytest.mark.parametrize("name", ["gray-jpeg", "gray-png", "gray-alpha-png", "jpeg-mft2", "png-mft2", "webp-mft2", "jpeg-mab"])
def test_each_source_kind_is_converted_and_refused_with_the_flags_off(name):
    data, icc, gray, kinds = sources()[name]
    as_it_is = run({0: data}, decode_steps("discard_color_profile"))
    want = emulated(as_it_is, icc, gray)
    assert want != as_it_is
    assert run({0: data}, decode_steps(), switch=True, kinds=kinds) == want
    assert run({0: data}, decode_steps("convert_color_profile"), kinds=kinds) == want
    assert run({0: data}, decode_steps(), kinds=kinds, tell=[(0, "convert_color_profile")]) == want
    # the kinds alone switch nothing on, and the other kind's flag does not convert this one
    code, message = run({0: data}, decode_steps(), kinds=kinds, expect=400)
    assert code == 8 and "ifhip_shim_context_set_color_management" in message
    other = {"lut": True} if "gray" in kinds else {"gray": True}
    assert run({0: data}, decode_steps(), switch=True, kinds=other, expect=400) == run({0: data}, decode_steps(), switch=True, expect=400)
    # flags off: the refusal of today, byte for byte
    code, message = run({0: data}, decode_steps(), switch=True, expect=400)
    case = "a GRAY colour space" if gray else "a LUT-based profile (A2B0)"
    what = "carries an embedded ICC profile that is not sRGB"
    assert code == 8 and message == (
        "ActionNotSupported: io_id 0 %s, and the profile is not convertible here: %s (matrix/TRC RGB profiles and gAMA + cHRM are converted; GRAY, "
        "CMYK, Lab and LUT-based profiles and curves that lift black are not).  Tell the decoder \"discard_color_profile\" to decode the samples as they are, or keep the file on "
        "the reference." % (what, case)), message
    # discard_color_profile wins over the switch, the command and the kinds
    assert run({0: data}, decode_steps("discard_color_profile"), switch=True, kinds=kinds) == as_it_is
    assert run({0: data}, decode_steps("convert_color_profile", "discard_color_profile"), kinds=kinds) == as_it_is


def test_a_malformed_lut_profile_is_a_color_profile_error_unless_told_to_ignore_it():
    data = png_of(6, 17, 9, 2, E.a2b0_only_profile())                               # an mAB element with no inputs: refused with the flag off,
    code, message = run({0: data}, decode_steps(), switch=True, expect=400)
    assert code == 8 and "LUT" in message and "not convertible here" in message
    code, message = run({0: data}, decode_steps(), switch=True, kinds={"lut": True}, expect=400)    # malformed with it on
    assert code == 4 and message.startswith("ColorProfileError") and "malformed" in message and "3 inputs" in message and "ignore_color_profile_errors" in message, message
    as_it_is = run({0: data}, decode_steps("discard_color_profile"))
    assert run({0: data}, decode_steps("ignore_color_profile_errors"), switch=True, kinds={"lut": True}) == as_it_is
    cut = jpeg(48, 32, 1, MFT2[:400])                                               # the CLUT runs past the profile's bytes
    code, message = run({0: cut}, decode_steps(), switch=True, kinds={"lut": True}, expect=400)
    assert code == 4 and message.startswith("ColorProfileError"), message


def test_a_profile_that_is_still_not_converted_names_its_case_and_no_longer_lists_its_kind():
    lab = png_of(6, 17, 9, 2, W.mft_profile(9, pcs=b"Lab ", grid=9, in_entries=256, out_entries=2).icc)
    code, message = run({0: lab}, decode_steps(), switch=True, kinds={"lut": True}, expect=400)
    assert code == 8 and "a lut8 or lut16 element with a Lab connection space" in message and "not convertible here" in message, message
    assert "RGB profiles with A2B0 are converted" in message and "LUT-based profiles" not in message and "GRAY, " in message
    gray_lab = png_of(0, 17, 9, 2, W.gray_profile(("gamma", 2.2), pcs=b"Lab "))
    code, message = run({0: gray_lab}, decode_steps(), switch=True, kinds={"gray": True, "lut": True}, expect=400)
    assert code == 8 and "a GRAY profile with a Lab connection space" in message and "GRAY, " not in message, message


def test_two_jobs_on_one_context_build_the_link_once():
    data, icc, gray, kinds = sources()["jpeg-mft2"]
    other = sources()["gray-jpeg"][0]
    outs = []
    with Context() as c:
        assert c.set_color_management(True) and c.set_color_profile_kinds(gray=True, lut=True)
        assert c.color_links_built() == 0
        for k, (io_id, source) in enumerate(((0, data), (1, data), (2, other), (3, sources()["png-mft2"][0]))):
            c.add_input_buffer(io_id, source)
            c.add_output_buffer(10 + io_id)
            status, r = c.send_json("v1/execute", {"framewise": {"steps": [{"decode": {"io_id": io_id}}, {"encode": {"io_id": 10 + io_id, "preset": "gif"}}]}})
            assert status == 200, r
            outs.append(c.get_output_buffer(10 + io_id))
            assert c.color_links_built() == (1, 1, 2, 2)[k]                          # the same profile in another file: the cached link
    assert outs[0] == outs[1] == emulated(run({0: data}, decode_steps("discard_color_profile")), icc, gray)


def test_a_grey_profile_on_a_colour_jpeg_decodes_unconverted_as_ever():
    tagged = jpeg(48, 32, 1, GRAY_ICC)                                              # mozjpeg_decoder.rs:391-395: SourceProfile::Srgb
    plain = run({0: jpeg(48, 32, 1)}, decode_steps())
    assert run({0: tagged}, decode_steps()) == plain
    assert run({0: tagged}, decode_steps(), switch=True, kinds={"gray": True, "lut": True}) == plain


def test_an_rgb_lut_profile_on_a_grey_jpeg_takes_the_rgb_route():
    data = gray_jpeg(48, 32, 1, MFT2)                                               # mozjpeg_decoder.rs:396-403
    as_it_is = run({0: data}, decode_steps("discard_color_profile"))
    assert run({0: data}, decode_steps(), switch=True, kinds={"lut": True}) == emulated(as_it_is, MFT2, True)


def test_a_querystring_job_on_a_lut_tagged_jpeg_takes_the_unfused_path():
    data = sources()["jpeg-mft2"][0]
    qs = [{"command_string": {"kind": "ir4", "value": "w=24&h=16&mode=max", "decode": 0, "encode": 9}}]
    with Context() as c:
        c.add_input_buffer(0, data)
        c.add_output_buffer(9)
        assert c.set_color_management(True) and c.set_color_profile_kinds(lut=True)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": qs}})
        assert status == 200, r
        got = c.get_output_buffer(9)
        assert c.L.ifhip_shim_fused_decode_resamples(c.p) == 0 and c.color_links_built() == 1
    assert unpack_raw_bgra(got)[1:3] == (24, 16)
    plain = run({0: data}, [{"command_string": {"kind": "ir4", "value": "w=24&h=16&mode=max&ignoreicc=true", "decode": 0, "encode": 9}}], switch=True, kinds={"lut": True})
    assert plain != got
