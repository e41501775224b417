"""Colour management through the job interface on an MI355X (csrc/abi_shim.cpp): with the context switch or the decoder command
"convert_color_profile", a JPEG, PNG or lossless WebP whose profile is not sRGB comes out as the CPU emulation of the
conversion (tests/color_profile_emulation.py) applied to the very frame the same job decodes under discard_color_profile --
byte for byte; sRGB sources are untouched; discard_color_profile wins; profiles that are not converted keep the refusal and
name their case; a malformed profile is a ColorProfileError unless the decoder was told to ignore it."""
import io
import struct
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from tests import color_profile_emulation as E  # noqa: E402
from tests import png_decode_oracle as O  # noqa: E402
from tests import vp8l_gen as G  # noqa: E402
from tests import webp_decode_fixtures as X  # noqa: E402
from tests.test_jpeg_headers import P3_XYZ, icc_app2, make_icc  # noqa: E402

pytestmark = pytest.mark.gpu
RAW = {"encode": {"io_id": 9, "preset": "gif"}}                        # (the raw BGRA container: the decoded frame as it is)
P3 = make_icc(xyz=P3_XYZ)
GAMA_CHRM = (45455, (31270, 32900, 68000, 32000, 26500, 69000, 15000, 6000))      # gamma 2.2 with Display P3's primaries


def jpeg(w, h, seed, profile=None):
    from PIL import Image
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) * 255 // (w + h - 2)], -1).astype(np.int16)
    img = np.clip(img + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=90, subsampling="4:2:0", optimize=False)
    data = b.getvalue()
    return data if profile is None else data[:2] + icc_app2(profile) + data[2:]


def png(w, h, seed, ancillary=b""):
    return O.write_png(O.random_samples(np.random.default_rng(seed), w, h, 6, 8, smooth=True), 6, 8, ancillary=ancillary)


def iccp(profile, name=b"profile"):
    return O.chunk(b"iCCP", name + b"\0\0" + zlib.compress(profile))


def gama_chrm(gama=GAMA_CHRM[0], chrm=GAMA_CHRM[1]):
    return O.chunk(b"gAMA", struct.pack(">I", gama)) + O.chunk(b"cHRM", struct.pack(">8I", *chrm))


def webp(w, h, seed, profile=None):
    from PIL import Image
    rng = np.random.default_rng(seed)
    b = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "RGBA").save(b, "WEBP", lossless=True, exact=True)
    payload = X.payload_of(b.getvalue())
    return G.riff(payload) if profile is None else G.riff(payload, vp8x=(0x20 | 0x10, w, h), before=((b"ICCP", profile),))


def sources():
    """name -> (the file tagged as not sRGB, the same file tagged sRGB, the emulation's plan for the first)"""
    if not hasattr(sources, "made"):
        p3_plan = E.plan_from_icc(P3)[1]
        gamma_plan = E.plan_from_gamma_primaries(GAMA_CHRM[0] / 100000, [v / 100000 for v in GAMA_CHRM[1]])[1]
        sources.made = {
            "jpeg": (jpeg(48, 32, 1, P3), jpeg(48, 32, 1, make_icc()), p3_plan),
            "png-iccp": (png(17, 9, 2, iccp(P3)), png(17, 9, 2, iccp(make_icc(), b"sRGB")), p3_plan),
            "png-gama-chrm": (png(17, 9, 2, gama_chrm()), png(17, 9, 2, gama_chrm(45455, (31270, 32900, 64000, 33000, 30000, 60000, 15000, 6000))), gamma_plan),
            "webp": (webp(20, 10, 3, P3), webp(20, 10, 3, make_icc()), p3_plan),
        }
    return sources.made


def run(inputs, steps, switch=False, tell=(), expect=200, outputs=(9,)):
    with Context() as c:
        for io_id, data in inputs.items():
            c.add_input_buffer(io_id, data)
        for io_id in outputs:
            c.add_output_buffer(io_id)
        if switch:
            assert c.set_color_management(True) is True
        for io_id, command in tell:
            assert c.send_json("v1/tell_decoder", {"io_id": io_id, "command": command})[0] == 200
        status, r = c.send_json("v1/execute", {"framewise": {"steps": steps}})
        assert status == expect, (status, r)
        if expect != 200:
            return c.error_code(), r["message"]
        return c.get_output_buffer(outputs[0])


def decode_steps(*commands):
    return [{"decode": {"io_id": 0, "commands": list(commands)}}, RAW]


def emulated(raw, plan):
    """the raw container of a decoded frame with the emulation's conversion applied to its pixels"""
    rows, w, h, alpha = unpack_raw_bgra(raw)
    return pack_raw_bgra(E.transform(rows, w, plan), w, h, alpha_meaningful=alpha)


@pytest.mark.parametrize("name", ["jpeg", "png-iccp", "png-gama-chrm", "webp"])
def test_a_tagged_source_is_converted_with_the_switch_or_the_command(name):
    tagged, srgb, plan = sources()[name]
    as_it_is = run({0: tagged}, decode_steps("discard_color_profile"))
    want = emulated(as_it_is, plan)
    assert want != as_it_is
    assert run({0: tagged}, decode_steps(), switch=True) == want
    assert run({0: tagged}, decode_steps("convert_color_profile")) == want                 # one input, no context switch
    assert run({0: tagged}, decode_steps(), tell=[(0, "convert_color_profile")]) == want
    # an sRGB-tagged copy: identical bytes with the switch on and off
    assert run({0: srgb}, decode_steps(), switch=True) == run({0: srgb}, decode_steps()) == as_it_is
    # discard_color_profile wins over the switch and over the command
    assert run({0: tagged}, decode_steps("discard_color_profile"), switch=True) == as_it_is
    assert run({0: tagged}, decode_steps("convert_color_profile", "discard_color_profile"), switch=True) == as_it_is
    assert run({0: tagged}, decode_steps(), switch=True, tell=[(0, "discard_color_profile")]) == as_it_is
    # off, it is the refusal as ever, and the message names the switch
    code, message = run({0: tagged}, decode_steps(), expect=400)
    assert code == 8 and "discard_color_profile" in message and "ifhip_shim_context_set_color_management" in message and "convert_color_profile" in message


def test_a_querystring_job_on_a_tagged_jpeg_takes_the_unfused_path():
    tagged = jpeg(48, 32, 1, P3)
    qs = [{"command_string": {"kind": "ir4", "value": "w=24&h=16&mode=max", "decode": 0, "encode": 9}}]
    steps = [{"decode": {"io_id": 0}}, {"constrain": {"mode": "within", "w": 24, "h": 16}}, RAW]
    with Context() as c:
        c.add_input_buffer(0, tagged)
        c.add_output_buffer(9)
        assert c.set_color_management(True)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": qs}})
        assert status == 200, r
        got = c.get_output_buffer(9)
        assert c.L.ifhip_shim_fused_decode_resamples(c.p) == 0                             # the frame was formed, converted, then resampled
    assert unpack_raw_bgra(got)[1:3] == (24, 16)
    # the step form: decode (hints as the querystring works them out: none at this ratio are needed for equality of the chain)
    from imageflow_amd import riapi
    commands = riapi.expand_text("w=24&h=16&mode=max", 48, 32)["decoder_commands"]
    steps[0]["decode"]["commands"] = commands
    assert got == run({0: tagged}, steps, switch=True)
    # and the conversion did happen: other bytes than under ignoreicc
    plain = run({0: tagged}, [{"command_string": {"kind": "ir4", "value": "w=24&h=16&mode=max&ignoreicc=true", "decode": 0, "encode": 9}}], switch=True)
    assert plain != got


def test_profiles_that_are_not_converted_keep_the_refusal_and_name_the_case():
    cmyk = jpeg(48, 32, 1, make_icc(space=b"CMYK"))                                         # a CMYK profile on a 3-component file
    code, message = run({0: cmyk}, decode_steps(), switch=True, expect=400)
    assert code == 8 and "CMYK" in message and "not convertible here" in message, message
    lut = png(17, 9, 2, iccp(E.a2b0_only_profile()))
    code, message = run({0: lut}, decode_steps(), switch=True, expect=400)
    assert code == 8 and "LUT" in message and "not convertible here" in message, message
    # told to discard the profile they decode
    assert run({0: cmyk}, decode_steps("discard_color_profile"), switch=True) == run({0: jpeg(48, 32, 1)}, decode_steps())


@pytest.mark.parametrize("name", ["jpeg", "png-iccp", "webp"])
def test_a_truncated_profile_is_a_color_profile_error_unless_told_to_ignore_it(name):
    cut = P3[:200]
    tagged = {"jpeg": lambda: jpeg(48, 32, 1, cut), "png-iccp": lambda: png(17, 9, 2, iccp(cut)), "webp": lambda: webp(20, 10, 3, cut)}[name]()
    code, message = run({0: tagged}, decode_steps(), switch=True, expect=400)
    assert code == 4 and message.startswith("ColorProfileError") and "malformed" in message and "ignore_color_profile_errors" in message, message
    as_it_is = run({0: tagged}, decode_steps("discard_color_profile"))
    assert run({0: tagged}, decode_steps("ignore_color_profile_errors"), switch=True) == as_it_is
    assert run({0: tagged}, decode_steps(), switch=True, tell=[(0, "ignore_color_profile_errors")]) == as_it_is


def test_a_watermark_input_with_a_profile_is_converted_too():
    from tests import util as U
    back = U.random_frames(1, 64, 48, seed0=51, alpha=False)[0]
    tagged, _, plan = sources()["png-iccp"]
    mark = emulated(run({0: tagged}, decode_steps("discard_color_profile")), plan)            # the converted logo, as a raw frame
    steps = [{"decode": {"io_id": 0}}, {"watermark": {"io_id": 1, "fit_mode": "distort", "fit_box": {"image_margins": {"left": 8, "top": 8, "right": 22, "bottom": 22}}}}, RAW]
    inputs = {0: pack_raw_bgra(back, 64, 48, alpha_meaningful=False)}
    want = run({**inputs, 1: mark}, steps)
    assert run({**inputs, 1: tagged}, steps, switch=True) == want
    assert run({**inputs, 1: tagged}, steps, tell=[(1, "convert_color_profile")]) == want
    code, message = run({**inputs, 1: tagged}, steps, expect=400)
    assert code == 8
    # a P3 JPEG as the watermark: its decode would otherwise be fused with the resample
    jmark = jpeg(48, 32, 1, P3)
    jraw = emulated(run({0: jmark}, decode_steps("discard_color_profile")), E.plan_from_icc(P3)[1])
    assert run({**inputs, 1: jmark}, steps, switch=True) == run({**inputs, 1: jraw}, steps)
