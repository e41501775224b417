"""Animated GIFs on an MI355X: every composed screen of a file in one pass (ifhip_gif_decode_frames_device) against the oracle
and against today's select_frame = k; N frames into one file (ifhip_gif_encode_animation_device) against the assembly of the
one-frame coder's emulation, byte for byte -- chunked stages, bodies at every byte of a dword, a short capacity, a side
stream; and jobs on a context with both switches on (Context.set_gif_animation, Context.set_gif_encoder): every frame
decoded, run and written, every other job byte for byte what it is with the switch off.  There is no tolerance anywhere."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import gif_decoder as D  # noqa: E402
from imageflow_amd.codecs import gif_encoder as GIF  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap, get_stride  # noqa: E402
from tests import gif_animation_emu as A  # noqa: E402
from tests import gif_encode_emu as G  # noqa: E402
from tests import gif_fixtures as X  # noqa: E402
from tests import gif_gen  # noqa: E402
from tests import gif_oracle as O  # noqa: E402
from tests import png_decode_oracle as PO  # noqa: E402
from tests import png_quantize_emu as Q  # noqa: E402
from tests.test_gif_animation_core import animations, seventy_frames  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILES = dict(animations(), seventy=seventy_frames())


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------

def screens_of(bitmap):
    rows = bitmap.to_numpy()
    return rows[:, :, :4 * bitmap.w].reshape(bitmap.n, bitmap.h, bitmap.w, 4)


@pytest.mark.parametrize("name", sorted(FILES))
def test_decode_gif_frames_gives_the_oracles_screens_and_todays_select_frame(name):
    data = FILES[name]
    P = O.parse(data, 1 << 30)
    screens, delays = D.decode_gif_frames(data, DEV)
    assert screens.n == P["frames_seen"] and delays == [f["delay"] for f in P["frames"]]
    got = screens_of(screens)
    for k in range(screens.n):
        assert np.array_equal(got[k], O.compose(P, k)), (name, k)
    ks = range(screens.n) if name != "seventy" else (0, 1, 35, 69)
    today, status = D.decode_gif_batch([data] * len(ks), list(ks), DEV)
    assert status == [0] * len(ks)
    for k, one in zip(ks, today):
        assert np.array_equal(screens_of(one)[0], got[k]), (name, k)


def test_a_damaged_middle_frame_writes_nothing_and_reports_the_status():
    good = gif_gen.frame(gif_gen.runs(61, 47, 16, 70), 61, 47, m=4)
    stream = gif_gen.lzw_stream(gif_gen.runs(61, 47, 16, 70).ravel(), 4)
    data = gif_gen.gif(61, 47, [good, gif_gen.frame(None, 61, 47, m=4, stream=stream[:50]), good], palette=gif_gen.palette_of(16))
    assert D.gif_frame_count(data)[0] == 3                                      # the host walk sees nothing wrong
    screens, delays, status = D.decode_gif_frames(data, DEV, fill=0xA5, with_status=True)
    assert status == O.TOO_LITTLE and delays == []
    assert (screens.data.cpu().numpy() == 0xA5).all(), "no screen is written"
    with pytest.raises(Exception) as e:
        D.decode_gif_frames(data, DEV)
    assert "ImageMalformed" in str(e.value)


def test_a_stride_with_padding_keeps_the_padding():
    data = FILES["dispose_mixed"]
    stride = get_stride(12) + 16
    screens, _ = D.decode_gif_frames(data, DEV, stride=stride, fill=0xA5)
    rows = screens.to_numpy()
    assert rows.shape == (3, 9, stride) and (rows[:, :, 4 * 12:] == 0xA5).all()
    assert np.array_equal(screens_of(screens), A.decode_frames(data)[1])


# ---- the coder -----------------------------------------------------------------------------------------------------------------------

def bitmap_of(frames, alpha, stride=None):
    h, w, _ = frames[0].shape
    rows = np.ascontiguousarray(np.stack([Q.bgra_rows(f, stride) for f in frames]))
    return Bitmap.from_numpy(rows, w, h, rows.shape[-1], DEV, alpha_meaningful=alpha)


def device_animation(frames, alpha, delays, user, repeat, max_images, **kw):
    h, w, _ = frames[0].shape
    stage = GIF.GifEncodeStage(w, h, max_images, DEV)
    return stage.encode_animation(bitmap_of(frames, alpha), delays, user, repeat, **kw)


def test_three_frames_with_alpha_equal_the_emulations_file():
    frames = A.photo_frames(17, 40, 3, True, seed=3)
    want, _ = A.assemble(frames, True, [4, 0, 250], [False, True, False], repeat=2)
    assert device_animation(frames, True, [4, 0, 250], [False, True, False], 2, 3) == want


def test_five_frames_through_a_stage_of_two_images():
    frames = A.photo_frames(17, 40, 5, True, seed=11)
    delays, user = [1, 2, 3, 4, 5], [True, False, False, True, False]
    want, _ = A.assemble(frames, True, delays, user, repeat=0)
    assert device_animation(frames, True, delays, user, 0, 2) == want             # chunks of 2, 2, 1
    assert device_animation(frames, True, delays, user, 0, 5) == want


def test_bodies_that_share_dwords_and_a_capacity_one_byte_short():
    frames = A.residue_frames()
    delays, user = list(range(len(frames))), [k % 2 == 1 for k in range(len(frames))]
    want, per_frame = A.assemble(frames, False, delays, user, repeat=0)
    assert {n % 4 for n in A.body_lengths(per_frame)} == {0, 1, 2, 3}
    for max_images in (1, 3, len(frames)):
        assert device_animation(frames, False, delays, user, 0, max_images) == want, max_images
    assert device_animation(frames, False, delays, user, 0, 3, capacity=len(want), with_status=True) == (want, 0)
    assert device_animation(frames, False, delays, user, 0, 3, capacity=len(want) - 1, with_status=True) == (None, GIF.GIF_FILE_OVERFLOW)


def test_one_frame_is_the_one_frame_coders_file():
    f = A.photo_frames(17, 40, 1, True, seed=9)
    want = G.encode(f[0], alpha=True, repeat=7, delay=12, user_input=True)["file"]
    assert device_animation(f, True, [12], [True], 7, 1) == want
    stage = GIF.GifEncodeStage(17, 40, 1, DEV)
    assert stage.encode(bitmap_of(f, True), repeat=7, delay=12, needs_user_input=True)[0][0] == want


def test_the_same_frames_give_the_same_bytes_on_a_side_stream():
    frames = A.photo_frames(17, 40, 5, True, seed=11)
    delays, user = [1, 2, 3, 4, 5], [False] * 5
    want = device_animation(frames, True, delays, user, -1, 2)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = device_animation(frames, True, delays, user, -1, 2)
    side.synchronize()
    assert got == want == A.assemble(frames, True, delays, user, -1)[0]


# ---- jobs ------------------------------------------------------------------------------------------------------------------------------

def run(msg, inputs, outputs, animation=True, gif=True, expect=200):
    with Context() as c:
        assert c.set_gif_encoder(gif) is True and c.set_gif_animation(animation) is True
        for io_id, data in inputs.items():
            c.add_input_buffer(io_id, data)
        for io_id in outputs:
            c.add_output_buffer(io_id)
        status, r = c.send_json("v1/execute", msg)
        assert status == expect, (status, r)
        if expect != 200:
            return c.error_code(), r
        return {o: bytes(c.get_output_buffer(o)) for o in outputs}, r


def steps(*nodes):
    return {"framewise": {"steps": list(nodes)}}


DECODE = {"decode": {"io_id": 0}}
GIF_OUT = {"encode": {"io_id": 1, "preset": "gif"}}


def rgba_of_raw(raw):
    rows, w, h, alpha = unpack_raw_bgra(raw)
    return np.ascontiguousarray(rows[:, :4 * w].reshape(h, w, 4)[..., [2, 1, 0, 3]]), alpha


def frames_of(data):
    """every frame of a file as a viewer shows it: the oracle's screens, RGBA"""
    n = O.parse(data, 1 << 30)["frames_seen"]
    return [O.decode(data, k)[1][..., [2, 1, 0, 3]] for k in range(n)]


def test_rgb_animation_through_decode_and_encode():
    src = X.rgb_animation()
    outs, r = run(steps(DECODE, GIF_OUT), {0: src}, [1])
    got = frames_of(outs[1])
    assert len(got) == 3
    for k, colour in enumerate(X.RGB[:3]):
        assert (got[k] == np.array(colour + (255,), np.uint8)).all(), k
    _, durations, info, n = A.pillow_frames(outs[1])
    assert n == 3 and durations == [100, 100, 100] and info["loop"] == 0        # (no NETSCAPE2.0 block in the source: Infinite, as the one-frame path has it)
    entries = r["data"]["job_result"]["encodes"]
    assert len(entries) == 1 and (entries[0]["preferred_mime_type"], entries[0]["preferred_extension"], entries[0]["w"], entries[0]["h"]) == ("image/gif", "gif", 4, 4)
    assert len(r["data"]["job_result"]["decodes"]) == 1
    netscape = b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + (5).to_bytes(2, "little") + b"\x00"
    frames = [gif_gen.frame(np.full((4, 4), k, np.uint8), 4, 4, m=2, delay=10 + k) for k in range(3)]
    looped = gif_gen.gif(4, 4, frames, palette=np.array(X.RGB, np.uint8), extensions=netscape)
    outs, _ = run(steps(DECODE, GIF_OUT), {0: looped}, [1])
    _, durations, info, n = A.pillow_frames(outs[1])
    assert n == 3 and durations == [100, 110, 120] and info["loop"] == 5


def test_a_dispose_mixed_animation_keeps_every_screen():
    src = FILES["dispose_mixed"]
    outs, _ = run(steps(DECODE, GIF_OUT), {0: src}, [1])
    want, got = frames_of(src), frames_of(outs[1])
    assert len(got) == len(want) == 3
    for k in range(3):
        assert len(np.unique(want[k].reshape(-1, 4), axis=0)) <= 256
        assert np.array_equal(got[k], want[k]), k


def sixteen():
    pal = gif_gen.palette_of(64, 9)
    frames = [gif_gen.frame(gif_gen.noise(16, 16, 64, 30 + k), 16, 16, m=6, delay=2 + k) for k in range(3)]
    return gif_gen.gif(16, 16, frames, palette=pal)


RESAMPLE = {"resample_2d": {"w": 8, "h": 8}}


def test_resample_between_decode_and_encode_equals_the_emulations_assembly_and_survives_a_second_pass():
    src = sixteen()
    outs, _ = run(steps(DECODE, RESAMPLE, GIF_OUT), {0: src}, [1])
    taps = []
    for k in range(3):                                                          # the frames the coder saw: raw-tap jobs with select_frame = k
        tap, _ = run(steps({"decode": {"io_id": 0, "commands": [{"select_frame": k}]}}, RESAMPLE, GIF_OUT), {0: src}, [1], gif=False)
        rgba, alpha = rgba_of_raw(tap[1])
        assert alpha and rgba.shape == (8, 8, 4)
        taps.append(rgba)
    want, _ = A.assemble(taps, True, [2, 3, 4], [False] * 3, repeat=0)
    assert outs[1] == want
    again, _ = run(steps(DECODE, RESAMPLE, GIF_OUT), {0: outs[1]}, [1])        # the reference's #643
    P = O.parse(again[1], 1 << 30)
    assert P["frames_seen"] == 3 and [f["delay"] for f in P["frames"]] == [2, 3, 4]


def test_a_graph_with_a_gif_and_a_png_encoder():
    src = FILES["dispose_keep"]
    job = {"framewise": {"graph": {
        "nodes": {"0": DECODE, "1": GIF_OUT, "2": {"encode": {"io_id": 2, "preset": {"libpng": {}}}}},
        "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 0, "to": 2, "kind": "input"}]}}}
    outs, r = run(job, {0: src}, [1, 2])
    want = frames_of(src)
    got = frames_of(outs[1])
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want))
    png, _ = PO.decode(outs[2])
    assert np.array_equal(png[..., [2, 1, 0, 3]], want[0]), "every other encoder takes the first frame"
    kinds = {e["io_id"]: e["preferred_mime_type"] for e in r["data"]["job_result"]["encodes"]}
    assert kinds == {1: "image/gif", 2: "image/png"} and len(r["data"]["job_result"]["encodes"]) == 2


def test_every_other_job_is_what_it_is_with_the_switch_off():
    import io
    from PIL import Image
    src = FILES["dispose_previous"]
    jpeg = io.BytesIO()
    Image.fromarray(Q.photo_rgba(40, 30, seed=22)[..., :3].copy(), "RGB").save(jpeg, "JPEG", quality=85)
    one_frame = X.good_files()["transparent_index"][0]
    cases = {
        "select_frame": (steps({"decode": {"io_id": 0, "commands": [{"select_frame": 1}]}}, GIF_OUT), src),
        "one_frame_gif": (steps(DECODE, GIF_OUT), one_frame),
        "jpeg": (steps(DECODE, GIF_OUT), jpeg.getvalue()),
        "no_gif_encoder_downstream": (steps(DECODE, {"encode": {"io_id": 1, "preset": {"libpng": {}}}}), src),
    }
    for name, (job, data) in cases.items():
        on, r_on = run(job, {0: data}, [1])
        off, r_off = run(job, {0: data}, [1], animation=False)
        assert on[1] == off[1], name
        assert r_on["data"]["job_result"]["encodes"] == r_off["data"]["job_result"]["encodes"], name
    assert O.parse(run(cases["select_frame"][0], {0: src}, [1])[0][1], 1 << 30)["frames_seen"] == 1
    # told through v1/tell_decoder
    with Context() as c:
        assert c.set_gif_encoder(True) and c.set_gif_animation(True)
        c.add_input_buffer(0, src)
        c.add_output_buffer(1)
        assert c.send_json("v1/tell_decoder", {"io_id": 0, "command": {"select_frame": 2}})[0] == 200
        assert c.send_json("v1/execute", steps(DECODE, GIF_OUT))[0] == 200
        told = bytes(c.get_output_buffer(1))
    assert O.parse(told, 1 << 30)["frames_seen"] == 1 and np.array_equal(frames_of(told)[0], frames_of(src)[2])
    # animation on, GIF encoder off: the raw container of frame 0
    raw, _ = run(steps(DECODE, GIF_OUT), {0: src}, [1], gif=False)
    assert raw[1][:7] == b"IFBGRA1" and np.array_equal(rgba_of_raw(raw[1])[0], frames_of(src)[0])


def test_two_animated_decodes_of_3_and_2_frames_are_an_invalid_operation():
    two = gif_gen.gif(12, 9, [gif_gen.frame(gif_gen.noise(12, 9, 8, k), 12, 9, m=3) for k in range(2)], palette=gif_gen.palette_of(8, 3))
    job = {"framewise": {"graph": {
        "nodes": {"0": DECODE, "1": {"decode": {"io_id": 2}}, "2": {"copy_rect_to_canvas": {"from_x": 0, "from_y": 0, "w": 4, "h": 4, "x": 1, "y": 1}}, "3": GIF_OUT},
        "edges": [{"from": 0, "to": 2, "kind": "input"}, {"from": 1, "to": 2, "kind": "canvas"}, {"from": 2, "to": 3, "kind": "input"}]}}}
    code, r = run(job, {0: FILES["dispose_keep"], 2: two}, [1], expect=500)
    assert "InvalidOperation" in r["message"] and "read_frame was called without a frame available" in r["message"]
    three = FILES["dispose_background"]
    outs, _ = run(job, {0: FILES["dispose_keep"], 2: three}, [1])
    assert O.parse(outs[1], 1 << 30)["frames_seen"] == 3


def test_a_job_over_the_total_pixel_bound_is_refused():
    src = sixteen()                                                             # 3 x 256 pixels decoded, 3 x 64 collected
    job = steps(DECODE, RESAMPLE, GIF_OUT)
    for bound, ok in ((3 * 256 + 3 * 64, True), (3 * 256 + 3 * 64 - 1, False), (3 * 256 - 1, False)):
        job["security"] = {"max_total_file_pixels": bound}
        if ok:
            assert O.parse(run(job, {0: src}, [1])[0][1], 1 << 30)["frames_seen"] == 3
        else:
            code, r = run(job, {0: src}, [1], expect=400)
            assert code == 2 and "SizeLimitExceeded" in r["message"] and "max_total_file_pixels" in r["message"]
    job["security"] = {"max_total_file_pixels": 1}                                # the rule is the animation path's alone
    assert run(job, {0: src}, [1], animation=False)[0][1][:6] == b"GIF89a"


def polls_to_finish(job, src):
    """the job with a cancellation at its n-th poll for n = 0, 1, ..: cancelled every time (OperationCancelled, nothing else)
    until n exceeds the polls the job has; -> that n"""
    for n in range(400):
        with Context() as c:
            assert c.set_gif_encoder(True) and c.set_gif_animation(True)
            c.add_input_buffer(0, src)
            c.add_output_buffer(1)
            c.L.ifhip_shim_request_cancellation_after_n_polls(c.p, n)
            status, r = c.send_json("v1/execute", job)
            left = c.L.ifhip_shim_cancellation_polls_remaining(c.p)
            if left > 0:
                assert status == 200 and not c.has_error()
                assert O.parse(bytes(c.get_output_buffer(1)), 1 << 30)["frames_seen"] >= 1
                return n
            if not (left == 0 and status == 200):
                assert left < 0 and status == 499 and c.error_code() == 21, (n, left, status, r)
    raise AssertionError("the job never finished")


def test_cancellation_is_polled_in_every_frame_and_between_frames():
    src = X.rgb_animation()
    one = polls_to_finish(steps({"decode": {"io_id": 0, "commands": [{"select_frame": 0}]}}, GIF_OUT), src)
    three = polls_to_finish(steps(DECODE, GIF_OUT), src)
    assert three >= one + 2 * 3, (one, three)                                   # per further frame: the frame's own poll and one per node at the least
