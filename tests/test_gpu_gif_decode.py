"""The device GIF decoder on an MI355X (csrc/gif_read.cpp + csrc/gif_decode.hip through imageflow_amd.codecs.gif_decoder and
the shim's `decode`): the files of tests/gif_fixtures.py -- every minimum code size, every code width, clears wherever the wave
step, the first chunk and a tail chunk end, deferred clears with long tails, KwKwK chains, interlaced heights, every palette
and compositing rule, three-frame animations with each disposal method -- decode byte for byte to the oracle's screen
(tests/gif_oracle.py, pinned to Pillow), which is also what the CPU emulation of the same core header gives
(tests/test_gif_decode_core.py); the frame's padding, pre-filled with 0xA5, comes back untouched, and every damaged file gets
its status word and leaves its frame and its neighbours alone.  There is no tolerance anywhere."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import gif_decoder as D  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap, get_stride  # noqa: E402
from tests import gif_fixtures as X  # noqa: E402
from tests import gif_oracle as O  # noqa: E402
from tests import png_decode_oracle as PO  # noqa: E402
from tests import util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOOD = sorted(X.good_files())
BAD = sorted(X.damaged_files())
# one batch per group: the test's name says what the group is there for
GROUPS = {
    "minimum_code_sizes_1_to_8": [n for n in GOOD if n[0] == "m" and n[1].isdigit()],
    "width_boundaries_and_full_tables": [n for n in GOOD if n.startswith(("widths_", "clear_early", "two_clears", "deferred_", "flat_", "mixed_"))],
    "clear_or_end_at_the_step_and_chunk_boundaries": [n for n in GOOD if n.startswith(("clear_at_", "end_at_"))],
    "stream_ends": [n for n in GOOD if n.startswith(("no_leading", "no_end", "bytes_after", "more_indices", "small_sub", "no_trailer", "gif87a"))],
    "frame_sizes_and_interlace": [n for n in GOOD if n.startswith(("size_", "interlaced_"))],
    "palettes": [n for n in GOOD if n.startswith(("local_", "no_global", "index_beyond", "transparent_", "background_"))],
    "compositing": [n for n in GOOD if n.startswith(("frame_", "zero_size", "dispose_", "rgb_animation"))],
}


def test_every_good_file_is_in_a_group():
    assert sorted(n for g in GROUPS.values() for n in g) == GOOD


def frames_for(files, extra_stride):
    """frames pre-filled with 0xA5 at the default stride plus `extra_stride` bytes (None where the file has no canvas)"""
    out = []
    for data in files:
        try:
            info = D.gif_info(data)
        except Exception:
            out.append(None)
            continue
        if not info["width"] or not info["height"]:
            out.append(None)
            continue
        stride = get_stride(info["width"]) + extra_stride
        out.append(Bitmap(torch.full((1, info["height"] * stride), 0xA5, dtype=torch.uint8, device=DEV), info["width"], info["height"], stride, alpha_meaningful=True))
    return out


def decode_and_check(names, extra_stride=0):
    """one batch: names of good files and of damaged ones; good frames against the oracle, padding untouched"""
    entries = [X.good_files()[n] if n in X.good_files() else X.damaged_files()[n] for n in names]
    files, targets = [e[0] for e in entries], [e[1] for e in entries]
    frames, status = D.decode_gif_batch(files, targets, DEV, frames=frames_for(files, extra_stride))
    torch.cuda.synchronize()
    for i, n in enumerate(names):
        if n in X.good_files():
            want = X.expected(n)
            assert status[i] == 0, (n, status[i])
            got, w = frames[i].to_numpy()[0], frames[i].w
            assert got.shape[0] == want.shape[0] and w == want.shape[1]
            assert np.array_equal(got[:, :4 * w].reshape(want.shape), want), n
            assert (got[:, 4 * w:] == 0xA5).all(), ("padding", n)
        else:
            assert status[i] == entries[i][2], (n, status[i], entries[i][2])
            if frames[i] is not None:
                assert (frames[i].to_numpy()[0] == 0xA5).all(), ("a damaged file's frame must stay untouched", n)
    return status


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_good_files(group):
    decode_and_check(GROUPS[group])


def test_a_file_alone_and_select_frame_beyond_the_file():
    decode_and_check(["deferred_m8_long_tail"])
    decode_and_check(["size_1x1"])
    assert decode_and_check(["rgb_animation_frame3"]) == [O.NO_SUCH_FRAME]
    bgra = D.decode_gif(X.good_files()["rgb_animation_frame1"][0], 1, DEV).to_numpy()[0]
    assert (bgra[:, :16].reshape(4, 4, 4) == (0, 255, 0, 255)).all()            # the green frame


@pytest.mark.parametrize("extra_stride", [0, 52])
def test_one_batch_of_good_files_of_mixed_sizes_with_every_damaged_file_between_them(extra_stride):
    good = [n for n in GOOD if not n.startswith(("end_at_", "interlaced_h", "dispose_"))] + ["interlaced_h37", "dispose_mixed_frame2", "end_at_64"]
    batch = []
    for k, name in enumerate(BAD):
        batch += [good[(5 * k) % len(good)], name]
    batch += good
    no_canvas = b"GIF89a" + bytes(32)
    files_extra = [no_canvas, b"not a gif at all"]
    entries = [X.good_files()[n] if n in X.good_files() else X.damaged_files()[n] for n in batch]
    files, targets = [e[0] for e in entries] + files_extra, [e[1] for e in entries] + [0, 0]
    frames, status = D.decode_gif_batch(files, targets, DEV, frames=frames_for(files, extra_stride))
    torch.cuda.synchronize()
    assert status[-2:] == [O.CONTAINER, O.CONTAINER]
    for i, n in enumerate(batch):
        if n in X.good_files():
            want, w = X.expected(n), frames[i].w
            got = frames[i].to_numpy()[0]
            assert status[i] == 0 and np.array_equal(got[:, :4 * w].reshape(want.shape), want), n
            assert (got[:, 4 * w:] == 0xA5).all(), ("padding", n)
        else:
            assert status[i] == entries[i][2], n
            assert (frames[i].to_numpy()[0] == 0xA5).all(), ("a damaged file's frame must stay untouched", n)


def test_host_drop_in_equals_the_batch_form_and_keeps_the_padding():
    for name in ("widths_m8_clear_at_full", "dispose_previous_frame2", "interlaced_h9", "size_1x37"):
        data, target = X.good_files()[name]
        want = X.expected(name)
        h, w = want.shape[:2]
        stride = 4 * w + 20
        out = np.full((h, stride), 0x5A, np.uint8)
        D.decode_gif_host(data, target, stride, out)
        assert np.array_equal(out[:, :4 * w].reshape(want.shape), want) and (out[:, 4 * w:] == 0x5A).all(), name
    for name, text in (("too_little_cut", "GIF decoding error"), ("bad_code_beyond_the_table", "GIF decoding error"), ("no_such_frame", "frame=2 requested but GIF only has 2 frames")):
        data, target, _ = X.damaged_files()[name]
        out = np.full((47, 4 * 61), 0x5A, np.uint8)
        with pytest.raises(Exception) as e:
            D.decode_gif_host(data, target, None, out)
        assert text in str(e.value) and (out == 0x5A).all()


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


RAW = {"encode": {"io_id": 9, "preset": "gif"}}                      # (the raw BGRA container)
LIBPNG = {"encode": {"io_id": 9, "preset": {"libpng": {}}}}


def test_decode_gif_then_encode_libpng_reproduces_the_oracles_pixels():
    for name in ("widths_m2_clear_at_full", "transparent_index", "interlaced_h37", "no_global_palette"):
        want = X.expected(name)
        outs, r = run_job({0: X.good_files()[name][0]}, [{"decode": {"io_id": 0}}, LIBPNG])
        got, info = PO.decode(outs[0])
        assert info["color_type"] == 6 and np.array_equal(got, want), name       # bgra_32 with meaningful alpha: RGBA
        dec = r["data"]["job_result"]["decodes"][0]
        assert (dec["preferred_mime_type"], dec["preferred_extension"], dec["w"], dec["h"]) == ("image/gif", "gif", want.shape[1], want.shape[0])


def test_select_frame_composes_up_to_the_frame_and_refuses_one_beyond_the_file():
    data = X.good_files()["rgb_animation_frame0"][0]                         # 4 x 4: red, green, blue
    colours = [(0, 0, 255, 255), (0, 255, 0, 255), (255, 0, 0, 255)]            # BGRA
    for n in range(3):
        for steps, tell in (([{"decode": {"io_id": 0, "commands": [{"select_frame": n}]}}, LIBPNG], None), ([{"decode": {"io_id": 0}}, LIBPNG], [(0, {"select_frame": n})])):
            got, _ = PO.decode(run_job({0: data}, steps, tell=tell)[0][0])
            assert (got == colours[n]).all(), n
    assert (PO.decode(run_job({0: data}, [{"decode": {"io_id": 0}}, LIBPNG])[0][0])[0] == colours[0]).all()      # without the command: frame 0
    code, r = run_job({0: data}, [{"decode": {"io_id": 0, "commands": [{"select_frame": 3}]}}, LIBPNG], expect=400)
    assert code == 2 and "InvalidArgument" in r["message"] and "frame=3 requested but GIF only has 3 frames" in r["message"]
    for kind in ("keep", "background", "previous", "mixed"):
        for n in range(3):
            name = "dispose_%s_frame%d" % (kind, n)
            got, _ = PO.decode(run_job({0: X.good_files()[name][0]}, [{"decode": {"io_id": 0, "commands": [{"select_frame": n}]}}, LIBPNG])[0][0])
            assert np.array_equal(got, X.expected(name)), name
    png = PO.write_png(np.zeros((5, 7, 3), np.uint32), 2, 8)                   # the other decoders ignore the command
    steps = [{"decode": {"io_id": 0}}, RAW]
    assert run_job({0: png}, steps, tell=[(0, {"select_frame": 4})])[0][0] == run_job({0: png}, steps)[0][0]


def test_a_gif_logo_watermarks_like_the_same_logo_in_the_raw_container():
    back = U.random_frames(1, 320, 200, seed0=51, alpha=False)[0]
    logo = X.expected("transparent_index")
    h, w = logo.shape[:2]
    rows = np.zeros((h, U.stride_for(w)), np.uint8)
    rows[:, :4 * w] = logo.reshape(h, 4 * w)
    steps = [{"decode": {"io_id": 0}}, {"watermark": {"io_id": 1, "opacity": 0.7, "gravity": {"percentage": {"x": 100, "y": 100}}}}, RAW]
    base = {0: pack_raw_bgra(back, 320, 200, alpha_meaningful=False)}
    a, _ = run_job({**base, 1: X.good_files()["transparent_index"][0]}, steps)
    b, _ = run_job({**base, 1: pack_raw_bgra(rows, w, h, alpha_meaningful=True)}, steps)
    assert a[0] == b[0]
    assert a[0] != run_job(base, [steps[0], steps[2]])[0][0]


def test_a_command_string_job_with_a_gif_source():
    data = X.good_files()["widths_m8_clear_at_full"][0]                      # 200 x 150
    outs, r = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=100", "decode": 0, "encode": 9}}])
    rows, w, h, alpha = unpack_raw_bgra(outs[0])
    assert (w, h) == (100, 75) and rows[:, :400].std() > 1
    code, r = run_job({0: data}, [{"command_string": {"kind": "ir4", "value": "width=100&frame=1", "decode": 0, "encode": 9}}], expect=400)
    assert "frame" in r["message"]                                             # the querystring key stays refused


def test_limits_are_enforced_from_the_header_and_damage_is_image_malformed():
    huge = b"GIF89a" + (60000).to_bytes(2, "little") * 2 + b"\x00\x00\x00"   # the header alone: no frame behind it
    code, r = run_job({0: huge}, [{"decode": {"io_id": 0}}, RAW], expect=400)
    assert code == 2 and "max_decode_size" in r["message"]
    data = X.good_files()["widths_m8_clear_at_full"][0]
    for key in ("max_decode_size", "max_frame_size"):
        code, r = run_job({0: data}, [{"decode": {"io_id": 0}}, RAW], expect=400, security={key: {"w": 100, "h": 100, "megapixels": 1}})
        assert code == 2 and key in r["message"]
    for name in ("too_little_cut", "bad_code_in_a_later_segment", "no_palette_at_all", "min_code_size_9", "unknown_block"):
        code, r = run_job({0: X.damaged_files()[name][0]}, [{"decode": {"io_id": 0}}, RAW], expect=400)
        assert code == 4 and "GIF decoding error" in r["message"], name
    assert "_some_ palette" in run_job({0: X.damaged_files()["no_palette_at_all"][0]}, [{"decode": {"io_id": 0}}, RAW], expect=400)[1]["message"]
    code, r = run_job({0: b"GIF89a" + bytes(40)}, [{"decode": {"io_id": 0}}, RAW], expect=400)
    assert code == 5
