"""Animated GIFs without a device: the host walk to a file's end (ifhip_gif_frame_count) against the oracle's; every composed
screen of a file in one replay (csrc/gif_decode_core.hpp on the CPU) against the oracle's compose for every frame; the
animation file -- assembled in plain Python from the one-frame coder's per-frame results, and laid out over the file's dwords
by csrc/gif_encode_core.hpp chunk by chunk -- read back by the oracle and by Pillow; the new C entries' argument checks; the
declarations; and the static guard on the new kernels.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd import _native  # noqa: E402
from imageflow_amd import build as B  # noqa: E402
from imageflow_amd.abi import Context  # noqa: E402
from imageflow_amd.codecs import gif_decoder as D  # noqa: E402
from imageflow_amd.codecs import gif_encoder as E  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from tests import gif_animation_emu as A  # noqa: E402
from tests import gif_encode_emu as G  # noqa: E402
from tests import gif_fixtures as X  # noqa: E402
from tests import gif_gen  # noqa: E402
from tests import gif_oracle as O  # noqa: E402
from tests.test_kernel_resources import _int, resource_usage  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = int(ErrorKind.InvalidArgument)
NO_DEVICE = (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
DISPOSE = {"keep": (O.KEEP, O.KEEP, O.KEEP), "background": (O.BACKGROUND, O.BACKGROUND, O.KEEP), "previous": (O.KEEP, O.PREVIOUS, O.PREVIOUS),
           "mixed": (O.PREVIOUS, O.BACKGROUND, O.ANY)}


def animations():
    out = {"dispose_" + name: X.animation(d) for name, d in DISPOSE.items()}
    out["dispose_background_off_the_canvas"] = X.animation((O.KEEP, O.BACKGROUND, O.KEEP), offscreen=True)
    out["dispose_previous_off_the_canvas"] = X.animation((O.KEEP, O.PREVIOUS, O.KEEP), offscreen=True)
    out["rgb_animation"] = X.rgb_animation()
    out["zero_size_frame_then_one"] = X.good_files()["zero_size_frame_then_one"][0]
    return out


def seventy_frames():
    """37 x 23, 70 frames: small frames at moving places, every disposal method, transparent entries"""
    pal = gif_gen.palette_of(16, 5)
    frames = [gif_gen.frame(gif_gen.noise(37, 23, 16, 1), 37, 23, m=4, delay=3)]
    for k in range(1, 70):
        w, h = 5 + k % 9, 3 + k % 7
        frames.append(gif_gen.frame(gif_gen.noise(w, h, 16, 100 + k), w, h, left=(3 * k) % 33, top=(5 * k) % 21, m=4, dispose=k % 4, transparent=k % 16 if k % 3 else None,
                                    delay=k))
    return gif_gen.gif(37, 23, frames, palette=pal, bg=3)


# ---- declarations and the switch ------------------------------------------------------------------------------------------------------

def test_headers_declare_and_the_library_exports_the_new_entries():
    header = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    subset = open(os.path.join(ROOT, "include", "imageflow_abi_subset.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop.rs")).read()
    L = _native.lib()
    for name in ("ifhip_gif_frame_count", "ifhip_gif_decode_frames_device", "ifhip_gif_enc_stage_max_animation_bytes", "ifhip_gif_encode_animation_device"):
        assert re.search(r"IFHIP_API [^;]*\b%s\(" % name, header), name
        assert re.search(r"\bfn %s\(" % name, bindings), name
        assert getattr(L, name) is not None
    assert re.search(r"IMAGEFLOW_SHIM_API bool ifhip_shim_context_set_gif_animation\(", subset)
    assert "Not built: multi-frame output" not in header
    with Context() as c:
        assert c.set_gif_animation(True) is True and c.set_gif_animation(False) is True


# ---- ifhip_gif_frame_count -----------------------------------------------------------------------------------------------------------

def walk(data):
    """(return code, frames) of the library's host walk, with delays and flags where it succeeds"""
    L = D._bind()
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    n = C.c_uint32(77)
    rc = L.ifhip_gif_frame_count(buf.ctypes.data, len(data), C.byref(n), None, None, 0)
    return rc, n.value


def test_frame_count_equals_the_oracles_walk():
    files = dict(animations())
    files["seventy"] = seventy_frames()
    files["no_trailer"] = X.good_files()["no_trailer"][0]
    files["no_trailer_3"] = X.rgb_animation()[:-1]
    for name, data in files.items():
        P = O.parse(data, 1 << 30)
        assert P["status"] == O.NO_SUCH_FRAME, name                                       # the oracle's word for "the walk reached the end"
        n, delays, flags = D.gif_frame_count(data)
        assert n == P["frames_seen"] == len(P["frames"]), name
        assert delays == [f["delay"] for f in P["frames"]] and flags == [f["user_input"] for f in P["frames"]], name
    assert D.gif_frame_count(files["rgb_animation"]) == (3, [10, 10, 10], [False] * 3)
    assert D.gif_frame_count(files["seventy"])[1][:4] == [3, 1, 2, 3]
    # a short capacity fills what it holds
    L = D._bind()
    buf = np.frombuffer(files["seventy"], np.uint8)
    n, d, f = C.c_uint32(0), (C.c_uint32 * 4)(9, 9, 9, 9), (C.c_uint32 * 4)(9, 9, 9, 9)
    assert L.ifhip_gif_frame_count(buf.ctypes.data, buf.size, C.byref(n), d, f, 3) == 0 and n.value == 70 and list(d) == [3, 1, 2, 9] and list(f) == [0, 0, 0, 9]
    assert L.ifhip_gif_frame_count(None, 0, C.byref(n), None, None, 0) == INVALID and L.ifhip_gif_frame_count(buf.ctypes.data, buf.size, None, None, None, 0) == INVALID


def test_frame_count_on_the_damaged_files():
    for name, (data, _, status) in X.damaged_files().items():
        P = O.parse(data, 1 << 30)
        rc, n = walk(data)
        assert n == P["frames_seen"], name
        if P["status"] == O.NO_SUCH_FRAME:                       # the host walk sees nothing wrong (the damage is inside a frame's LZW data)
            assert rc == 0, name
        else:
            assert rc == INVALID and b"ImageMalformed" in _native.lib().ifhip_last_error_message(), name
    assert walk(b"GIF89a")[0] == INVALID


# ---- compose-all on the CPU ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(animations()) + ["seventy"])
def test_emulated_compose_all_gives_the_oracles_screen_for_every_frame(name):
    data = seventy_frames() if name == "seventy" else animations()[name]
    P = O.parse(data, 1 << 30)
    st, screens, _ = A.decode_frames(data)
    assert st == 0 and len(screens) == P["frames_seen"]
    for k in range(len(screens)):
        assert np.array_equal(screens[k], O.compose(P, k)), (name, k)


def test_emulated_compose_all_keeps_padding_and_writes_nothing_for_a_damaged_file():
    data = animations()["dispose_mixed"]
    st, screens, block = A.decode_frames(data, stride=4 * 12 + 8, pad_rows=1, fill=0x5A)
    assert st == 0 and np.array_equal(screens, A.decode_frames(data)[1])
    rows = block.reshape(3, 10, 4 * 12 + 8)
    assert (rows[:, :9, 4 * 12:] == 0x5A).all() and (rows[:, 9] == 0x5A).all()
    bad, _, status = X.damaged_files()["second_frame_damaged"]
    assert A.decode_frames(bad)[0] == status


# ---- the coder's file ------------------------------------------------------------------------------------------------------------------

def check_reads_back(data, per_frame, alpha, delays, repeat):
    """the oracle (the reference's Screen::blit) and Pillow read every frame back as the pixels the coder chose"""
    want = [G.decoded(q) for q in per_frame]
    n = len(want)
    P = O.parse(data, 1 << 30)
    assert P["frames_seen"] == n and [f["delay"] for f in P["frames"]] == list(delays)
    for k in range(n):
        st, screen, _ = O.decode(data, k)
        assert st == O.OK and np.array_equal(screen[..., [2, 1, 0, 3]], want[k]), k
    frames, durations, info, n_frames = A.pillow_frames(data)
    assert n_frames == n and durations == [10 * d for d in delays]
    assert info.get("loop") == (repeat if repeat >= 0 else None)
    for k in range(n):
        assert np.array_equal(frames[k][..., 3], want[k][..., 3]), "alpha mask of frame %d" % k
        seen = want[k][..., 3] == 255
        assert np.array_equal(frames[k][seen], want[k][seen]), "visible colours of frame %d" % k


@pytest.mark.parametrize("alpha", [True, False])
def test_the_assembled_file_reads_back_frame_by_frame(alpha):
    frames = A.photo_frames(17, 40, 3, alpha, seed=3)
    delays, user = [4, 0, 250], [False, True, False]
    data, per_frame = A.assemble(frames, alpha, delays, user, repeat=2)
    check_reads_back(data, per_frame, alpha, delays, 2)
    assert all(q["n_trans"] == (1 if alpha else 0) for q in per_frame)
    gce = [m.start() for m in re.finditer(re.escape(b"\x21\xF9\x04"), data)][:1]
    assert data[gce[0] + 3] >> 2 == (2 if alpha else 1)
    # the layout over the file's dwords gives the same bytes, whatever the chunk
    for chunk in (1, 2, 3):
        assert A.layout(frames, alpha, delays, user, repeat=2, chunk=chunk, per_frame=per_frame) == (data, 0), chunk
    again, _ = A.assemble(frames, alpha, delays, user, repeat=-1, per_frame=per_frame)
    assert A.layout(frames, alpha, delays, user, repeat=-1, chunk=2, per_frame=per_frame) == (again, 0)
    check_reads_back(again, per_frame, alpha, delays, -1)


def test_with_keep_a_transparent_pixel_would_show_the_frame_before():
    """the ground of the disposal rule: the same bodies with the reference's Keep do NOT read back"""
    frames = A.photo_frames(17, 40, 3, True, seed=3)
    data, per_frame = A.assemble(frames, True, [1, 1, 1], [False] * 3)
    keep = bytearray(data)
    for m in re.finditer(re.escape(b"\x21\xF9\x04\x09"), data):
        keep[m.start() + 3] = 1 << 2 | 1
    st, screen, _ = O.decode(bytes(keep), 1)
    assert st == O.OK and not np.array_equal(screen[..., [2, 1, 0, 3]], G.decoded(per_frame[1]))


def test_the_one_frame_animation_is_the_one_frame_file():
    for alpha in (True, False):
        f = A.photo_frames(17, 40, 1, alpha, seed=9)
        for repeat in (-1, 0, 7):
            want = G.encode(f[0], alpha=alpha, repeat=repeat, delay=12, user_input=True)["file"]
            assert A.assemble(f, alpha, [12], [True], repeat)[0] == want
            assert A.layout(f, alpha, [12], [True], repeat) == (want, 0)


def test_bodies_at_every_byte_of_a_dword_and_chunks_of_every_size():
    frames = A.residue_frames()
    delays, user = list(range(len(frames))), [k % 2 == 1 for k in range(len(frames))]
    data, per_frame = A.assemble(frames, False, delays, user, repeat=0)
    assert {n % 4 for n in A.body_lengths(per_frame)} == {0, 1, 2, 3}
    starts = np.cumsum([A.SCREEN + A.NETSCAPE] + A.body_lengths(per_frame))
    assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}, "a body starts at every byte of a dword"
    for chunk in range(1, len(frames) + 1):
        assert A.layout(frames, False, delays, user, repeat=0, chunk=chunk, per_frame=per_frame) == (data, 0), chunk
    check_reads_back(data, per_frame, False, delays, 0)
    # a capacity one byte short: no file
    assert A.layout(frames, False, delays, user, repeat=0, chunk=2, cap=len(data), per_frame=per_frame) == (data, 0)
    assert A.layout(frames, False, delays, user, repeat=0, chunk=2, cap=len(data) - 1, per_frame=per_frame) == (None, A.FILE_OVERFLOW)
    assert len(data) <= A.max_animation_bytes(9, 7, len(frames))


# ---- argument checks come before the device check --------------------------------------------------------------------------------------

def test_argument_checks_of_the_new_entries_come_before_the_device_check():
    """The device pointers are made up: every call below fails its checks or, on a machine without a GPU, reaches the device
    check.  Where a GPU is present the calls that would pass their checks are not made."""
    gpu = torch.cuda.is_available()
    L, LE = D._bind(), E._bind()
    data = X.rgb_animation()                                                 # 4 x 4, 3 frames
    buf = np.frombuffer(data, np.uint8)
    n = C.c_uint32(5)
    SCREENS, STATUS = 0x7F0000000000, 0x7F0000200000

    def frames(screens=SCREENS, pitch=64, stride=16, max_frames=3, status=STATUS, out=n, src=buf.ctypes.data):
        return L.ifhip_gif_decode_frames_device(src, buf.size, screens, pitch, stride, max_frames, status, C.byref(out) if out is not None else None, None)
    assert frames(src=None) == INVALID and frames(out=None) == INVALID and frames(screens=None) == INVALID and frames(status=None) == INVALID
    assert frames(stride=12) == INVALID and frames(stride=18) == INVALID and frames(pitch=60) == INVALID and frames(screens=SCREENS + 2) == INVALID
    assert frames(max_frames=2) == INVALID and b"3 frames" in L.ifhip_last_error_message()
    assert frames(max_frames=0) == INVALID and n.value == 0
    bad = np.frombuffer(X.damaged_files()["unknown_block"][0], np.uint8)
    assert L.ifhip_gif_decode_frames_device(bad.ctypes.data, bad.size, SCREENS, 61 * 47 * 4, 61 * 4, 9, STATUS, C.byref(n), None) == INVALID
    assert b"ImageMalformed" in L.ifhip_last_error_message()
    if not gpu:
        assert frames() in NO_DEVICE

    stage = C.c_void_p()
    assert LE.ifhip_gif_enc_stage_create(C.byref(stage), 17, 40, 2) == 0
    size = C.c_size_t(1)
    assert LE.ifhip_gif_enc_stage_max_animation_bytes(stage, 5, C.byref(size)) == 0
    assert size.value == 13 + 19 + 5 * LE.ifhip_gif_enc_stage_max_file_bytes(stage) + 1 == A.max_animation_bytes(17, 40, 5)
    assert LE.ifhip_gif_enc_stage_max_animation_bytes(stage, 0, C.byref(size)) == INVALID and size.value == 0
    assert LE.ifhip_gif_enc_stage_max_animation_bytes(None, 5, C.byref(size)) == INVALID
    assert LE.ifhip_gif_enc_stage_max_animation_bytes(stage, 5, None) == INVALID
    assert LE.ifhip_gif_enc_stage_max_animation_bytes(stage, 4000000, C.byref(size)) == INVALID and size.value == 0     # 2^32 bytes or more
    IMAGES, FILE, LENGTH = 0x7F0000000000, 0x7F0000400000, 0x7F0000600000
    delays, user = (C.c_uint32 * 3)(1, 2, 3), (C.c_uint8 * 3)(0, 1, 0)

    def encode(stage=stage, images=IMAGES, image_bytes=40 * 68, stride=68, n_frames=3, repeat=0, d=delays, u=user, file=FILE, capacity=1 << 20, length=LENGTH):
        return LE.ifhip_gif_encode_animation_device(stage, images, image_bytes, stride, 1, n_frames, repeat, d, u, file, capacity, length, None, None)
    assert encode(stage=None) == INVALID and encode(images=None) == INVALID and encode(file=None) == INVALID and encode(length=None) == INVALID
    assert encode(d=None) == INVALID and encode(u=None) == INVALID
    assert encode(n_frames=0) == INVALID
    assert encode(capacity=32) == INVALID and b"capacity" in LE.ifhip_last_error_message()
    assert encode(stride=64) == INVALID and encode(stride=70) == INVALID and encode(image_bytes=39 * 68) == INVALID
    assert encode(file=FILE + 1) == INVALID and encode(repeat=-2) == INVALID and encode(repeat=65536) == INVALID
    assert encode(d=(C.c_uint32 * 3)(1, 65536, 3)) == INVALID
    if not gpu:
        assert encode() in NO_DEVICE
    LE.ifhip_gif_enc_stage_destroy(stage)


# ---- the static guard --------------------------------------------------------------------------------------------------------------------

def test_the_new_kernels_use_no_scratch_and_hold_the_lds_of_the_design_table():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.17" in design
    rows = dict(resource_usage(os.path.join(B.CSRC, "gif_decode.hip")))
    rows.update(resource_usage(os.path.join(B.CSRC, "gif_encode.hip")))
    want_lds = {"gif_compose_all_kernel": 0, "gif_anim_offsets_kernel": 4 * 256 // 64, "gif_anim_layout_kernel": 0}
    for name, lds in want_lds.items():
        r = rows[name]
        assert _int(r, "ScratchSize [bytes/lane]") == 0, (name, r)
        assert _int(r, "VGPRs") <= 128, (name, r)
        assert _int(r, "LDS Size [bytes/block]") == lds, (name, r)
        m = re.search(r"\| `%s` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|" % name, design)      # lanes, VGPRs, LDS bytes, scratch
        assert m, name
        assert int(m.group(1)) == 256 and int(m.group(3)) == lds and int(m.group(4)) == 0, (name, m.groups(), r)
    # the replay the two compose kernels share costs the one-frame kernel no scratch either
    assert _int(rows["gif_compose_kernel"], "ScratchSize [bytes/lane]") == 0
