"""The colour link kernels on an MI355X (csrc/color_link.hip through imageflow_amd.codecs.color_profile) against their CPU emulation
(tests/color_link_emulate.cpp: the same arithmetic header on the same links), byte for byte: odd widths, padding and a base that
is not 16-byte aligned, a batch, every order of the three remainders and their ties, the top cell and byte 0, the grey table on
the B byte alone, one profile per element type, and the batch call's stream order at its first use (which uploads the link) and
at a later one.  And without a device: the argument checks, which come before the device is touched."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.codecs import color_profile as CP  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import color_link_emulation as L  # noqa: E402
from tests import color_link_profiles as W  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0xA5
INVALID = int(ErrorKind.InvalidArgument)


def profiles():
    """name -> (icc, frame_is_gray): one profile per element type, and a grey one"""
    if not hasattr(profiles, "made"):
        profiles.made = {"mft1": (W.mft_profile(1, wide=False, grid=9).icc, False), "mft2": (W.mft_profile(6, grid=9, in_entries=4096, out_entries=2, version=4).icc, False),
                         "mAB": (W.mab_profile(17, pcs=b"Lab ", grid=(17, 9, 9), a_curves="para").icc, False),
                         "gray": (W.gray_profile(W.GRAY_TRCS["dotgain"]), True)}
    return profiles.made


def links(name):
    """-> (the native link, the emulation's link of the same profile)"""
    if not hasattr(links, "made"):
        links.made = {}
    if name not in links.made:
        icc, gray = profiles()[name]
        status, emulated, why = L.link_from_icc(icc, gray)
        assert status == L.PLANNED, why
        links.made[name] = (CP.link_from_icc(icc, gray), emulated)
    return links.made[name]


def on_device(host, w, h, stride, image_bytes, n, name, offset=0):
    """`host`: uint8 [offset + n * image_bytes + slack]; the frames start at `offset`.  -> the whole buffer after the device call"""
    data = torch.from_numpy(host.copy()).to(DEV)
    frames = data[offset:offset + n * image_bytes].view(n, image_bytes)
    CP.link_to_srgb(Bitmap(frames, w, h, stride), links(name)[0])
    torch.cuda.synchronize()
    return data.cpu().numpy()


def emulated(host, w, h, stride, image_bytes, n, name, offset=0):
    want = host.copy()
    for i in range(n):
        at = offset + i * image_bytes
        valid = (h - 1) * stride + 4 * w
        rows = np.zeros(h * stride, np.uint8)
        rows[:valid] = host[at:at + valid]
        want[at:at + valid] = L.transform(rows.reshape(h, stride), w, links(name)[1]).ravel()[:valid]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mft1", "mft2", "mAB", "gray"])
def test_an_odd_frame_with_padding_off_the_16_byte_grid(name):
    """47 x 9 at a stride of 47 * 4 + 12, the base one pixel into the allocation; guard bytes around the frame and the padding keep
    their values"""
    w, h = 47, 9
    stride = 4 * w + 12
    valid = (h - 1) * stride + 4 * w
    host = np.full(4 + valid + 64, SENTINEL, np.uint8)
    rng = np.random.default_rng(7)
    rows = np.full((h, stride), SENTINEL, np.uint8)
    rows[:, :4 * w] = rng.integers(0, 256, (h, 4 * w), dtype=np.uint8)
    host[4:4 + valid] = rows.ravel()[:valid]
    image_bytes = (valid + 3) // 4 * 4
    got, want = on_device(host, w, h, stride, image_bytes, 1, name, offset=4), emulated(host, w, h, stride, image_bytes, 1, name, offset=4)
    assert np.array_equal(got, want)
    assert (got[:4] == SENTINEL).all() and (got[4 + valid:] == SENTINEL).all()
    body = got[4:4 + valid]
    for y in range(h - 1):
        assert (body[y * stride + 4 * w:(y + 1) * stride] == SENTINEL).all()
    assert not np.array_equal(got, host)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mft2", "gray"])
def test_a_batch_of_two_frames(name):
    n, w, h = 2, 48, 32
    stride = 4 * w
    rng = np.random.default_rng(11)
    host = rng.integers(0, 256, n * h * stride, dtype=np.uint8)
    got, want = on_device(host, w, h, stride, h * stride, n, name), emulated(host, w, h, stride, h * stride, n, name)
    assert np.array_equal(got, want) and not np.array_equal(got[:h * stride], got[h * stride:])
    assert np.array_equal(got[3::4], host[3::4])                                   # the fourth byte as it was


def remainder_pixels():
    """R, G, B bytes whose remainders in a cell of the 33-grid take all six orders, the ties rx = ry, ry = rz, rx = rz and all
    equal, byte 255 on each axis (the top cell: a wrong index reads node 33), byte 0, and the 86^3 grid of the matrix tests"""
    a, b, c = 1, 3, 6                                                               # three bytes of one cell with rising remainders
    pts = [(x, y, z) for x in (a, b, c) for y in (a, b, c) for z in (a, b, c)]      # every order and every tie inside the cell at 0
    pts += [(x + 64, y + 128, z + 200) for x, y, z in pts]
    top = (0, 3, 128, 254, 255)
    pts += [(x, y, z) for x in top for y in top for z in top]
    axis = np.arange(0, 256, 3)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([np.array(pts), grid]).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mft1", "mft2", "mAB"])
def test_every_tetrahedron_the_top_cell_and_the_colour_grid(name):
    rgb = remainder_pixels()
    pos = rgb.astype(np.int64) * 257 * 32
    rest = (pos + (pos + 0x7FFF) // 0xFFFF) & 0xFFFF
    orders = {tuple(np.argsort(-r, kind="stable")) for r in rest if len(set(r)) == 3}
    assert len(orders) == 6                                                         # the frame does hold all six tetrahedra
    assert any(r[0] == r[1] != r[2] for r in rest) and any(r[1] == r[2] != r[0] for r in rest) and any(r[0] == r[1] == r[2] != 0 for r in rest)
    w = 1024
    h = (len(rgb) + w - 1) // w
    px = np.zeros((h * w, 4), np.uint8)
    px[:len(rgb), 0], px[:len(rgb), 1], px[:len(rgb), 2] = rgb[:, 2], rgb[:, 1], rgb[:, 0]
    px[:, 3] = np.arange(h * w) % 251
    host = px.ravel()
    got, want = on_device(host, w, h, 4 * w, h * 4 * w, 1, name), emulated(host, w, h, 4 * w, h * 4 * w, 1, name)
    assert np.array_equal(got, want)
    assert np.array_equal(got[3::4], host[3::4])


@pytest.mark.gpu
def test_the_grey_table_reads_the_b_byte_alone_and_keeps_alpha():
    w, h = 256, 3
    px = np.zeros((h, w, 4), np.uint8)
    px[..., 0] = np.arange(256)                                                     # B: every value
    px[..., 1] = 255 - np.arange(256)                                               # G and R hold other values: they must not be read
    px[..., 2] = (np.arange(256) * 7 + 13) % 256
    px[0, :, 3], px[1, :, 3], px[2, :, 3] = 0, 1, 255
    host = px.ravel()
    got = on_device(host, w, h, 4 * w, h * 4 * w, 1, "gray").reshape(h, w, 4)
    table = links("gray")[1].table
    for c in range(3):
        assert np.array_equal(got[..., c], np.broadcast_to(table, (h, w)))
    assert np.array_equal(got[..., 3], px[..., 3])
    assert np.array_equal(got.ravel(), emulated(host, w, h, 4 * w, h * 4 * w, 1, "gray"))


@pytest.mark.gpu
def test_the_host_form_and_the_links_contents():
    w, h, stride = 37, 6, 4 * 37 + 8
    rng = np.random.default_rng(21)
    rows = np.full((h, stride), SENTINEL, np.uint8)
    rows[:, :4 * w] = rng.integers(0, 256, (h, 4 * w), dtype=np.uint8)
    native, emu = links("mAB")
    assert np.array_equal(CP.link_to_srgb_host(rows.copy(), w, native), L.transform(rows, w, emu))
    assert native.kind == CP.LINK_RGB and np.array_equal(native.nodes(), emu.nodes)


@pytest.mark.gpu
def test_the_batch_call_follows_a_late_stream_at_its_first_use_and_later():
    """tests/stream_order.py's late inputs.  First use: a fresh link, whose device copy is uploaded on the late stream (no plain run
    ahead of it: that would be the first use).  Later use: the same link, first from the default stream -- another stream than the
    upload's, which waits for the upload's event on the device -- then from the late stream again, where the call must return
    with the window open."""
    from tests import stream_order as SO
    try:
        S, Wt = SO.choose_streams(DEV)
    except SO.StreamOrderError as e:
        pytest.fail(str(e))
    try:
        icc, _ = profiles()["mft2"]
        emu = links("mft2")[1]
        fresh = CP.link_from_icc(icc)
        n, w, h, stride = 2, 67, 33, 4 * 67 + 4
        image_bytes = h * stride
        rng = np.random.default_rng(5)

        def frames(seed):
            r = np.random.default_rng(seed)
            f = np.full((n, h, stride), SENTINEL, np.uint8)
            f[:, :, :4 * w] = r.integers(0, 256, (n, h, 4 * w), dtype=np.uint8)
            return f
        real, decoy = frames(1), frames(2)
        exp = np.stack([L.transform(real[i], w, emu) for i in range(n)])
        guard = np.full(256, SENTINEL, np.uint8)
        t = torch.empty(n * image_bytes + 256, dtype=torch.uint8, device=DEV)
        buf = SO.Buf("frames", t, np.concatenate([real.ravel(), guard]), np.concatenate([decoy.ravel(), guard]), np.concatenate([exp.ravel(), guard]))
        bm = Bitmap(t[:n * image_bytes].view(n, image_bytes), w, h, stride)

        def call():
            CP.link_to_srgb(bm, fresh)
        first = SO.check_late("color_link_transform 67x33 mft2, first use", [buf], call, S, Wt, call_ms=2.0)
        later = SO.check_late("color_link_transform 67x33 mft2, later use", [buf], call, S, Wt)
        del rng
    except SO.StreamOrderError as e:
        pytest.fail(str(e))
    finally:
        # choose_streams took 8 of torch's 32 pooled streams: take the other 24, so that the stream-order tests that run after this
        # file are handed the very streams they were handed before it existed (tests/test_gpu_jpeg_progressive_stream_order.py)
        _ = [torch.cuda.Stream(DEV) for _ in range(24)]
    print("stream-order", first, later)
    assert first["checks"] == "a b c" and later["checks"] == "a b c"
    assert later["blocking"] is False, "a later use waited for the stream on the host"
    fresh.close()


def test_argument_checks_come_before_the_device_is_touched():
    """Bad arguments are argument errors with or without a GPU (the made-up pointers are never dereferenced: no kernel is launched
    for them); without one, a well-formed call gets as far as the device check."""
    lib = CP._bind()
    link = links("mft2")[0]
    Wd, H, STRIDE = 37, 23, 4 * 37 + 12
    p = 0x7F0000000000

    def call(ptr=p, image_bytes=H * STRIDE, n=1, w=Wd, h=H, stride=STRIDE, handle=link.p):
        return lib.ifhip_color_link_transform_batch_device(ptr, image_bytes, n, w, h, stride, handle, None)
    assert call(ptr=None) == INVALID
    assert call(handle=None) == INVALID
    assert call(stride=4 * Wd - 4) == INVALID
    assert call(stride=STRIDE + 2) == INVALID
    assert call(ptr=p + 2) == INVALID
    assert call(w=0) == INVALID and call(h=0) == INVALID
    assert call(image_bytes=(H - 1) * STRIDE + 4 * Wd - 4) == INVALID
    assert call(n=65536) == INVALID
    assert call(n=0, ptr=None) == 0
    frame = (C.c_uint8 * (H * STRIDE))()
    assert lib.ifhip_color_link_transform(frame, Wd, H, 4 * Wd - 4, link.p) == INVALID
    assert lib.ifhip_color_link_transform(None, Wd, H, STRIDE, link.p) == INVALID
    assert lib.ifhip_color_link_transform(frame, Wd, H, STRIDE, None) == INVALID
    small = (C.c_uint8 * 16)()
    assert lib.ifhip_color_link_copy_nodes(link.p, small, 16, None) == INVALID
    if not torch.cuda.is_available():
        unavailable = (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
        assert call() in unavailable
        assert lib.ifhip_color_link_transform(frame, Wd, H, STRIDE, link.p) in unavailable
