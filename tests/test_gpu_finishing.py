"""round_image_corners and white_balance_histogram_area_threshold_srgb on the GPU (csrc/round_corners.hip,
csrc/white_balance.hip, csrc/abi_shim.cpp):
  * the reference's seven synthetic round-corner jobs (visuals/canvas.rs:240-388), sent as JSON through the C ABI, hash to
    the ids canvas.checksums stores;
  * both batch entry points equal the CPU restatements (tests/rounded_corners_oracle.py, tests/white_balance_oracle.py)
    over sizes, strides, mixed batches, radius modes, mattes, thresholds and contents, with a guard region behind the frames;
  * d_histograms equals a bincount;
  * s.roundcorners / a.balancewhite in a querystring give the bytes of the explicit graph, on raw and JPEG input;
  * a shared parent keeps its pixels."""
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from imageflow_amd.graphics.rounded_corners import clear_around_rounded_corners  # noqa: E402
from imageflow_amd.graphics.white_balance import white_balance_srgb  # noqa: E402
from tests import rounded_corners_oracle as R  # noqa: E402
from tests import white_balance_oracle as WB  # noqa: E402
from tests.seahash import bitmap_checksum, checksum_id_digits  # noqa: E402
from tests.test_finishing_oracle import REFERENCE_JOBS, color32  # noqa: E402

DEV = "cuda:0"
GUARD = 0x5A
RAW = {"lodepng": {"maximum_deflate": False}}       # this shim writes its raw BGRA container for non-JPEG presets


def _run(ctx, method, job, expect=200):
    status, r = ctx.send_json(method, job)
    assert status == expect, (status, r, ctx.error_message())
    return r


def _pixels(buf):
    rows, w, h, alpha = unpack_raw_bgra(buf)
    return rows[:, :4 * w].reshape(h, w, 4), alpha


def _color(hex8):
    return {"srgb": {"hex": hex8}}


@pytest.mark.parametrize("name", list(REFERENCE_JOBS))
def test_reference_round_corner_jobs_hash_to_the_reference_checksums(name):
    w, h, bg, matte, mode, radii, want = REFERENCE_JOBS[name]
    if mode == "circle":
        radius = "circle"
    elif mode == "pixels":
        radius = {"pixels": radii[0]}
    else:
        radius = {mode: dict(zip(("top_left", "top_right", "bottom_right", "bottom_left"), radii))}
    steps = [{"create_canvas": {"w": w, "h": h, "format": "bgra_32", "color": _color(bg)}},
             {"round_image_corners": {"radius": radius, "background_color": _color(matte)}},
             {"encode": {"io_id": 1, "preset": RAW}}]
    with Context() as c:
        c.add_output_buffer(1)
        _run(c, "v1/execute", {"framewise": {"steps": steps}})
        px, _ = _pixels(c.get_output_buffer(1))
    assert checksum_id_digits(px) == want, bitmap_checksum(px)


# ---- device sweeps against the restatements ---------------------------------------------------------------------------
def _batch(frames, w, h, pad_bytes, seed):
    """frames [n][h][w][4] -> (Bitmap over a buffer with a guard region behind it, the buffer, the host image)"""
    n = len(frames)
    stride = 4 * w + pad_bytes
    host = np.random.default_rng(seed).integers(0, 256, (n, h, stride), dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i, :, :4 * w] = f.reshape(h, 4 * w)
    buf = torch.full((n * h * stride + 4096,), GUARD, dtype=torch.uint8, device=DEV)
    buf[:n * h * stride] = torch.from_numpy(host.reshape(-1)).to(DEV)
    return Bitmap(buf[:n * h * stride].view(n, h * stride), w, h, stride), buf, host


def _collect(buf, host, w, h):
    n, _, stride = host.shape
    out = buf.cpu().numpy()
    assert (out[n * h * stride:] == GUARD).all(), "write behind the frames"
    out = out[:n * h * stride].reshape(n, h, stride)
    assert np.array_equal(out[:, :, 4 * w:], host[:, :, 4 * w:]), "write into the row padding"
    return out[:, :, :4 * w].reshape(n, h, w, 4)


def _content(kind, w, h, rng):
    if kind == "constant":
        f = np.empty((h, w, 4), np.uint8)
        f[:] = rng.integers(0, 256, 4, dtype=np.uint8)
        return f
    f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "alpha0":
        f[..., 3] = np.where(rng.random((h, w)) < 0.5, 0, f[..., 3])
    elif kind == "narrow":                                         # low contrast: white balance stretches it
        f[..., :3] = 60 + f[..., :3] // 3
    elif kind == "bimodal":
        f[..., :3] = np.where(rng.random((h, w, 1)) < 0.5, 30, 210)
    return f


RC_SIZES = [(1, 1), (1, 9), (9, 1), (2, 3), (5, 5), (17, 4), (99, 100), (100, 99), (64, 37), (150, 200), (201, 150)]
RC_MODES = [("percentage", [0.0]), ("percentage", [10.0]), ("percentage", [33.3]), ("percentage", [250.0]), ("percentage", [-5.0]),
            ("pixels", [0.5]), ("pixels", [2.25]), ("pixels", [7.0]), ("pixels", [1000.0]), ("circle", [0.0]),
            ("percentage_custom", [0.0, 10.0, 50.0, 100.0]), ("percentage_custom", [12.5, 0.0, 99.0, 3.0]),
            ("pixels_custom", [0.0, 1.0, 50.0, 20.0]), ("pixels_custom", [3.7, 1000.0, 0.25, 9.0])]
MATTES = [0xFF0000FF, 0x80102030, 0x00000000, 0x00FFFFFF]


@pytest.mark.parametrize("w,h", RC_SIZES)
def test_round_corners_batch_equals_the_restatement(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    mismatches = []
    for mode, radii in RC_MODES:
        for matte in MATTES:
            frames = [_content(k, w, h, rng) for k in ("random", "alpha0", "constant")]      # one mixed batch
            b, buf, host = _batch(frames, w, h, 4 * int(rng.integers(0, 6)), int(rng.integers(1 << 30)))
            clear_around_rounded_corners(b, mode, radii, matte)
            got = _collect(buf, host, w, h)
            for i, f in enumerate(frames):
                want = R.clear_around_rounded_corners(f.copy(), mode, (radii * 4)[:4], matte)
                if not np.array_equal(got[i], want):
                    mismatches.append((mode, radii, hex(matte), i, int((got[i] != want).any(-1).sum())))
    assert not mismatches, mismatches[:8]


def test_round_corners_on_a_4k_frame():
    rng = np.random.default_rng(4)
    f = _content("alpha0", 3840, 2160, rng)
    for mode, radii, matte in (("percentage", [10.0], 0x80FFFFFF), ("circle", [0.0], 0xFF000000)):
        b, buf, host = _batch([f], 3840, 2160, 64, 1)
        clear_around_rounded_corners(b, mode, radii, matte)
        got = _collect(buf, host, 3840, 2160)[0]
        assert np.array_equal(got, R.clear_around_rounded_corners(f.copy(), mode, radii * 4, matte)), mode


WB_SIZES = [(1, 1), (1, 300), (300, 1), (3, 5), (37, 29), (255, 257), (640, 480), (1001, 3)]
THRESHOLDS = [None, 0.0, 0.5, 1.0, -1.0, 0.02]
WB_KINDS = ["random", "constant", "narrow", "bimodal"]


@pytest.mark.parametrize("w,h", WB_SIZES)
def test_white_balance_batch_and_histograms_equal_the_restatement(w, h):
    rng = np.random.default_rng(w * 7 + h)
    mismatches = []
    for t in THRESHOLDS:
        frames = [_content(k, w, h, rng) for k in WB_KINDS]
        b, buf, host = _batch(frames, w, h, 4 * int(rng.integers(0, 6)), int(rng.integers(1 << 30)))
        hist = torch.full((len(frames) * 768 + 8,), -7, dtype=torch.int64, device=DEV)
        white_balance_srgb(b, t, hist)
        got = _collect(buf, host, w, h)
        hs = hist.cpu().numpy()
        assert (hs[len(frames) * 768:] == -7).all(), "write behind the histograms"
        for i, f in enumerate(frames):
            assert np.array_equal(hs[i * 768:(i + 1) * 768].reshape(3, 256), WB.histograms(f).astype(np.int64)), (t, i)
            want = WB.white_balance(f.copy(), t)
            if not np.array_equal(got[i], want):
                mismatches.append((t, WB_KINDS[i], int((got[i] != want).any(-1).sum())))
    assert not mismatches, mismatches[:8]


@pytest.mark.parametrize("kind", ["random", "constant", "narrow"])
def test_white_balance_on_4k_frames(kind):
    rng = np.random.default_rng(9)
    frames = [_content(kind, 3840, 2160, rng) for _ in range(2)]
    b, buf, host = _batch(frames, 3840, 2160, 0, 2)
    white_balance_srgb(b)
    got = _collect(buf, host, 3840, 2160)
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], WB.white_balance(f.copy())), i


# ---- nodes, querystring, shared parents ---------------------------------------------------------------------------------
def _photo(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 4), np.uint8)
    f[..., 0] = 40 + (x * 150) // w
    f[..., 1] = 50 + (y * 120) // h
    f[..., 2] = 70 + rng.integers(0, 90, (h, w))
    f[..., 3] = 255
    return f


def _jpeg(img):
    PIL = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    PIL.fromarray(np.ascontiguousarray(img[..., 2::-1])).save(b, "JPEG", quality=90, subsampling="4:2:0")
    return b.getvalue()


def _encode_one(data, steps):
    with Context() as c:
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        _run(c, "v1/build", {"io": [{"io_id": 0, "direction": "in", "io": "placeholder"}, {"io_id": 1, "direction": "out", "io": "placeholder"}],
                             "framewise": {"steps": steps}})
        return c.get_output_buffer(1)


QS_CASES = [
    ("width=400&s.roundcorners=10", "width=400", [{"round_image_corners": {"radius": {"percentage": 10.0}, "background_color": "transparent"}}], False),
    ("s.roundcorners= 5, 10,15 ,20&width=400", "width=400",
     [{"round_image_corners": {"radius": {"percentage_custom": {"top_left": 5, "top_right": 10, "bottom_right": 15, "bottom_left": 20}},
                               "background_color": "transparent"}}], False),
    ("width=400&a.balancewhite=true", "width=400", [{"white_balance_histogram_area_threshold_srgb": {"threshold": None}}], False),
    ("width=400&a.balancewhite=Area&s.roundcorners=30&format=jpg", "width=400&format=jpg",
     [{"round_image_corners": {"radius": {"percentage": 30.0}, "background_color": _color("FFFFFFFF")}},
      {"white_balance_histogram_area_threshold_srgb": {}}], True),
    ("width=400&s.roundcorners=12&quality=abc", "width=400&quality=abc",          # quality=abc: a JPEG, but transparent corners
     [{"round_image_corners": {"radius": {"percentage": 12.0}, "background_color": "transparent"}}], True),
    ("width=400&a.balancewhite=gimp&s.roundcorners=1,2", "width=400", [], False),  # neither key adds a node
]


@pytest.mark.parametrize("source", ["raw", "jpeg"])
@pytest.mark.parametrize("qs,rest,nodes,jpeg_out", QS_CASES)
def test_querystring_equals_the_explicit_graph(source, qs, rest, nodes, jpeg_out):
    src = _photo(640, 420, 3)
    data = pack_raw_bgra(src.reshape(420, 4 * 640), 640, 420, alpha_meaningful=False) if source == "raw" else _jpeg(src)
    a = _encode_one(data, [{"command_string": {"kind": "ir4", "value": qs, "decode": 0, "encode": 1}}])
    preset = {"libjpeg_turbo": {"quality": 90}} if jpeg_out else RAW
    b = _encode_one(data, [{"decode": {"io_id": 0}}, {"command_string": {"kind": "ir4", "value": rest}}] + nodes
                    + [{"encode": {"io_id": 1, "preset": preset}}])
    assert a == b
    if not jpeg_out and any("round_image_corners" in n for n in nodes):
        px, alpha = _pixels(a)
        assert alpha and px[0, 0, 3] == 0 and px[px.shape[0] // 2, px.shape[1] // 2, 3] == 255   # transparent corners
    if "format=jpg" in qs:
        PIL = pytest.importorskip("PIL.Image")
        corner = np.asarray(PIL.open(io.BytesIO(a)).convert("RGB"))[0, 0]
        assert corner.min() >= 250                                                              # white corners


def _graph_two_outputs(first, node):
    nodes = {"0": first, "1": node, "2": {"encode": {"io_id": 1, "preset": RAW}}, "3": {"encode": {"io_id": 2, "preset": RAW}}}
    edges = [{"from": a, "to": b, "kind": "input"} for a, b in ((0, 1), (0, 2), (1, 3))]
    return {"framewise": {"graph": {"nodes": nodes, "edges": edges}}}


@pytest.mark.parametrize("node", [
    {"round_image_corners": {"radius": {"pixels": 9}, "background_color": _color("33669980")}},
    {"white_balance_histogram_area_threshold_srgb": {"threshold": 0.01}},
    {"command_string": {"kind": "ir4", "value": "s.roundcorners=20&a.balancewhite=true"}},
])
def test_a_shared_parent_keeps_its_pixels(node):
    src = _photo(90, 70, 5)
    qs = "command_string" in node                  # Bgr32: the same-size resample hands its input on, the keys must copy it
    if not qs:
        src[..., 3] = np.random.default_rng(1).integers(0, 256, (70, 90))
    with Context() as c:
        c.add_input_buffer(0, pack_raw_bgra(src.reshape(70, 360), 90, 70, alpha_meaningful=not qs))
        c.add_output_buffer(1)
        c.add_output_buffer(2)
        job = _graph_two_outputs({"decode": {"io_id": 0}}, node)
        job["io"] = [{"io_id": 0, "direction": "in", "io": "placeholder"}, {"io_id": 1, "direction": "out", "io": "placeholder"},
                     {"io_id": 2, "direction": "out", "io": "placeholder"}]
        _run(c, "v1/build", job)
        parent, _ = _pixels(c.get_output_buffer(1))
        child, _ = _pixels(c.get_output_buffer(2))
    assert np.array_equal(parent, src)
    want = src.copy()
    if "round_image_corners" in node:
        R.clear_around_rounded_corners(want, "pixels", [9.0] * 4, color32("33669980"))
    elif "white_balance_histogram_area_threshold_srgb" in node:
        WB.white_balance(want, 0.01)
    else:
        R.round_image_corners(want, False, "percentage", [20.0] * 4, 0)
        WB.white_balance(want)
    assert np.array_equal(child, want)


def test_bgr32_frame_gains_alpha_for_a_transparent_matte_only():
    src = _photo(60, 50, 7)
    data = pack_raw_bgra(src.reshape(50, 240), 60, 50, alpha_meaningful=False)
    for matte, alpha_after in (("00000000", True), ("102030FF", False)):
        out = _encode_one(data, [{"decode": {"io_id": 0}}, {"round_image_corners": {"radius": {"pixels": 12}, "background_color": _color(matte)}},
                                 {"encode": {"io_id": 1, "preset": RAW}}])
        px, alpha = _pixels(out)
        want = src.copy()
        R.round_image_corners(want, False, "pixels", [12.0] * 4, color32(matte))
        assert alpha == alpha_after and np.array_equal(px, want), matte


def test_node_parameter_errors():
    for node in ({"round_image_corners": {"radius": {"pixels": 5}}},                              # background_color required
                 {"round_image_corners": {"radius": "square", "background_color": "black"}},
                 {"round_image_corners": {"radius": {"pixels_custom": {"top_left": 1}}, "background_color": "black"}},
                 {"white_balance_histogram_area_threshold_srgb": {"threshold": "high"}}):
        with Context() as c:
            c.add_output_buffer(1)
            status, _ = c.send_json("v1/execute", {"framewise": {"steps": [
                {"create_canvas": {"w": 20, "h": 20, "format": "bgra_32", "color": "black"}}, node, {"encode": {"io_id": 1, "preset": RAW}}]}})
            assert status == 400, node
