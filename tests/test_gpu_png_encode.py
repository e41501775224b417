"""The device PNG coder on an MI355X (csrc/png_encode.hip through imageflow_amd.codecs.libpng_encoder and the `libpng`
preset of `encode`): every file is parsed by the test-side oracle (tests/png_oracle.py: all CRCs, zlib's inflate with the
Adler-32), opened by Pillow, and compared with the source pixels and with the oracle's filter choice; the size conditions
are the ones the feature was accepted under -- stored is the floor, runs are found, and the photo and product frames are
not larger than zlib level 1 with Z_FILTERED on the oracle's own filtered stream."""
import ctypes as C
import io
import json

import numpy as np
import pytest
from PIL import Image

torch = pytest.importorskip("torch")

from imageflow_amd.codecs import libpng_encoder as PNG  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import png_oracle as P  # noqa: E402
from tests import util as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 32768
Image.MAX_IMAGE_PIXELS = None


def bgra_from_rgba(px, stride=None):
    """uint8 [h, w, 3 or 4] RGB(A) -> one BGRA frame [h, stride]; the padding is filled with 0xA5 so that a leak shows."""
    h, w, bpp = px.shape
    stride = stride or U.stride_for(w)
    out = np.full((h, stride), 0xA5, np.uint8)
    v = out[:, :4 * w].reshape(h, w, 4)
    v[..., 0], v[..., 1], v[..., 2] = px[..., 2], px[..., 1], px[..., 0]
    v[..., 3] = px[..., 3] if bpp == 4 else 255
    return out


def rgba_from_bgra(frame, w):
    v = frame[:, :4 * w].reshape(frame.shape[0], w, 4)
    return np.ascontiguousarray(v[..., [2, 1, 0, 3]])


def bitmap(frames, w, h, alpha=True):
    frames = np.ascontiguousarray(frames)
    return Bitmap.from_numpy(frames, w, h, frames.shape[-1], DEV, alpha_meaningful=alpha)


def stored_bound(n, chunks):
    """exact arithmetic of the deflate format: stored blocks of at most 65535 bytes, the zlib header and Adler-32, and the 5
    bytes of the empty stored block that closes a chunk to a byte boundary"""
    return n + 5 * -(-n // 65535) + 6 + 5 * chunks


def check_file(data, rgba, color_type, slow_unfilter=None):
    """Everything a file must be, against the source pixels rgba [h, w, 4].  Returns the oracle's dict."""
    h, w, _ = rgba.shape
    want = rgba if color_type == PNG.PNG_RGBA else np.ascontiguousarray(rgba[..., :3])
    small = w * h <= 300 * 300 if slow_unfilter is None else slow_unfilter
    d = P.decode(data, pixels=small)
    assert (d["width"], d["height"], d["color_type"]) == (w, h, color_type)
    P.check_ancillary(d["chunks"])
    filters, stream = P.filter_image(want)
    assert np.array_equal(d["filters"], filters), "every row's filter type is the oracle's choice"
    assert d["stream"] == stream, "the filtered stream (so the pixels: the filters are bijections)"
    if small:
        assert np.array_equal(d["pixels"], want)
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.mode == ("RGBA" if color_type == PNG.PNG_RGBA else "RGB") and im.size == (w, h)
    assert np.array_equal(np.asarray(im), want)
    n = len(stream)
    print(f"{w}x{h} ct{color_type}: IDAT {len(d['idat'])} of {n} filtered bytes")
    assert len(d["idat"]) <= stored_bound(n, -(-n // CHUNK)), "never worse than stored"
    return d


def flat_frame(w, h):
    px = np.zeros((h, w, 4), np.uint8)
    px[...] = (40, 90, 200, 255)
    return px


def frame_set(w, h):
    out = {
        "gradient": rgba_from_bgra(U.gradient_frames(1, w, h, 3)[0], w),
        "random": rgba_from_bgra(U.random_frames(1, w, h, 1234)[0], w),
        "flat": flat_frame(w, h),
        "photo": np.dstack([P.photo_frame(w, h), np.full((h, w), 255, np.uint8)]),
    }
    if w == h and w >= 8:
        out["product"] = P.product_frame(w)
    return out


SIZES = [(1, 1, None), (1, 300, None), (300, 1, None), (37, 23, 4 * 37 + 8), (800, 450, None), (800, 800, None)]


@pytest.mark.parametrize("color_type", [PNG.PNG_RGB, PNG.PNG_RGBA])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip_is_exact_and_rows_carry_libpngs_filter(size, color_type):
    w, h, stride = size
    frames = frame_set(w, h)
    names = sorted(frames)
    batch = np.stack([bgra_from_rgba(frames[k], stride) for k in names])
    stage = PNG.PngEncodeStage(w, h, color_type, len(names), DEV)
    files, status = stage.encode(bitmap(batch, w, h))
    assert status == [0] * len(names)
    for k, data in zip(names, files):
        print(k, end=": ")
        check_file(data, frames[k], color_type)
    # image i of a batch equals the same image encoded alone, and the same pixels give the same bytes on every run
    alone = PNG.PngEncodeStage(w, h, color_type, 1, DEV)
    for i in (0, len(names) - 1):
        one, _ = alone.encode(bitmap(batch[i:i + 1], w, h))
        assert one[0] == files[i]
    again, _ = stage.encode(bitmap(batch, w, h))
    assert again == files


def test_transparent_pixels_keep_their_colour():
    w, h = 64, 40
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[::2, :, 3] = 0                                                  # fully transparent, colour bytes non-zero
    data = PNG.PngEncodeStage(w, h, PNG.PNG_RGBA, 1, DEV).encode(bitmap(bgra_from_rgba(px)[None], w, h))[0][0]
    d = check_file(data, px, PNG.PNG_RGBA)
    assert np.array_equal(d["pixels"][::2, :, :3], px[::2, :, :3])


@pytest.mark.parametrize("color_type", [PNG.PNG_RGB, PNG.PNG_RGBA])
def test_a_2160p_frame(color_type):
    w, h = 3840, 2160
    px = np.dstack([P.photo_frame(w, h, 21), np.full((h, w), 255, np.uint8)])
    px[200:900, 300:2000] = (255, 255, 255, 0 if color_type == PNG.PNG_RGBA else 255)
    data = PNG.PngEncodeStage(w, h, color_type, 1, DEV).encode(bitmap(bgra_from_rgba(px)[None], w, h))[0][0]
    check_file(data, px, color_type)


def test_size_conditions():
    """1: never worse than stored (check_file asserts it for every frame, random noise included).  2: a flat 1024 x 1024
    frame's IDAT payload is at most 1 % of its filtered length.  3: on the photo 800 x 450 RGB and product 800 x 800 RGBA
    frames the IDAT payload is <= R1, zlib level 1 with Z_FILTERED on the oracle's own filtered stream; no margin."""
    flat = flat_frame(1024, 1024)
    for ct in (PNG.PNG_RGB, PNG.PNG_RGBA):
        data = PNG.PngEncodeStage(1024, 1024, ct, 1, DEV).encode(bitmap(bgra_from_rgba(flat)[None], 1024, 1024))[0][0]
        d = check_file(data, flat, ct, slow_unfilter=False)
        assert len(d["idat"]) * 100 <= len(d["stream"]), (len(d["idat"]), len(d["stream"]))
    photo = np.dstack([P.photo_frame(800, 450), np.full((450, 800), 255, np.uint8)])
    product = P.product_frame(800)
    for name, px, ct in (("photo", photo, PNG.PNG_RGB), ("product", product, PNG.PNG_RGBA), ("photo", photo, PNG.PNG_RGBA), ("product", product, PNG.PNG_RGB)):
        h, w, _ = px.shape
        data = PNG.PngEncodeStage(w, h, ct, 1, DEV).encode(bitmap(bgra_from_rgba(px)[None], w, h))[0][0]
        d = check_file(data, px, ct, slow_unfilter=False)
        s, r1, r6 = len(d["idat"]), P.reference_size(d["stream"], 1), P.reference_size(d["stream"], 6)
        print(f"{name} ct{ct}: S {s} R1 {r1} R6 {r6} S/R1 {s / r1:.4f} S/R6 {s / r6:.4f}")
        assert s <= r1


def test_zlib_level_0_writes_stored_blocks_and_levels_share_one_strategy():
    w, h = 300, 200
    px = np.dstack([P.photo_frame(w, h, 2), np.full((h, w), 255, np.uint8)])
    stage = PNG.PngEncodeStage(w, h, PNG.PNG_RGBA, 1, DEV)
    b = bitmap(bgra_from_rgba(px)[None], w, h)
    stored = stage.encode(b, 0)[0][0]
    d = check_file(stored, px, PNG.PNG_RGBA)
    assert P.stored_only(d["idat"])
    n = len(d["stream"])
    assert len(d["idat"]) == n + 5 * -(-n // CHUNK) + 6
    files = {lv: stage.encode(b, lv)[0][0] for lv in (-1, 1, 6, 9)}
    idats = {lv: P.decode(f, pixels=False)["idat"] for lv, f in files.items()}
    assert len({v[2:] for v in idats.values()}) == 1                   # only the zlib header's FLEVEL bits differ
    assert files[-1] == files[6] and not P.stored_only(idats[6])


def test_dropin_equals_the_device_form():
    w, h, stride = 37, 23, 4 * 37 + 8
    px = rgba_from_bgra(U.random_frames(1, w, h, 77)[0], w)
    frame = bgra_from_rgba(px, stride)
    for ct in (PNG.PNG_RGB, PNG.PNG_RGBA):
        host = PNG.encode_png_host(frame, w, h, stride, ct)
        dev = PNG.PngEncodeStage(w, h, ct, 1, DEV).encode(bitmap(frame[None], w, h))[0][0]
        assert host == dev
        check_file(host, px, ct)


def test_guard_regions_and_file_overflow():
    w, h, n = 120, 90, 3
    frames = np.stack([bgra_from_rgba(rgba_from_bgra(U.random_frames(1, w, h, 300 + i)[0], w)) for i in range(n)])
    stage = PNG.PngEncodeStage(w, h, PNG.PNG_RGBA, n, DEV)
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    guard = 4096
    files = torch.full((n * pitch + guard,), 0x5C, dtype=torch.uint8, device=DEV)
    lengths = torch.full((n + 64,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((n + 64,), -9, dtype=torch.int32, device=DEV)
    out, _, _ = stage.encode_device(bitmap(frames, w, h), 6, pitch, files[:n * pitch].view(n, pitch), lengths, status)
    torch.cuda.synchronize()
    assert bool((files[n * pitch:] == 0x5C).all()) and bool((lengths[n:] == -7).all()) and bool((status[n:] == -9).all())
    ln = lengths[:n].cpu().numpy()
    assert (status[:n].cpu().numpy() == 0).all() and (ln > 0).all() and (ln <= stage.max_file_bytes).all()
    host = files.cpu().numpy()
    for i in range(n):
        assert (host[i * pitch + ln[i]:(i + 1) * pitch] == 0x5C).all(), "nothing behind a file's end is touched"
        check_file(host[i * pitch:i * pitch + ln[i]].tobytes(), rgba_from_bgra(frames[i], w), PNG.PNG_RGBA)
    # a pitch below the file: the image is dropped with the status word, nothing is written
    small = 4096
    files2 = torch.full((n * small + guard,), 0x5C, dtype=torch.uint8, device=DEV)
    _, l2, s2 = stage.encode_device(bitmap(frames, w, h), 6, small, files2[:n * small].view(n, small))
    torch.cuda.synchronize()
    assert l2.cpu().tolist() == [0] * n and s2.cpu().tolist() == [PNG.PNG_FILE_OVERFLOW] * n
    assert bool((files2 == 0x5C).all())


def test_short_image_bytes_is_refused_on_the_device():
    w, h, stride = 37, 23, 4 * 37 + 8
    frame = torch.zeros(h * stride, dtype=torch.uint8, device=DEV)
    stage = PNG.PngEncodeStage(w, h, PNG.PNG_RGBA, 1, DEV)
    files = torch.zeros(stage.max_file_bytes + 16, dtype=torch.uint8, device=DEV)
    ln = torch.zeros(2, dtype=torch.int32, device=DEV)
    L = PNG._bind()
    short = (h - 1) * stride + 4 * w - 4
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(DEV):
        assert L.ifhip_png_encode_batch_device(stage._h, frame.data_ptr(), short, stride, 1, 6, files.data_ptr(), files.numel(), ln.data_ptr(), None, stream) == 1
        assert L.ifhip_png_encode_batch_device(stage._h, frame.data_ptr(), short + 4, stride, 1, 6, files.data_ptr(), files.numel(), ln.data_ptr(), None, stream) == 0
        torch.cuda.synchronize()
    assert int(ln[0]) > 0


# ---- the `libpng` preset of `encode` (csrc/abi_shim.cpp) ------------------------------------------------------------------------

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from oracle import oracle as O  # noqa: E402

RAW = {"lodepng": {"maximum_deflate": False}}          # still this shim's raw BGRA container
MATTE = {"srgb": {"hex": "999999"}}
PRESETS = [{"libpng": {}}, {"libpng": {"depth": "png_24"}}, {"libpng": {"matte": MATTE}}, {"libpng": {"zlib_compression": 0}}]


def _run(ctx, job, expect=200):
    status, r = ctx.send_json("v1/execute", job)
    assert status == expect, (status, r, ctx.error_message())
    return r


def _jpeg_input(w=203, h=131):
    rgb = P.photo_frame(w, h, 9)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=85)
    return b.getvalue()


def _chains():
    src = np.ascontiguousarray(bgra_from_rgba(P.product_frame(160)))
    rounded = [{"decode": {"io_id": 0}},
               {"round_image_corners": {"radius": {"pixels": 40.0}, "background_color": "transparent"}}]
    return {"rounded": (pack_raw_bgra(src, 160, 160, alpha_meaningful=True), rounded),
            "jpeg": (_jpeg_input(), [{"decode": {"io_id": 0}}])}


def _encode_both(data, steps, preset):
    """The chain once with `preset` and once with the raw container; returns (file, response entry, raw rows, w, h, alpha)."""
    with Context() as c:
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        r = _run(c, {"framewise": {"steps": steps + [{"encode": {"io_id": 1, "preset": preset}}]}})
        got = bytes(c.get_output_buffer(1))
    with Context() as c:
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        _run(c, {"framewise": {"steps": steps + [{"encode": {"io_id": 1, "preset": RAW}}]}})
        raw = bytes(c.get_output_buffer(1))
        assert raw[:7] == b"IFBGRA1", "the lodepng preset still returns the raw container"
        rows, w, h, alpha = unpack_raw_bgra(raw)
    return got, r["data"]["job_result"]["encodes"][0], rows, w, h, alpha


@pytest.mark.parametrize("preset", PRESETS, ids=lambda p: json.dumps(p["libpng"]))
@pytest.mark.parametrize("chain", ["rounded", "jpeg"])
def test_libpng_preset_writes_the_chains_pixels(chain, preset):
    data, steps = _chains()[chain]
    got, enc, rows, w, h, alpha = _encode_both(data, steps, preset)
    assert (enc["preferred_mime_type"], enc["preferred_extension"], enc["w"], enc["h"]) == ("image/png", "png", w, h)
    assert alpha == (chain == "rounded")
    opts = preset["libpng"]
    frame = np.ascontiguousarray(rows)
    if "matte" in opts and alpha:                                   # applied only when given, only to meaningful alpha; opaque: clears it
        assert O.apply_matte(frame, w, h, frame.shape[1], 0xFF999999, True) == 0
        alpha = False
    want_ct = PNG.PNG_RGB if (not alpha or opts.get("depth") == "png_24") else PNG.PNG_RGBA
    d = check_file(got, rgba_from_bgra(frame, w), want_ct)
    if opts.get("zlib_compression") == 0:
        assert P.stored_only(d["idat"])
    if chain == "rounded" and want_ct == PNG.PNG_RGBA:
        assert (d["pixels"][..., 3] == 0).any() and (d["pixels"][..., 3] == 255).any()


def test_zlib_compression_is_clamped_like_the_reference():
    data, steps = _chains()["jpeg"]
    files = {}
    for v in (None, -3, 6, 12, 300):
        opts = {} if v is None else {"zlib_compression": v}
        files[v] = _encode_both(data, steps, {"libpng": opts})[0]
    assert files[None] == files[6] == files[12] == files[300]                      # above 9: the default
    assert P.stored_only(P.decode(files[-3], pixels=False)["idat"])                 # negatives clamp to 0: stored


def test_unknown_depth_is_invalid_json():
    data, steps = _chains()["jpeg"]
    with Context() as c:
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": steps + [{"encode": {"io_id": 1, "preset": {"libpng": {"depth": "png_8"}}}}]}})
        assert status != 200 and "InvalidJson" in r["message"]


def test_a_shared_frame_keeps_its_pixels_under_a_matte():
    src = np.ascontiguousarray(bgra_from_rgba(P.product_frame(96)))
    with Context() as c:
        c.add_input_buffer(0, pack_raw_bgra(src, 96, 96, alpha_meaningful=True))
        c.add_output_buffer(1)
        c.add_output_buffer(2)
        _run(c, {"framewise": {"graph": {
            "nodes": {"0": {"decode": {"io_id": 0}}, "1": {"encode": {"io_id": 1, "preset": {"libpng": {"matte": MATTE}}}},
                      "2": {"encode": {"io_id": 2, "preset": RAW}}},
            "edges": [{"from": 0, "to": 1, "kind": "input"}, {"from": 0, "to": 2, "kind": "input"}]}}})
        png = bytes(c.get_output_buffer(1))
        rows, w, h, alpha = unpack_raw_bgra(c.get_output_buffer(2))
    assert alpha and np.array_equal(rows[:, :4 * w], src[:, :4 * w]), "the other consumer's pixels are untouched"
    matted = src.copy()
    assert O.apply_matte(matted, 96, 96, matted.shape[1], 0xFF999999, True) == 0
    check_file(png, rgba_from_bgra(matted, 96), PNG.PNG_RGB)
