"""The device palette quantiser's algorithm without a device (csrc/png_quantize_core.hpp: histogram keys, palette growth,
Lloyd refinement, the nearest-entry search, Floyd-Steinberg error diffusion, the palette framing -- what the gfx950 kernels
of csrc/png_quantize.hip are built from).  tests/png_quantize_emulate.cpp runs the passes on the CPU; Pillow and zlib read
what comes out, and Pillow's own quantisers are the yardstick of the palette's quality.  The GPU tests
(tests/test_gpu_png_quantize.py) hold the kernels to this emulation byte for byte.

Measured with Pillow 12.2.0 (squared error summed over R, G, B, mean over pixels; photo_frame(256, 160), 256 colours,
undithered): this quantiser 100.0, MEDIANCUT 178.9, MAXCOVERAGE 159.1, FASTOCTREE 321.3.  With real alpha, on premultiplied
values (R, G, B times alpha / 255, and alpha): this quantiser 62.8 on the 160 x 160 frame used below, FASTOCTREE 332.9.
Dithering, 256 x 64 ramps at 16 colours: error of the 8 x 8 box means 137.0 dithered against 370.7 plain, a ratio of 0.37."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_oracle as P
from tests import png_quantize_emu as E


def rgb_error(a, b):
    return ((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2).sum(-1).mean()


def premultiplied_error(a, b):
    def pre(v):
        v = v.astype(np.float64)
        return np.dstack([v[..., :3] * v[..., 3:] / 255.0, v[..., 3:]])
    return ((pre(a) - pre(b)) ** 2).sum(-1).mean()


@pytest.fixture(scope="module")
def photo():
    return E.photo_rgba(256, 160)


# ---- exactness ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", [False, True], ids=["opaque", "alpha"])
@pytest.mark.parametrize("n_colors", [1, 2, 256])
def test_at_most_256_colours_are_kept_exactly(n_colors, alpha):
    w, h = 40, 30
    rgba = E.colour_frame(w, h, n_colors, seed=n_colors, alpha=alpha)
    if alpha and n_colors == 256:
        rgba[rgba[..., 3] == rgba[0, 0, 3]] = (77, 66, 55, 0)         # one of the values becomes "transparent, with a colour"
    q = E.quantize(rgba, alpha=alpha)
    src = E.normalized(rgba, alpha)
    want = np.unique(src.reshape(-1, 4), axis=0)
    assert q["status"] == 0 and q["mse"] == 0.0
    assert sorted(map(tuple, q["palette"])) == sorted(map(tuple, want)), "the palette is exactly the set of values"
    assert np.array_equal(q["palette"][q["indices"]], src), "every pixel decodes to its source value; dithering changes nothing"
    n_trans = int((want[:, 3] < 255).sum())
    assert q["n_trans"] == n_trans
    d = E.check_palette_file(q["file"], w, h, q["palette"], q["indices"])
    assert len(d.get(b"tRNS", b"")) == n_trans
    plain = E.quantize(rgba, alpha=alpha, dither=False, file=False)
    assert np.array_equal(plain["indices"], q["indices"])


def test_a_frame_that_is_transparent_throughout():
    rgba = np.zeros((9, 13, 4), np.uint8)
    rgba[..., :3] = np.random.default_rng(1).integers(0, 256, (9, 13, 3))
    q = E.quantize(rgba, alpha=True)
    assert q["palette"].tolist() == [[0, 0, 0, 0]] and q["n_trans"] == 1 and not q["indices"].any() and q["mse"] == 0.0
    d = E.check_palette_file(q["file"], 13, 9, q["palette"], q["indices"])
    assert d[b"tRNS"] == b"\x00"
    opaque = E.quantize(rgba, alpha=False, file=False)                 # alpha not meaningful: quantised with every alpha byte 255
    assert (opaque["palette"][:, 3] == 255).all() and np.array_equal(opaque["palette"][opaque["indices"]][..., :3], rgba[..., :3])


def test_257_colours_leave_256_entries():
    rgba = E.colour_frame(40, 30, 257, seed=9)
    q = E.quantize(rgba, alpha=False, file=False)
    assert len(q["palette"]) == 256 and q["mse"] > 0.0
    assert int(q["indices"].max()) < 256
    values = set(map(tuple, rgba.reshape(-1, 4)))
    assert sum(tuple(e) in values for e in q["palette"]) >= 254, "all but the values that share an entry are kept as they are"


def test_the_distance_gives_a_transparent_pixels_colour_no_weight():
    L = E.emulator()
    key = lambda r, g, b, a: b | (g << 8) | (r << 16) | (a << 24)  # noqa: E731
    assert L.pq_emu_distance(key(255, 0, 0, 0), key(0, 255, 0, 0)) == 0
    assert L.pq_emu_distance(key(255, 0, 0, 1), key(0, 255, 0, 1)) > 0
    assert L.pq_emu_distance(key(255, 0, 0, 1), key(0, 255, 0, 1)) < L.pq_emu_distance(key(255, 0, 0, 255), key(0, 255, 0, 255)) // 60000
    assert L.pq_emu_distance(key(0, 0, 0, 255), key(255, 255, 255, 255)) == E.DISTANCE_UNIT
    assert L.pq_emu_distance(key(10, 20, 30, 200), key(10, 20, 30, 201)) > 0


# ---- palette quality, against Pillow ------------------------------------------------------------------------------------------------

def test_the_undithered_palette_is_no_worse_than_pillows_median_cut(photo):
    q = E.quantize(photo, alpha=False, dither=False, file=False)
    assert len(q["palette"]) == 256
    mine = rgb_error(q["palette"][q["indices"]], photo)
    pil = Image.fromarray(photo[..., :3]).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB")
    theirs = rgb_error(np.asarray(pil), photo)
    print(f"photo 256x160, 256 colours, undithered: this quantiser {mine:.1f}, Pillow MEDIANCUT {theirs:.1f}")
    assert mine <= theirs


def test_with_real_alpha_the_palette_is_no_worse_than_pillows_octree():
    rgba = P.product_frame(160).copy()
    x = np.mgrid[0:160, 0:160][1]
    rgba[..., 3] = np.where(rgba[..., 3] > 0, np.clip(x * 2, 1, 255), 0).astype(np.uint8)
    q = E.quantize(rgba, alpha=True, dither=False, file=False)
    mine = premultiplied_error(q["palette"][q["indices"]], rgba)
    pil = Image.fromarray(rgba, "RGBA").quantize(256, method=Image.Quantize.FASTOCTREE, dither=Image.Dither.NONE).convert("RGBA")
    theirs = premultiplied_error(np.asarray(pil), rgba)
    print(f"product 160x160 with an alpha ramp, premultiplied: this quantiser {mine:.1f}, Pillow FASTOCTREE {theirs:.1f}")
    assert mine <= theirs
    assert q["n_trans"] > 0 and (q["palette"][:q["n_trans"], 3] < 255).all() and (q["palette"][q["n_trans"]:, 3] == 255).all()


# ---- dithering ------------------------------------------------------------------------------------------------------------------------

def test_dithering_lowers_the_error_of_the_box_means():
    x = np.arange(256)[None, :].repeat(64, 0)
    y = (np.arange(64) * 4)[:, None].repeat(256, 1)
    ramp = np.dstack([x, y, np.zeros_like(x), np.full_like(x, 255)]).astype(np.uint8)
    box = lambda a: a[..., :3].astype(np.float64).reshape(8, 8, 32, 8, 3).mean((1, 3))  # noqa: E731
    err = {}
    for dither in (False, True):
        q = E.quantize(ramp, alpha=False, max_colors=16, dither=dither, file=False)
        assert len(q["palette"]) == 16 and int(q["indices"].max()) < 16
        err[dither] = ((box(q["palette"][q["indices"]]) - box(ramp)) ** 2).sum(-1).mean()
    print(f"8x8 box means, 16 colours: dithered {err[True]:.1f}, plain {err[False]:.1f}, ratio {err[True] / err[False]:.3f}")
    assert err[True] < err[False]


# ---- quality end points -----------------------------------------------------------------------------------------------------------------

def test_quality_end_points_and_monotonicity(photo):
    L = E.emulator()
    bounds = [L.pq_emu_quality_bound(q) for q in range(101)]
    assert bounds[100] == 0 and bounds[0] > E.DISTANCE_UNIT, "100 asks for no error, 0 is unbounded"
    assert all(a >= b for a, b in zip(bounds, bounds[1:])), "a higher quality never allows more error"
    assert E.quantize(photo, alpha=False, minimum_quality=100, file=False)["status"] == E.QUALITY_TOO_LOW
    assert E.quantize(E.colour_frame(40, 30, 256, seed=4), alpha=False, minimum_quality=100, file=False)["status"] == 0
    counts = []
    for quality in (100, 80, 50, 20):
        q = E.quantize(photo, alpha=False, quality=quality, minimum_quality=0, file=False)
        assert q["status"] == 0, "quality 100 with minimum 0 is never too low, nor is any target"
        counts.append(len(q["palette"]))
    print("palette sizes at quality 100, 80, 50, 20:", counts)
    assert counts[0] == 256 and all(a >= b for a, b in zip(counts, counts[1:]))
    # the minimum is clamped to the target (pngquant.rs:55): minimum 100 under quality 50 asks for 50
    assert E.quantize(photo, alpha=False, quality=50, minimum_quality=100, file=False)["status"] == 0


def test_speed_trades_refinement_for_time_and_never_posterises_a_small_palette(photo):
    errs = [E.quantize(photo, alpha=False, speed=s, dither=False, file=False)["mse"] for s in (1, 4, 10)]
    assert errs[0] <= errs[1] <= errs[2]
    rgba = E.colour_frame(40, 30, 256, seed=4)
    for speed in (1, 10, 200):
        q = E.quantize(rgba, alpha=False, speed=speed, file=False)
        assert q["level"] == 0 and np.array_equal(q["palette"][q["indices"]], rgba)


# ---- the file ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, False), (1, 40, False), (40, 1, False), (70, 130, False), (300, 70, True)],
                         ids=lambda s: f"{s[0]}x{s[1]}{'a' if s[2] else ''}")
def test_the_file(shape):
    w, h, alpha = shape
    rgba = E.photo_rgba(w, h, seed=3, alpha=alpha)
    q = E.quantize(rgba, alpha=alpha, stride=4 * w + 8)
    assert q["status"] == 0
    d = E.check_palette_file(q["file"], w, h, q["palette"], q["indices"])
    assert not {b"gAMA", b"sRGB", b"cHRM"} & set(d)
    assert len(zlib.decompress(d[b"IDAT"])) == h * (1 + w)
    assert (b"tRNS" in d) == (alpha and q["n_trans"] > 0)
    pytest.importorskip("torch")
    from imageflow_amd.codecs import libpng_decoder
    info = libpng_decoder.png_info(q["file"])                           # the project's own ifhip_png_info
    assert (info["color_type"], info["bit_depth"], info["width"], info["height"], info["uses_palette"]) == (3, 8, w, h, True)


def test_same_pixels_same_bytes_whatever_the_stride(photo):
    small = photo[:50, :70]
    a = E.quantize(small, alpha=False)
    b = E.quantize(small, alpha=False, stride=4 * 70 + 24)
    assert a["file"] == b["file"]
