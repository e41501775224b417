"""The CPU restatements of graphics/rounded_corners.rs (tests/rounded_corners_oracle.py) and flow/nodes/white_balance.rs
(tests/white_balance_oracle.py) against the reference's own stored ids and hand-computed answers, and the shim's
acceptance of the s.roundcorners / a.balancewhite querystring keys.  No GPU needed."""
import numpy as np
import pytest

from imageflow_amd.abi import Context, pack_raw_bgra
from tests import rounded_corners_oracle as R
from tests import white_balance_oracle as WB
from tests.seahash import bitmap_checksum, checksum_id_digits


def color32(hex8):
    r, g, b, a = (int(hex8[i:i + 2], 16) for i in (0, 2, 4, 6))
    return (a << 24) | (r << 16) | (g << 8) | b


def canvas(w, h, hex8):
    c = color32(hex8)
    img = np.zeros((h, w, 4), np.uint8)
    img[:] = [c & 255, (c >> 8) & 255, (c >> 16) & 255, c >> 24]
    return img


# visuals/canvas.rs:240-388 -> canvas.checksums: (w, h, canvas colour, matte, mode, radii in JSON order, id)
REFERENCE_JOBS = {
    "large": (400, 400, "FFFF00FF", "0000FFFF", "pixels", [200.0], "a70bb2e52e"),
    "small": (100, 100, "FFFF00FF", "0000FFFF", "pixels", [5.0], "a89e7d6ea8"),
    "custom_pixels": (100, 99, "ddeecc88", "000000BB", "pixels_custom", [0.0, 1.0, 50.0, 20.0], "154de3acc8"),
    "custom_percent": (100, 99, "2288ffEE", "000000DD", "pixels_custom", [50.0, 5.0, 100.0, 200.0], "dff48806b5"),
    "excessive_radius": (200, 150, "FFFF00FF", "0000FFFF", "pixels", [100.0], "80bf247392"),
    "circle_wide_canvas": (200, 150, "FFFFFFFF", "000000FF", "circle", [0.0], "312b8c473b"),
    "circle_tall_canvas": (150, 200, "FFFFFFFF", "00000000", "circle", [0.0], "31f079eefc"),
}


@pytest.mark.parametrize("name", list(REFERENCE_JOBS))
def test_restatement_reproduces_the_reference_round_corner_ids(name):
    w, h, bg, matte, mode, radii, want = REFERENCE_JOBS[name]
    img = canvas(w, h, bg)
    R.round_image_corners(img, True, mode, (radii * 4)[:4], color32(matte))
    assert checksum_id_digits(img) == want, bitmap_checksum(img)


def test_get_radius_reorders_custom_corners_and_clamps():
    # Custom([tl, tr, bl, br]) from the JSON's tl, tr, br, bl (rounded_corners.rs:15-29); pixels clamp to half the short side
    assert R.get_radius("pixels_custom", [1, 2, 3, 400], 100, 99) == ("custom", [1, 2, np.float32(49.5), 3])
    assert R.get_radius("percentage_custom", [10, 20, 30, 200], 200, 100) == ("custom", [5, 10, 50, 15])
    kind, r = R.get_radius("percentage", [float("nan")] * 4, 10, 10)
    assert kind == "all" and r != r                          # f32::clamp lets NaN through; ceil(NaN) as usize is 0: no rows
    img = canvas(10, 10, "112233FF")
    assert np.array_equal(R.clear_around_rounded_corners(img.copy(), "percentage", [float("nan")] * 4, 0), img)


def test_odd_side_quadrants_touch_the_same_row_and_order_matters():
    """h = 99: a radius of 49.5 reaches row 49 from the top and from the bottom quadrants (the second blends over what the
    first wrote: the kernel applies both in one lane, in this order)."""
    qs = R.plan_quadrants(R.get_radius("pixels", [60] * 4, 99, 99), 99, 99)
    tl, bl = qs[0], qs[2]
    assert tl["y"] + int(np.ceil(tl["r"])) == 50 and tl["y"] + tl["h"] + 0 == 50     # TL arc rows [0, 50)
    assert bl["y"] + bl["h"] - int(np.ceil(bl["r"])) == 49                         # BL arc rows [49, 99): row 49 twice
    a = canvas(99, 99, "80C0FF90")
    R.clear_around_rounded_corners(a, "pixels", [60] * 4, color32("10203080"))
    assert checksum_id_digits(a) != checksum_id_digits(canvas(99, 99, "80C0FF90"))


def test_transparent_matte_over_transparent_pixels_reads_lut_index_zero():
    img = canvas(40, 40, "FFFFFF00")
    R.clear_around_rounded_corners(img, "pixels", [15] * 4, 0)
    assert img[..., 3].max() == 0 and img[..., :3].min() == 0 and img[20, 20, 0] == 255   # 0/0 -> NaN -> index 0 (0)


# ---- white balance -----------------------------------------------------------------------------------------------------
def frame(r, g, b, a=255):
    f = np.zeros((len(r), 1, 4), np.uint8)
    f[:, 0, 0], f[:, 0, 1], f[:, 0, 2], f[:, 0, 3] = b, g, r, a
    return f


def test_default_threshold_is_the_f32_literal():
    assert WB.DEFAULT_THRESHOLD == 0.006000000052154064 != 0.006


def test_threshold_at_or_above_one_is_the_identity():
    rng = np.random.default_rng(1)
    f = rng.integers(0, 256, (30, 20, 4), dtype=np.uint8)
    for t in (1.0, 2.0, float("nan")):
        assert np.array_equal(WB.white_balance(f.copy(), t), f)


def test_one_value_channel_maps_to_255():
    f = frame([7] * 50, np.arange(50) * 5, [200] * 50, a=17)
    out = WB.white_balance(f.copy())
    assert (out[..., 2] == 255).all() and (out[..., 0] == 255).all() and (out[..., 3] == 17).all()
    assert out[0, 0, 1] == 0 and out[-1, 0, 1] == 255                               # the ramp is stretched


def test_bimodal_channel_at_half_maps_to_zero():
    """threshold 0.5 on a channel split evenly between 10 and 200: low = 200 (first bin whose area exceeds half), high =
    10 (searched from the top with the same threshold), high - low wraps: scale ~1.4e-17, everything 0."""
    vals = [10] * 50 + [200] * 50
    lo, hi = WB.area_threshold(WB.histograms(frame(vals, vals, vals))[0], 100, 0.5, 0.5)
    assert (lo, hi) == (200, 10)
    out = WB.white_balance(frame(vals, vals, vals), 0.5)
    assert not out[..., :3].any()


def test_default_threshold_stretches_and_rounds_half_away_from_zero():
    # 5 outliers at each end stay below 0.6 % of 865 pixels, the next bin does not: low 20, high 190, scale 255 / 170 = 1.5
    r = np.concatenate([np.full(5, 0), np.arange(20, 191).repeat(5), np.full(5, 255)])
    f = frame(r, r, r)
    lo, hi = WB.area_threshold(WB.histograms(f)[0], len(r), WB.DEFAULT_THRESHOLD, WB.DEFAULT_THRESHOLD)
    assert (lo, hi) == (20, 190)
    m = WB.byte_mapping(lo, hi)
    assert (m[0], m[20], m[21], m[23], m[190], m[255]) == (0, 0, 2, 5, 255, 255)      # 1.5 -> 2, 4.5 -> 5 (not 4)


def test_negative_threshold_is_the_identity():
    f = frame([3, 9, 250], [0, 0, 1], [255, 255, 255])
    assert np.array_equal(WB.white_balance(f.copy(), -1.0), f)


# ---- the shim takes the keys (they used to answer ActionNotSupported) --------------------------------------------------
@pytest.mark.parametrize("qs", ["s.roundcorners=10", "s.roundcorners= 0, 0,40 ,  50&width=20", "s.roundcorners=10,20",
                                "s.roundcorners=abc", "s.roundcorners=", "S.RoundCorners=5&format=jpg", "a.balancewhite=true",
                                "a.balancewhite=AREA", "a.balancewhite=gimp", "a.balancewhite=simple", "a.balancewhite=maybe",
                                "s.roundcorners=inf,nan,1e1,.5&a.balancewhite=True"])
def test_querystring_keys_are_no_longer_refused(qs):
    src = np.full((8, 12, 4), 200, np.uint8)
    with Context() as c:
        c.add_input_buffer(0, pack_raw_bgra(src.reshape(8, 48), 12, 8, alpha_meaningful=False))
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": [{"command_string": {"kind": "ir4", "value": qs, "decode": 0, "encode": 1}}]}})
        assert "ActionNotSupported" not in r.get("message", ""), r
        assert status in (200, 500), r                     # 500: no GPU on this machine; the keys were parsed


def test_round_image_corners_needs_an_input_and_its_params():
    with Context() as c:
        status, r = c.send_json("v1/execute", {"framewise": {"graph": {"nodes": {"0": {"round_image_corners": {
            "radius": {"pixels": 5}, "background_color": "transparent"}}}, "edges": []}}})
        assert status == 400 and c.error_code() == 7       # GraphInvalid before any parameter is read
