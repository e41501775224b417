"""GRAY and LUT-based colour profiles as links (csrc/color_link.cpp) and the link's arithmetic (csrc/color_link_core.hpp) on the
CPU: the emulation against lcms2 2.x through Pillow (the back end the links are pinned to), the nodes against an f64 statement
of the pipeline, the status and reason of every profile that is refused or not sound, a sanitizer run over every prefix and
seeded single-byte changes, and the old planner's answer for all of them.

Measured here against lcms2 2.18 (Pillow 12.2), on the colour grid of 18^3 points {0, 15, ..., 255}^3 -- which holds 0 and 255
on every axis and meets the 33-grid's nodes nowhere else -- maximum difference of a channel and share of points more than 2
apart (2 is the reference's own acceptance between its back ends, cms.rs:91-96):

    family        max   share > 2    profiles
    grey            0   0            every kTRC form, v2 and v4, the reference's gray.icc: all 256 values equal, R = G = B
    mft1-XYZ        1   0            lut8, grids 9 and 17, v2 and v4
    mft2-XYZ        1   0            lut16, grids 2, 3, 9, 17, tables of 2, 256 and 4096 entries, v2 and v4
    mAB-XYZ         1   0            with and without CLUT, matrix, M and A curves; 8- and 16-bit CLUT; unequal grids; v2 and v4
    mAB-Lab         1   0            v4 Lab, 8- and 16-bit CLUT, unequal grids
    mft1-Lab       11   1.8 - 2.9 %  REFUSED: 8 to 25 of the 102 to 170 channel values more than 2 apart sit in cells no node of
    mft2-Lab     7-14   1.1 - 2.6 %  which is clipped (lcms2 samples behind pre-linearisation curves, the link at uniform values)
"""
import io
import os
import subprocess

import numpy as np
import pytest

from tests import color_link_emulation as L
from tests import color_link_profiles as W
from tests import color_profile_emulation as E

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = W.families()
CONVERTED = ("mft1-XYZ", "mft2-XYZ", "mAB-XYZ", "mAB-Lab")
REFUSED = ("mft1-Lab", "mft2-Lab")
MEASURED = {"mft1-XYZ": (1, 0.0), "mft2-XYZ": (1, 0.0), "mAB-XYZ": (1, 0.0), "mAB-Lab": (1, 0.0)}        # family -> (max, share > 2)
AXIS = np.arange(0, 256, 15)
GRID = np.stack(np.meshgrid(AXIS, AXIS, AXIS, indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)
GOLDEN_GRAY = os.path.join(HERE, "golden", "gray.icc")
_LINKS = {}


def link_of(p):
    if p.name not in _LINKS:
        status, link, why = L.link_from_icc(p.icc)
        assert status == L.PLANNED, (p, why)
        _LINKS[p.name] = link
    return _LINKS[p.name]


def gray_profiles():
    out = [("%s-v%d" % (name, v), W.gray_profile(trc, version=v), trc) for name, trc in sorted(W.GRAY_TRCS.items()) for v in (2, 4)]
    with open(GOLDEN_GRAY, "rb") as f:
        out.append(("reference-gray.icc", f.read(), None))
    return out


def lcms(icc, values, mode):
    ImageCms = pytest.importorskip("PIL.ImageCms")
    from PIL import Image
    transform = ImageCms.buildTransform(ImageCms.ImageCmsProfile(io.BytesIO(icc)), ImageCms.createProfile("sRGB"), mode, "RGB", ImageCms.Intent.PERCEPTUAL)
    im = Image.fromarray(values.reshape(1, -1, 3), "RGB") if mode == "RGB" else Image.fromarray(values.reshape(1, -1), "L")
    return np.asarray(ImageCms.applyTransform(im, transform)).reshape(-1, 3).astype(int)


# ---- against lcms2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", CONVERTED)
def test_rgb_links_agree_with_lcms2_as_measured(family):
    """The figures of this module's docstring, asserted: both sides are deterministic integer code."""
    worst, far = 0, 0.0
    for p in FAMILIES[family]:
        ours = L.transform_rgb(GRID, link_of(p)).astype(int)
        theirs = lcms(p.icc, GRID, "RGB")
        d = np.abs(ours - theirs).max(axis=1)
        print(family, p, "max", d.max(), "share > 2", (d > 2).mean())
        worst, far = max(worst, int(d.max())), max(far, float((d > 2).mean()))
        # a transform that does nothing must not pass: lcms2 itself moves most of the grid by more than the bound
        assert (np.abs(theirs - GRID.astype(int)).max(axis=1) > MEASURED[family][0]).mean() > 0.5, p
    assert (worst, far) == MEASURED[family]


@pytest.mark.parametrize("name,icc,trc", gray_profiles(), ids=[g[0] for g in gray_profiles()])
def test_grey_tables_equal_lcms2_on_all_256_values(name, icc, trc):
    status, link, why = L.link_from_icc(icc, True)
    assert status == L.PLANNED and link.kind == L.GRAY, why
    theirs = lcms(icc, np.arange(256, dtype=np.uint8), "L")
    assert (theirs[:, 0] == theirs[:, 1]).all() and (theirs[:, 1] == theirs[:, 2]).all()
    assert np.abs(link.table.astype(int) - theirs[:, 1]).max() == 0
    # a table that does nothing must not pass: but for the identity (the grey axis of linear light) and sRGB's own curve, lcms2
    # moves most of the ramp by more than the bound, 0
    moved = (theirs[:, 1] != np.arange(256)).mean()
    print(name, "moved", moved)
    if name.startswith(("para3", "para4", "reference-gray")):                   # (the reference's gray.icc holds sRGB's curve, 1024 entries)
        assert moved == 0.0
    else:
        assert moved > 0.5


@pytest.mark.parametrize("family", REFUSED)
def test_lut8_and_lut16_with_a_lab_pcs_keep_the_refusal(family):
    for p in FAMILIES[family]:
        status, link, why = L.link_from_icc(p.icc)
        assert status == L.NOT_CONVERTIBLE and link is None and why == "a lut8 or lut16 element with a Lab connection space", (p, why)


# ---- against an f64 statement of the pipeline --------------------------------------------------------------------------------
def srgb_oetf(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.maximum(v, 0) ** (1 / 2.4) - 0.055)


def xyz_from_lab(lab):
    fy = (lab[0] + 16) / 116
    f = np.array([fy + lab[1] / 500, fy, fy - lab[2] / 200])
    return np.where(f > 24 / 116, f ** 3, (108 / 841) * (f - 16 / 116)) * W.D50


def pcs_of_corner(p, corner):
    """XYZ of a corner of the device cube through the profile's own stages, f64: at a corner every table is read at an end"""
    v = np.array(corner, np.float64)
    for stage in p.stages:
        if stage[0] == "curves":
            v = np.array([E.curve_f64(c, v[k]) if isinstance(c, tuple) else np.interp(v[k], np.arange(len(c)) / (len(c) - 1), np.asarray(c) / 65535.0) for k, c in enumerate(stage[1])], np.float64)
        elif stage[0] == "clut":
            assert set(v) <= {0.0, 1.0}
            v = stage[1][tuple(int(t) * (g - 1) for t, g in zip(v, stage[1].shape[:3]))] / 65535.0
        else:
            v = stage[1] @ v + stage[2]
    return v * W.MAX_XYZ if p.pcs == b"XYZ " else xyz_from_lab((v[0] * 100, v[1] * 255 - 128, v[2] * 255 - 128))


def black_point(p):
    if p.version >= 4:
        return np.array([0.00336, 0.0034731, 0.00287])
    y = pcs_of_corner(p, (0, 0, 0))[1]
    lightness = 116 * (np.cbrt(y) if y > (24 / 116) ** 3 else (841 / 108) * y + 16 / 116) - 16
    return xyz_from_lab((min(max(lightness, 0.0), 50.0), 0.0, 0.0))


@pytest.mark.parametrize("p", [p for f in CONVERTED for p in FAMILIES[f]], ids=repr)
def test_the_nodes_at_the_cubes_corners_are_the_f64_pipeline(p):
    """Bound: 1 of 65535 for the final rounding (0.5) and the f32 hand-overs between stages (2^-24 relative each, which sRGB's
    slope at black, 12.92, and the matrix's gain bring to less than a quarter of a unit); and for every tabulated curve stage behind
    the first stage, which lcms2 evaluates in 16 bits: half a unit of the PCS, times the gain of sRGB's matrix on encoded XYZ
    (the largest row, (3.14 + 1.62 + 0.50) * 1.99997 = 10.5), times 12.92 -- 68 units.  (At a corner the first stage is read at
    a table's end, without a rounding.)"""
    rounding_stages = sum(1 for k, stage in enumerate(p.stages) if k > 0 and stage[0] == "curves"
                          and any((not isinstance(c, tuple)) or (c[0] == "curv" and len(c[1]) > 1) for c in stage[1]))
    bound = 1.0 + 68.0 * rounding_stages
    nodes = link_of(p).nodes
    bp = black_point(p)
    for corner in np.ndindex(2, 2, 2):
        xyz = pcs_of_corner(p, corner)
        if bp.any():
            xyz = xyz * (W.D50 / (W.D50 - bp)) - W.D50 * bp / (W.D50 - bp)
        want = np.clip(srgb_oetf(np.linalg.inv(E.lcms_srgb_f64()) @ xyz), 0, 1) * 65535
        got = nodes[tuple(32 * c for c in corner)].astype(float)
        assert np.abs(got - want).max() <= bound, (p, corner, got, want, bound)


@pytest.mark.parametrize("name,trc", sorted(W.GRAY_TRCS.items()))
def test_the_grey_table_is_the_f64_pipeline_resampled_at_33_nodes(name, trc):
    """lcms2 resamples the grey transform at 33 nodes and interpolates linearly; so does the f64 statement.  Bound 1 of 255: the
    final rounding and the 16-bit nodes (half of 1 / 257 of a byte)."""
    status, link, why = L.link_from_icc(W.gray_profile(trc), True)
    assert status == L.PLANNED, why
    at = np.round(np.arange(33) * 65535 / 32) / 65535
    node = np.clip(srgb_oetf(E.curve_f64(trc, at)), 0, 1)                        # Y on the D50 axis is sRGB's grey of the same Y
    want = np.interp(np.arange(256) / 255.0, at, node) * 255
    assert np.abs(link.table.astype(float) - want).max() <= 1.0
    assert link.table[0] == 0 and link.table[255] == 255


# ---- refusals and malformed profiles -------------------------------------------------------------------------------------------
def patched(icc, at, value):
    return icc[:at] + value + icc[at + len(value):]


def a2b0(element, **kw):
    return E.icc_profile((), (), extra=[(b"A2B0", element)], **kw)


MFT2 = FAMILIES["mft2-XYZ"][3]                                                   # grid 2, tables of 256
MAB = FAMILIES["mAB-XYZ"][0]
ELEMENT_AT = 128 + 4 + 12                                                       # the one tag's element follows the table
CASES = [
    ("cmyk", patched(MFT2.icc, 16, b"CMYK"), False, L.NOT_CONVERTIBLE, "a CMYK colour space"),
    ("lab-space", patched(MFT2.icc, 16, b"Lab "), False, L.NOT_CONVERTIBLE, "a colour space other than RGB and GRAY"),
    ("device-link", patched(MFT2.icc, 12, b"link"), False, L.NOT_CONVERTIBLE, "a device-link, abstract or named-colour profile"),
    ("abstract", patched(MFT2.icc, 12, b"abst"), False, L.NOT_CONVERTIBLE, "a device-link, abstract or named-colour profile"),
    ("named-colour", patched(MFT2.icc, 12, b"nmcl"), False, L.NOT_CONVERTIBLE, "a device-link, abstract or named-colour profile"),
    ("d2b0-only", patched(MFT2.icc, 132, b"D2B0"), False, L.NOT_CONVERTIBLE, "a floating-point LUT (D2B0)"),
    ("matrix-trc", E.icc_profile(E.ADOBE_XYZ, [("gamma", 2.2)] * 3), False, L.NOT_CONVERTIBLE, "an RGB profile without A2B0 (a matrix/TRC profile is a plan, not a link)"),
    ("gray-on-colour", W.gray_profile(("gamma", 2.2)), False, L.NOT_CONVERTIBLE, "a GRAY profile on a colour frame"),
    ("gray-lut", W.gray_profile(("gamma", 2.2), extra=[(b"A2B0", b"mft2" + b"\0" * 48)]), True, L.NOT_CONVERTIBLE, "a GRAY profile with a LUT (A2B0)"),
    ("gray-lab", W.gray_profile(("gamma", 2.2), pcs=b"Lab "), True, L.NOT_CONVERTIBLE, "a GRAY profile with a Lab connection space"),
    ("gray-no-ktrc", E.icc_profile((), (), space=b"GRAY"), True, L.MALFORMED, "the GRAY profile lacks its tone curve (kTRC) inside its length"),
    ("gray-bad-curve", W.gray_profile(("raw", b"para" + b"\0" * 4 + b"\0\x09\0\0" + b"\0" * 8)), True, L.MALFORMED, "a para element has a function type above 4"),
    ("odd-pcs", patched(MFT2.icc, 20, b"Luv "), False, L.MALFORMED, "the connection space is neither XYZ nor Lab"),
    ("empty-mab", E.a2b0_only_profile(), False, L.MALFORMED, "the A2B0 element of an RGB profile does not have 3 inputs and 3 outputs"),
    ("four-inputs", patched(MFT2.icc, ELEMENT_AT + 8, b"\x04"), False, L.MALFORMED, "the A2B0 element of an RGB profile does not have 3 inputs and 3 outputs"),
    ("grid-of-1", patched(MFT2.icc, ELEMENT_AT + 10, b"\x01"), False, L.MALFORMED, "the A2B0 element has a grid of fewer than 2 points"),
    ("grid-of-0", patched(MFT2.icc, ELEMENT_AT + 10, b"\x00"), False, L.MALFORMED, "the A2B0 element has a grid of fewer than 2 points"),
    ("grid-past-element", patched(MFT2.icc, ELEMENT_AT + 10, b"\x09"), False, L.MALFORMED, "the tables of a lut8 or lut16 element run past the element"),
    ("entries-past-element", patched(MFT2.icc, ELEMENT_AT + 48, b"\x10\x00"), False, L.MALFORMED, "the tables of a lut8 or lut16 element run past the element"),
    ("one-entry", patched(MFT2.icc, ELEMENT_AT + 50, b"\x00\x01"), False, L.MALFORMED, "a lut16 element claims tables of one entry"),
    ("too-many-entries", patched(MFT2.icc, ELEMENT_AT + 48, b"\x80\x00"), False, L.MALFORMED, "a lut16 element claims tables of more than 32767 entries"),
    ("short-mft2", a2b0(b"mft2" + b"\0" * 20), False, L.MALFORMED, "a lut8 or lut16 element is shorter than its header"),
    ("unknown-element", a2b0(b"mBA " + b"\0" * 60), False, L.MALFORMED, "the A2B0 element is neither mft1, mft2 nor mAB"),
    ("mab-curves-past", patched(MAB.icc, ELEMENT_AT + 12, b"\x00\xFF\xFF\xF0"), False, L.MALFORMED, "a curve of the mAB element lies past the element"),
    ("mab-clut-past", patched(MAB.icc, ELEMENT_AT + 24, b"\x7F\xFF\xFF\xF0"), False, L.MALFORMED, "the CLUT of the mAB element lies past the element"),
    ("mab-matrix-past", patched(MAB.icc, ELEMENT_AT + 16, b"\x7F\xFF\xFF\xF0"), False, L.MALFORMED, "the matrix of the mAB element lies past the element"),
    ("short", MFT2.icc[:100], False, L.MALFORMED, "the profile is shorter than an ICC header and a tag count"),
    ("no-acsp", patched(MFT2.icc, 36, b"nope"), False, L.MALFORMED, "the profile lacks the 'acsp' signature"),
]


@pytest.mark.parametrize("name,icc,gray,status,reason", CASES, ids=[c[0] for c in CASES])
def test_refusals_and_malformed_profiles_name_their_case(name, icc, gray, status, reason):
    got, link, why = L.link_from_icc(icc, gray)
    assert (got, why) == (status, reason) and link is None


def test_mab_clut_cases():
    at = MAB.icc.index(bytes([9, 7, 5]) + b"\0" * 13)                           # the CLUT's grid bytes
    for value, reason in ((b"\x01", "the A2B0 element has a grid of fewer than 2 points"), (b"\xFF", "the CLUT of the mAB element runs past the element")):
        assert L.link_from_icc(patched(MAB.icc, at, value))[::2] == (L.MALFORMED, reason)
    assert L.link_from_icc(patched(MAB.icc, at + 16, b"\x03"))[::2] == (L.MALFORMED, "the CLUT of the mAB element has entries of neither 1 nor 2 bytes")


def test_an_rgb_profile_on_a_grey_frame_stays_on_the_rgb_route():
    status, link, _ = L.link_from_icc(MFT2.icc, True)                            # mozjpeg_decoder.rs:396-403
    assert status == L.PLANNED and link.kind == L.RGB and link.nodes.tobytes() == link_of(MFT2).nodes.tobytes()


def sweep_profiles():
    return [p.icc for f in CONVERTED + REFUSED for p in FAMILIES[f]] + [g[1] for g in gray_profiles()]


def test_prefixes_and_changed_bytes_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (tests/color_link_prefix_sweep.cpp + csrc/color_link.cpp), g++ on the host: every prefix of every test
    profile and seeded single-byte changes, each in a heap block of exactly its size."""
    exe = str(tmp_path / "link_sweep")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            os.path.join(HERE, "color_link_prefix_sweep.cpp"), os.path.join(E.CSRC, "color_link.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    files = []
    for k, icc in enumerate(sweep_profiles()):
        files.append(str(tmp_path / f"profile{k}.icc"))
        with open(files[-1], "wb") as f:
            f.write(icc)
    run = subprocess.run([exe, "16"] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    counts = dict(zip(("planned", "not_convertible", "malformed"), (int(v) for v in run.stdout.split()[1::2])))
    assert counts["planned"] >= len(files) - 5 and counts["not_convertible"] >= 5 and counts["malformed"] > 1000, counts


# ---- the library's own entry points, and the old planner ------------------------------------------------------------------------
def test_the_library_builds_the_emulations_links():
    from imageflow_amd.codecs import color_profile as CP
    for p in (FAMILIES["mft1-XYZ"][0], FAMILIES["mft2-XYZ"][1], FAMILIES["mAB-Lab"][0]):
        link = CP.link_from_icc(p.icc)
        assert link.kind == CP.LINK_RGB and link.nodes().tobytes() == link_of(p).nodes.tobytes()
        link.close()
    gray = CP.link_from_icc(W.gray_profile(W.GRAY_TRCS["dotgain"]), frame_is_gray=True)
    assert gray.kind == CP.LINK_GRAY and gray.nodes().tobytes() == L.link_from_icc(W.gray_profile(W.GRAY_TRCS["dotgain"]), True)[1].table.tobytes()
    status, link, message = CP.try_link_from_icc(E.a2b0_only_profile())
    assert status == CP.MALFORMED and link is None and "malformed" in message and "3 inputs" in message
    status, link, message = CP.try_link_from_icc(FAMILIES["mft2-Lab"][0].icc)
    assert status == CP.NOT_CONVERTIBLE and "not convertible here" in message and "Lab connection space" in message


def test_the_old_planner_still_turns_all_of_them_away():
    for icc in sweep_profiles():
        assert E.plan_from_icc(icc)[0] == E.NOT_CONVERTIBLE
