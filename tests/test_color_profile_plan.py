"""Colour profiles as conversion plans (csrc/color_profile.cpp) and the conversion's arithmetic (csrc/color_profile_core.hpp)
on the CPU: tables and matrix against an f64 statement, the status of profiles that are not converted or not sound, a
sanitizer run over every prefix, and the emulation against lcms2 (through Pillow), the back end the plans are pinned to."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import color_profile_emulation as E
from tests.test_jpeg_headers import P3_XYZ, SRGB_XYZ, make_icc

HERE = os.path.dirname(os.path.abspath(__file__))
SRGB_PARA = ("para", 3, [2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045])
_XS1024 = [k / 1023 for k in range(1024)]
CURV1024 = ("curv", [int(round((x / 12.92 if x <= 0.04045 else ((x + 0.055) / 1.055) ** 2.4) * 65535)) for x in _XS1024])
MAKE_ICC_TRC = {"para": SRGB_PARA, "curv1024": CURV1024, "gamma22": ("gamma", int(2.2 * 256) / 256)}
COLOURANTS = {"srgb": SRGB_XYZ, "p3": P3_XYZ, "adobe": E.ADOBE_XYZ}
# the five function types of a para element.  Types 2 and 4 lift black by 3 / 65536 only (type 4 stays continuous at d: e = f):
# a curve that lifts it by more than 1e-4 is not converted, because lcms2 would compensate the black point
LIFT = 3 / 65536
PARA_TYPES = [("para", 0, [2.2]), ("para", 1, [2.0, 1.1, -0.1]), ("para", 2, [2.0, 1.1, -0.1, LIFT]), SRGB_PARA,
              ("para", 4, [2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045, LIFT, LIFT])]
THREE_TRCS = [("gamma", 563 / 256), SRGB_PARA, ("curv", [int(round((k / 16) ** 1.8 * 65535)) for k in range(17)])]
# gAMA + cHRM of a wide-gamut source: gamma 0.5, D65, Adobe RGB's primaries
GAMMA_CASE = (0.5, (0.3127, 0.3290, 0.64, 0.33, 0.21, 0.71, 0.15, 0.06))
SRGB_CHRM = E.SRGB_CHRM


def native():
    from imageflow_amd.codecs import color_profile as CP
    return CP


def native_plan(icc):
    status, plan, message = native().try_plan_from_icc(icc)
    assert status == E.PLANNED, message
    return plan.tables(), plan.matrix3()


def check_plan(icc, xyz, specs):
    tables, matrix = native_plan(icc)
    x = np.arange(256) / 255.0
    for c in range(3):
        want = E.curve_f64(specs[c], x).astype(np.float32)
        assert E.ulps(tables[c], want).max() <= 1.0, (c, specs[c][:2])
    assert E.ulps(matrix, E.matrix_f64(xyz).astype(np.float32)).max() <= 1.0
    status, plan, _ = E.plan_from_icc(icc)                                       # the emulation runs on the very same plan
    assert status == E.PLANNED and plan.tobytes() == np.concatenate([tables.ravel(), matrix.ravel()]).tobytes()


@pytest.mark.parametrize("trc", sorted(MAKE_ICC_TRC))
@pytest.mark.parametrize("name", sorted(COLOURANTS))
def test_matrix_trc_profiles_give_the_f64_tables_and_matrix_to_one_ulp(name, trc):
    check_plan(make_icc(xyz=COLOURANTS[name], trc=trc), COLOURANTS[name], [MAKE_ICC_TRC[trc]] * 3)


def test_each_channel_takes_its_own_tone_curve():
    check_plan(E.icc_profile(P3_XYZ, THREE_TRCS, version=2), P3_XYZ, THREE_TRCS)
    tables, _ = native_plan(E.icc_profile(P3_XYZ, THREE_TRCS))
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])


@pytest.mark.parametrize("ftype", range(5))
def test_para_function_types(ftype):
    spec = PARA_TYPES[ftype]
    check_plan(E.icc_profile(E.ADOBE_XYZ, [spec] * 3, version=2), E.ADOBE_XYZ, [spec] * 3)


def test_curv_without_entries_is_the_identity_curve():
    tables, _ = native_plan(E.icc_profile(P3_XYZ, [("curv", [])] * 3))
    assert np.array_equal(tables[0], (np.arange(256) / 255.0).astype(np.float32))


def status_of(icc):
    status, plan, message = native().try_plan_from_icc(icc)
    assert (plan is None) == (status != E.PLANNED)
    assert E.plan_from_icc(icc)[0] == status
    return status, message


@pytest.mark.parametrize("icc, word", [
    (make_icc(space=b"GRAY", trc="gamma22"), "GRAY"),
    (make_icc(space=b"CMYK"), "CMYK"),
    (make_icc(xyz=P3_XYZ, pcs=b"Lab "), "Lab"),
    (E.a2b0_only_profile(), "LUT"),
    (E.icc_profile(P3_XYZ, [SRGB_PARA] * 3, extra=[(b"A2B0", b"mft2" + b"\0" * 48)]), "LUT"),      # lcms2 reads the LUT when there is one
    (E.icc_profile(E.ADOBE_XYZ, [("para", 2, [2.0, 0.9, 0.05, 0.05])] * 3, version=2), "black"),      # lcms2 would compensate the black point
], ids=["gray", "cmyk", "lab", "a2b0-only", "a2b0-and-matrix", "lifted-black"])
def test_profiles_that_are_not_converted_say_which_case(icc, word):
    status, message = status_of(icc)
    assert status == E.NOT_CONVERTIBLE and word in message and "not convertible here" in message, message


def _with_tag_field(icc, sig, field, value):
    at = icc.index(sig, 128)
    return icc[:at + 4 + 4 * field] + struct.pack(">I", value) + icc[at + 8 + 4 * field:]


P3 = make_icc(xyz=P3_XYZ)
MALFORMED = {
    "empty": b"",
    "header-only": P3[:128],
    "truncated-in-the-table": P3[:150],
    "truncated-in-a-colourant": P3[:P3.index(b"XYZ ", 132) + 10],
    "no-acsp": P3[:36] + b"xxxx" + P3[40:],
    "tag-offset-beyond-the-length": _with_tag_field(P3, b"gXYZ", 0, len(P3) + 64),
    "tag-offset-wraps": _with_tag_field(P3, b"rTRC", 0, 0xFFFFFFF8),
    "tag-size-beyond-the-length": _with_tag_field(P3, b"bTRC", 1, 0x7FFFFFFF),
    "zero-length-curv": _with_tag_field(P3, b"rTRC", 1, 0),
    "absurd-entry-count": E.icc_profile(P3_XYZ, [("raw", b"curv" + b"\0" * 4 + struct.pack(">I", 0x40000000) + b"\0" * 8)] * 3),
    "entries-beyond-the-element": E.icc_profile(P3_XYZ, [("raw", b"curv" + b"\0" * 4 + struct.pack(">I", 300) + b"\0" * 8)] * 3),
    "para-type-5": E.icc_profile(P3_XYZ, [("para", 5, [2.2])] * 3),
    "para-short": E.icc_profile(P3_XYZ, [("para", 4, [2.2, 1.0])] * 3),
    "no-colourants": E.icc_profile(P3_XYZ, [SRGB_PARA] * 3, drop=(b"gXYZ",)),
    "too-many-tags": P3[:128] + struct.pack(">I", 101) + P3[132:],
    "unknown-pcs": make_icc(xyz=P3_XYZ, pcs=b"Luv "),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_profiles(case):
    status, message = status_of(MALFORMED[case])
    assert status == E.MALFORMED and "malformed" in message and message.startswith("ColorProfileError"), message


def test_status_texts():
    CP = native()
    assert [CP.status_text(s) for s in (0, 1, 2)] == ["planned", "not convertible here", "malformed"]


def sweep_profiles():
    return [make_icc(xyz=P3_XYZ), make_icc(xyz=E.ADOBE_XYZ, trc="curv1024"), make_icc(trc="gamma22"), E.icc_profile(P3_XYZ, THREE_TRCS, version=2),
            E.icc_profile(E.ADOBE_XYZ, [PARA_TYPES[4]] * 3, version=2), E.a2b0_only_profile()]


def test_every_prefix_of_a_valid_profile_has_a_status():
    for icc in sweep_profiles():
        whole = status_of(icc)[0]
        seen = {native().try_plan_from_icc(icc[:n])[0] for n in range(len(icc))}
        assert seen <= {E.MALFORMED, whole}, seen           # (a profile's own size field is clamped to the bytes there are)
        assert native().try_plan_from_icc(icc[:131])[0] == E.MALFORMED


def test_prefix_sweep_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program (tests/color_profile_prefix_sweep.cpp + csrc/color_profile.cpp), g++ on the host: every prefix and
    hostile header, table and element words, each in a heap block of exactly its size."""
    exe = str(tmp_path / "prefix_sweep")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            os.path.join(HERE, "color_profile_prefix_sweep.cpp"), os.path.join(E.CSRC, "color_profile.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    files = []
    for k, icc in enumerate(sweep_profiles()):
        files.append(str(tmp_path / f"profile{k}.icc"))
        with open(files[-1], "wb") as f:
            f.write(icc)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    counts = dict(zip(("planned", "not_convertible", "malformed"), (int(v) for v in run.stdout.split()[1::2])))
    assert counts["planned"] >= 5 and counts["not_convertible"] >= 1 and counts["malformed"] > sum(len(p) for p in sweep_profiles()) // 2, counts


# ---- gAMA + cHRM ---------------------------------------------------------------------------------------------------------
def test_srgbs_own_gamma_and_primaries_give_the_identity():
    CP = native()
    for gamma in (0.45455, 1 / 2.4):                        # (0.45455 is "neutral": SourceProfile::Srgb, the plan that changes nothing)
        status, plan, message = CP.try_plan_from_gamma_primaries(gamma, SRGB_CHRM)
        assert status == E.PLANNED, message
        assert np.abs(plan.matrix3() - np.eye(3)).max() < 1e-4
    _, plan, _ = CP.try_plan_from_gamma_primaries(1 / 2.4, SRGB_CHRM)
    want = ((np.arange(256) / 255.0) ** 2.4).astype(np.float32)
    assert E.ulps(plan.tables()[1], want).max() <= 1.0


@pytest.mark.parametrize("white", [(0.3127, 0.3290), (0.3457, 0.3585), (0.32, 0.36)], ids=["d65", "d50", "greenish"])
def test_gamma_and_primaries_against_an_f64_bradford_statement(white):
    gamma, xy = GAMMA_CASE[0], white + GAMMA_CASE[1][2:]
    status, plan, message = native().try_plan_from_gamma_primaries(gamma, xy)
    assert status == E.PLANNED, message
    want = np.linalg.inv(E.lcms_srgb_f64()) @ E.bradford_adapted_f64(xy)
    assert E.ulps(plan.matrix3(), want.astype(np.float32)).max() <= 1.0
    curve = ((np.arange(256) / 255.0) ** (1 / gamma)).astype(np.float32)
    assert all(E.ulps(plan.tables()[c], curve).max() <= 1.0 for c in range(3))
    assert E.plan_from_gamma_primaries(gamma, xy)[1].tobytes() == np.concatenate([plan.tables().ravel(), plan.matrix3().ravel()]).tobytes()


@pytest.mark.parametrize("gamma, xy", [(0.0, SRGB_CHRM), (-1.0, SRGB_CHRM), (float("nan"), SRGB_CHRM), (float("inf"), SRGB_CHRM),
                                       (0.5, (0.3127, 0.0) + SRGB_CHRM[2:]), (0.5, SRGB_CHRM[:3] + (0.0,) + SRGB_CHRM[4:]),
                                       (0.5, SRGB_CHRM[:6] + (float("nan"), 0.06))])
def test_degenerate_gamma_or_primaries_count_as_srgb(gamma, xy):
    """source_profile.rs:225-236: such a file is SourceProfile::Srgb -- the plan changes no byte."""
    status, plan, _ = native().try_plan_from_gamma_primaries(gamma, xy)
    assert status == E.PLANNED and np.array_equal(plan.matrix3(), np.eye(3, dtype=np.float32))
    rows = np.repeat(np.arange(256, dtype=np.uint8), 4).reshape(1, -1)
    assert np.array_equal(E.transform(rows, 256, E.plan_from_gamma_primaries(gamma, xy)[1]), rows)


def test_primaries_on_one_line_are_malformed():
    status, _, message = native().try_plan_from_gamma_primaries(0.5, (0.3127, 0.3290, 0.6, 0.3, 0.4, 0.2, 0.2, 0.1))
    assert status == E.MALFORMED and "one line" in message


# ---- the emulation against lcms2 -------------------------------------------------------------------------------------------
def grid():
    g = np.arange(0, 256, 3, dtype=np.uint8)
    r, gg, b = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([r.ravel(), gg.ravel(), b.ravel()], 1)                 # 86^3 pixels, R G B


def lcms_cases():
    cases = [(f"{name}-{trc}", make_icc(xyz=COLOURANTS[name], trc=trc), None) for name in sorted(COLOURANTS) for trc in sorted(MAKE_ICC_TRC)]
    cases.append(("three-trcs", E.icc_profile(P3_XYZ, THREE_TRCS, version=2), None))
    cases += [(f"para{t}", E.icc_profile(E.ADOBE_XYZ, [PARA_TYPES[t]] * 3, version=2), None) for t in range(5)]
    # gAMA + cHRM: lcms2 sees a profile written from the same adapted colourants and a para type-0 curve of exponent 1 / gamma
    gamma, xy = GAMMA_CASE
    adapted = E.bradford_adapted_f64(xy)
    cases.append(("gama-chrm", E.icc_profile([tuple(adapted[:, k]) for k in range(3)], [("para", 0, [1 / gamma])] * 3), (gamma, xy)))
    return cases


# the least share of the grid that lcms2 itself moves by more than 2: a transform that does nothing cannot pass
MOVED = {"p3-para": 0.5, "p3-curv1024": 0.5, "p3-gamma22": 0.5, "adobe-para": 0.5, "adobe-curv1024": 0.5, "adobe-gamma22": 0.5, "srgb-gamma22": 0.5}


@pytest.mark.parametrize("case", lcms_cases(), ids=[c[0] for c in lcms_cases()])
def test_emulation_agrees_with_lcms2_to_2(case):
    """Bound 2: the reference's own figure for the agreement of its two CMS back ends on RGB profiles (codecs/cms.rs:92-96).
    Measured with lcms2 2.18: a maximum of 1 on every case, 1.7 - 7.0 % of the pixels differing at all, none on sRGB's own
    profile."""
    features = pytest.importorskip("PIL.features")
    if not features.check("littlecms2"):
        pytest.skip("Pillow without littlecms2")
    from PIL import Image, ImageCms
    name, icc, gamma_xy = case
    px = grid()
    n, w = len(px), 512
    h = -(-n // w)
    buf = np.zeros((h * w, 3), np.uint8)
    buf[:n] = px
    t = ImageCms.buildTransform(ImageCms.ImageCmsProfile(io.BytesIO(icc)), ImageCms.createProfile("sRGB"), "RGB", "RGB", renderingIntent=ImageCms.Intent.PERCEPTUAL)
    ref = np.asarray(ImageCms.applyTransform(Image.fromarray(buf.reshape(h, w, 3), "RGB"), t)).reshape(-1, 3)[:n].astype(int)
    status, plan, why = E.plan_from_gamma_primaries(*gamma_xy) if gamma_xy else E.plan_from_icc(icc)
    assert status == E.PLANNED, why
    bgra = np.concatenate([px[:, ::-1], np.full((n, 1), 0x5A, np.uint8)], 1).reshape(1, -1)
    out = E.transform(bgra, n, plan).reshape(n, 4)
    assert np.all(out[:, 3] == 0x5A)
    mine = out[:, 2::-1].astype(int)
    d = np.abs(mine - ref)
    moved = (np.abs(ref - px.astype(int)).max(1) > 2).mean()
    print(f"{name}: max {d.max()}, share of pixels that differ {(d.max(1) > 0).mean():.4f}, share lcms2 moves by more than 2 {moved:.2f}")
    assert d.max() <= 2
    if name in MOVED:
        assert moved >= MOVED[name], moved
