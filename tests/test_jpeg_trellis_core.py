"""The mozjpeg preset's trellis quantisation without a device: tests/jpeg_trellis_emulate.cpp (plain C++ over
csrc/jpeg_trellis_core.hpp, the routines the gfx950 kernels of csrc/jpeg_trellis.hip are built from) DEFINES the coder; here
its plain half is pinned to the oracle (and so to libjpeg-turbo), its search to brute force, and its files -- written by the
host writer, read by Pillow -- to a better rate-distortion curve than the plain quantiser's.  The GPU tests
(tests/test_gpu_jpeg_trellis.py) compare the kernels with the same planes."""
import io
import itertools

import numpy as np
import pytest
from PIL import Image

from oracle import oracle as O
from tests import jpeg_trellis_emu as E
from tests import webp_frames as F

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
          50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def plain(frame, qt, sampling):
    h, w = frame.shape[:2]
    return O.jpeg_forward(frame, w, h, w * 4, sampling[0], sampling[1], qt)


@pytest.mark.parametrize("quality", [1, 75, 100])
@pytest.mark.parametrize("size,sampling", [((1, 1), E.S420), ((17, 9), E.S420), ((33, 31), E.S420), ((257, 17), E.S420), ((33, 31), E.S444)],
                         ids=["1x1", "17x9", "33x31", "257x17", "33x31_444"])
def test_lambda_zero_is_the_plain_coder(size, sampling, quality):
    """byte for byte the oracle's planes (pinned to libjpeg-turbo), dummy blocks included"""
    f = F.photo(*size)
    qt = E.quality_tables(quality)
    r = E.emulate(f, qt, sampling, lambda_scale=0)
    for got, want in zip(r["coef"], plain(f, qt, sampling)):
        assert np.array_equal(got, want)
    assert r["guards"] == (0, 0)


def rate_model():
    return E.reference("photo", 160, 120, 75)["len"][0]


def sparse_block(rng, Q, positions):
    """raw values (natural order) that are not zero at the given zigzag positions only: plain levels 1..3, many of them near a
    rounding threshold, where the search has something to decide"""
    raw = np.zeros(64, np.int16)
    raw[0] = rng.integers(-8000, 8000)
    for k in positions:
        step = 8 * int(Q[ZIGZAG[k]])
        a = int(step * (rng.integers(1, 4) + rng.choice([-0.45, -0.2, 0.0, 0.3, 0.49])))
        raw[ZIGZAG[k]] = min(a, 16383) * rng.choice([-1, 1])
    return raw


TABLES = {"Q1": np.ones(64, np.uint16), "q75": None, "Q255": np.full(64, 255, np.uint16)}
# position 63; a gap of 17 zeros (2 -> 20) and of 33 (21 -> 55); a block that ends before 63 behind a gap of 36
POSITIONS = [(1, 2, 20, 21, 55, 62, 63), (3, 40, 41, 60), (5, 22, 63), (1, 2, 3, 4, 5, 6, 7)]


@pytest.mark.parametrize("lambda_scale", [256, 4096])
@pytest.mark.parametrize("table", list(TABLES))
def test_the_search_is_optimal(table, lambda_scale):
    """every combination of the candidates (0, q, q - 1 where q >= 2) under the core's stand-alone block cost"""
    Q = TABLES[table] if TABLES[table] is not None else E.quality_tables(75)[0]
    lens = rate_model()
    rng = np.random.default_rng(11)
    changed = 0
    for positions in POSITIONS:
        for _ in range(3):
            raw = sparse_block(rng, Q, positions)
            level, cost, guards = E.search_block(raw, Q, lens, lambda_scale)
            assert guards == (0, 0)
            assert cost == E.block_cost(raw, Q, level, lens, lambda_scale)
            q = [(abs(int(raw[ZIGZAG[k]])) + 4 * int(Q[ZIGZAG[k]])) // (8 * int(Q[ZIGZAG[k]])) for k in positions]
            assert all(v >= 1 for v in q)
            best = None
            for combo in itertools.product(*[[0, v] + ([v - 1] if v >= 2 else []) for v in q]):
                cand = np.zeros(64, np.int16)
                for k, v in zip(positions, combo):
                    cand[ZIGZAG[k]] = v
                c = E.block_cost(raw, Q, cand, lens, lambda_scale)
                best = c if best is None or c < best else best
            assert cost == best, (table, positions, raw.tolist())
            changed += int(any(abs(int(level[ZIGZAG[k]])) != v for k, v in zip(positions, q)))
    # (with the heavier factor the search decides something; at Q = 255 the blocks' energy makes the factor too small for that)
    if lambda_scale == 4096 and table != "Q255":
        assert changed > 0


def blocks_of(r, w, h, sampling):
    for c, (rbw, rbh) in enumerate(E.real_blocks(w, h, sampling)):
        for by in range(rbh):
            for bx in range(rbw):
                yield c, by, bx


@pytest.mark.parametrize("kind,size", [("photo", (160, 120)), ("noise", (64, 48))])
def test_never_worse_than_plain_under_the_stages_own_model(kind, size):
    """a condition, not a measurement: the plain levels are in the search space"""
    w, h = size
    qt = E.quality_tables(75)
    r = E.reference(kind, w, h, 75)
    p = plain(E.frame(kind, w, h), qt, E.S420)
    better = 0
    for c, by, bx in blocks_of(r, w, h, E.S420):
        lens = r["len"][1 if c else 0]
        jt = E.block_cost(r["raw"][c][by, bx], qt[c], r["coef"][c][by, bx], lens)
        jp = E.block_cost(r["raw"][c][by, bx], qt[c], p[c][by, bx], lens)
        assert jt <= jp, (c, by, bx)
        better += int(jt < jp)
    assert better > 0 and r["guards"] == (0, 0)


@pytest.mark.parametrize("kind,size", [("photo", (160, 120)), ("noise", (64, 48)), ("photo", (17, 9)), ("flat", (33, 31))])
def test_candidate_property(kind, size):
    """every level is zero or has the plain level's sign and at most its magnitude; DC and dummy blocks are the plain coder's"""
    w, h = size
    qt = E.quality_tables(75)
    r = E.reference(kind, w, h, 75)
    p = plain(E.frame(kind, w, h), qt, E.S420)
    for c in range(3):
        t, q = r["coef"][c].astype(np.int32), p[c].astype(np.int32)
        assert np.array_equal(t[..., 0], q[..., 0])
        assert np.all((t == 0) | ((np.sign(t) == np.sign(q)) & (np.abs(t) <= np.abs(q))))
        assert np.all((t == q) | (t == 0) | ((np.abs(q) >= 2) & (np.abs(t) == np.abs(q) - 1)))
        rbw, rbh = E.real_blocks(w, h, E.S420)[c]
        dummy = np.ones(t.shape[:2], bool)
        dummy[:rbh, :rbw] = False
        assert np.array_equal(t[dummy], q[dummy])
        assert not r["raw"][c][dummy].any()


def test_extremes():
    """a frame of one colour: EOB-only AC everywhere; noise at quality 100 and at quality 1 runs; no overflow guard trips"""
    r = E.emulate(F.one_colour(40, 24), E.quality_tables(75))
    assert r["guards"] == (0, 0) and not any(c[..., 1:].any() for c in r["coef"])
    for quality in (100, 1):
        r = E.reference("noise", 64, 48, quality)
        assert r["guards"] == (0, 0)
    assert any(c[..., 1:].any() for c in E.reference("noise", 64, 48, 100)["coef"])
    # the all-ones table on the largest AC values 8-bit samples can give (|raw| < 2^14): the costs stay far below 2^61
    rng = np.random.default_rng(3)
    raw = (rng.integers(8000, 16384, 64) * rng.choice([-1, 1], 64)).astype(np.int16)
    for Q in (np.ones(64, np.uint16), np.full(64, 255, np.uint16)):
        level, cost, guards = E.search_block(raw, Q, rate_model(), 65535)
        assert guards[1] == 0 and 0 <= cost < 1 << 59


def test_rate_table_gives_every_legal_symbol_a_length():
    lens = E.rate_table(np.zeros(256, np.uint32))
    legal = [s for s in range(256) if s in (0, 0xF0) or 1 <= (s & 15) <= 10]
    assert len(legal) == 162
    assert all(1 <= lens[s] <= 16 for s in legal) and not any(lens[s] for s in range(256) if s not in legal)
    assert sum(2.0 ** -int(lens[s]) for s in legal) < 1.0          # (a prefix code with libjpeg's reserved code point)


# ---- rate-distortion, through Pillow (libjpeg-turbo) ---------------------------------------------------------------------------

RD_W, RD_H = 256, 192


def psnr(data, rgb):
    im = Image.open(io.BytesIO(data))
    assert im.size == (RD_W, RD_H) and im.format == "JPEG"
    return 10 * np.log10(255.0 ** 2 / np.mean((np.asarray(im.convert("RGB")).astype(np.float64) - rgb) ** 2))


@pytest.fixture(scope="module")
def plain_curve():
    """the libjpeg_turbo preset's own files (progressive, optimised tables) at every integer quality"""
    from imageflow_amd.codecs.mozjpeg import write_jpeg
    f = E.frame("photo", RD_W, RD_H)
    return {q: write_jpeg(plain(f, E.quality_tables(q), E.S420), RD_W, RD_H, *E.S420, q, progressive=True, optimize_coding=True)
            for q in range(1, 101)}


@pytest.mark.parametrize("quality", [50, 75, 90])
def test_trellis_files_dominate_the_plain_curve(plain_curve, quality):
    """With q' the largest quality whose plain file is no larger than the trellis file at q: q' < q (the trellis file is
    smaller than the plain file at q) and the trellis file's PSNR is at least the plain file's at q'.
    Measured with the shipped (HVS-PSNR, 14.75 / 16.5) tuning: q50 4409 bytes 31.695 dB against q' = 48, 4369 bytes 31.616 dB;
    q75 6082 bytes 32.982 dB against q' = 73, 5967 bytes 32.894 dB; q90 9844 bytes 35.046 dB against q' = 89, 9428 bytes 34.878 dB."""
    from imageflow_amd.codecs.mozjpeg import write_jpeg
    f = E.frame("photo", RD_W, RD_H)
    rgb = f[..., 2::-1].astype(np.float64)
    r = E.reference("photo", RD_W, RD_H, quality)
    data = write_jpeg(r["coef"], RD_W, RD_H, *E.S420, quality, progressive=True, optimize_coding=True)
    assert data[:2] == b"\xff\xd8" and b"\xff\xc2" in data[:700]
    fits = [q for q, d in plain_curve.items() if len(d) <= len(data)]
    assert fits, "the trellis file is smaller than every plain file"
    q_prime = max(fits)
    got, want = psnr(data, rgb), psnr(plain_curve[q_prime], rgb)
    print(f"q {quality}: trellis {len(data)} bytes {got:.3f} dB; plain at q {len(plain_curve[quality])} bytes; "
          f"q' {q_prime}: {len(plain_curve[q_prime])} bytes {want:.3f} dB")
    assert q_prime < quality
    assert got >= want
