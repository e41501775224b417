"""The device entropy coder's optimised-table and progressive forms without a device (csrc/jpeg_encode_progressive_core.hpp:
the block routines, the end-of-band run walk, jpeg_gen_optimal_table in lane-sized pieces, the placement of scans and
segments that the gfx950 kernels of csrc/jpeg_encode_progressive.hip are built from).  tests/enc_progressive_emulate.cpp
runs the passes lane by lane on the CPU; the file must equal what libjpeg-turbo wrote (through Pillow; the coefficients come
back through the oracle's entropy decoder from the baseline twin of the file).  The GPU tests
(tests/test_gpu_jpeg_device_coder_progressive.py) compare the kernels with the same files."""
import ctypes as C
import io
import os
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image, ImageFile

ImageFile.MAXBLOCK = 1 << 24

from imageflow_amd import _native
from oracle import oracle as O
from tests.test_jpeg_device_coder import SAMPLINGS, photo, tables_and_header

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = {1: {"optimize": True}, 2: {"progressive": True}, 3: {"optimize": True, "progressive": True}}
_EMU = {}


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="enc_progressive_emulate_")
        so = os.path.join(d, "libenc_progressive_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas",
                        os.path.join(HERE, "enc_progressive_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.enc_progressive_emulate.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 5 + [
            C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.c_void_p]
        _EMU["lib"] = lib
    return _EMU["lib"]


def emulate(j, quality, flags, capacity=None):
    """j: a jpeg_read_coefficients dict.  Returns (file bytes or None, status, violations, (runs cut at 0x7FFF, runs cut by bits))."""
    lib = emulator()
    ncomp = j["ncomp"]
    hs, vs = (list(j["hs"]) + [1, 1, 1])[:3], (list(j["vs"]) + [1, 1, 1])[:3]
    _, header = tables_and_header(ncomp, hs, vs, j["width"], j["height"], quality)
    bw, bh = np.array((list(j["bw"]) + [0, 0, 0])[:3], np.uint32), np.array((list(j["bh"]) + [0, 0, 0])[:3], np.uint32)
    h, v = np.array(hs, np.uint8), np.array(vs, np.uint8)
    planes = [np.ascontiguousarray(j["coef"][c], np.int16) if c < ncomp else None for c in range(3)]
    cap = capacity if capacity is not None else 8192 + 8 * sum(p.size for p in planes if p is not None)
    out, n, st, viol, cuts = np.zeros(cap, np.uint8), C.c_size_t(0), C.c_uint32(0), C.c_int(0), np.zeros(2, np.int32)
    rc = lib.enc_progressive_emulate(*[p.ctypes.data if p is not None else None for p in planes], j["width"], j["height"], ncomp,
                                     h.ctypes.data, v.ctypes.data, bw.ctypes.data, bh.ctypes.data, header.ctypes.data, header.size, flags,
                                     out.ctypes.data, out.size, C.byref(n), C.byref(st), C.byref(viol), cuts.ctypes.data)
    assert rc == 0
    return (out[:n.value].tobytes() if n.value else None), st.value, viol.value, (int(cuts[0]), int(cuts[1]))


def save(img, quality, sampling=None, **kw):
    buf = io.BytesIO()
    if sampling is not None:
        kw["subsampling"] = sampling
    Image.fromarray(img).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def twin(img, quality, sampling=None):
    """The coefficients libjpeg-turbo codes for these pixels: read back from the baseline file."""
    return O.jpeg_read_coefficients(save(img, quality, sampling, optimize=False))


def flat_gray():
    return np.full((1456, 1456), 131, np.uint8)


def noise_gray(side=512, seed=1):
    return (np.random.default_rng(seed).integers(0, 2, (side, side)) * 255).astype(np.uint8)


def synthetic_planes(ncomp, seed=5):
    """64 luma blocks whose AC coefficients all have magnitude 4..7 and a random sign: 63 correction bits per block in every
    refinement scan, a cut every 15 blocks.  No image produces them; the yardstick is the host writer."""
    rng = np.random.default_rng(seed)
    if ncomp == 1:
        shapes, size, hs, vs = [(8, 8)], (64, 64), [1, 1, 1], [1, 1, 1]
    else:
        shapes, size, hs, vs = [(8, 8), (4, 4), (4, 4)], (64, 64), [2, 1, 1], [2, 1, 1]
    coef = []
    for bh, bw in shapes:
        c = (rng.integers(4, 8, (bh, bw, 64)) * rng.choice([-1, 1], (bh, bw, 64))).astype(np.int16)
        c[:, :, 0] = rng.integers(-500, 500, (bh, bw))
        coef.append(c)
    return {"ncomp": ncomp, "width": size[0], "height": size[1], "hs": hs[:ncomp] if ncomp == 3 else [1], "vs": vs[:ncomp] if ncomp == 3 else [1],
            "bw": [s[1] for s in shapes], "bh": [s[0] for s in shapes], "coef": coef}


def host_writer(j, quality, progressive, optimize_coding=False):
    from imageflow_amd.codecs.mozjpeg import write_jpeg
    return write_jpeg([np.ascontiguousarray(c) for c in j["coef"][:j["ncomp"]]], j["width"], j["height"], list(j["hs"])[:j["ncomp"]],
                      list(j["vs"])[:j["ncomp"]], quality, progressive=progressive, optimize_coding=optimize_coding)


@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("sampling", ["4:2:0", "4:2:2", "4:4:4"])
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (17, 9), (64, 48), (203, 131)])
@pytest.mark.parametrize("quality", [5, 75, 100])
def test_emulated_passes_write_libjpeg_turbos_file(flags, sampling, size, quality):
    w, h = size
    img = photo(w, h, w * 31 + h + quality)
    j = twin(img, quality, sampling)
    assert (j["hs"], j["vs"]) == SAMPLINGS[sampling]
    out, status, violations, _ = emulate(j, quality, flags)
    assert status == 0 and violations == 0
    assert out == save(img, quality, sampling, **FLAGS[flags])


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_grayscale(flags):
    img = photo(150, 97, 3)[:, :, 0]
    j = twin(img, 80)
    assert j["ncomp"] == 1
    out, status, violations, _ = emulate(j, 80, flags)
    assert (status, violations) == (0, 0) and out == save(img, 80, **FLAGS[flags])


def test_flat_frame_cuts_a_run_at_0x7fff_blocks():
    """1456 x 1456 gray, flat: 33 124 blocks and one end-of-band run in every AC scan, cut once at 32 767 blocks (4 AC scans:
    the emulator counts 4 cuts) -- and walked by ONE wave across the scan's 17 chunks."""
    img = flat_gray()
    j = twin(img, 75)
    out, status, violations, cuts = emulate(j, 75, 2)
    assert (status, violations) == (0, 0) and out == save(img, 75, progressive=True)
    assert cuts[0] > 0, cuts


def test_noise_at_q100_cuts_runs_by_the_correction_bit_bound():
    """512 x 512 gray of 0 / 255 pixels at quality 100: runs of blocks without a new coefficient whose buffered correction
    bits pass 937.  With libjpeg-turbo's own coefficients (seed 1) the emulator counts 19 such cuts at 512 x 512 and 3 at
    256 x 256, all in the last refinement scan; the counter is asserted, not assumed."""
    img = noise_gray()
    j = twin(img, 100)
    data = save(img, 100, progressive=True)
    out, status, violations, cuts = emulate(j, 100, 2)
    assert (status, violations) == (0, 0) and out == data
    assert cuts[1] > 0, cuts


@pytest.mark.parametrize("ncomp", [1, 3])
def test_synthetic_planes_cut_every_15_blocks(ncomp):
    j = synthetic_planes(ncomp)
    want = host_writer(j, 90, progressive=True)
    out, status, violations, cuts = emulate(j, 90, 2)
    assert (status, violations) == (0, 0) and out == want
    # 15 blocks of 63 bits pass 937: luma has two AC refinement scans of 64 blocks, each chroma plane one of 16
    assert cuts == (0, 2 * (64 // 15) + (2 * (16 // 15) if ncomp == 3 else 0)), cuts
    Image.open(io.BytesIO(out)).load()
    from tests.test_jpeg_progressive import read_host
    got = read_host(out)
    for c in range(ncomp):
        assert np.array_equal(got["coef"][c], j["coef"][c]), c


def test_max_file_bytes_for_bounds_the_noise_file():
    img = noise_gray()
    j = twin(img, 100)
    data = save(img, 100, progressive=True)
    L = _native.lib()
    L.ifhip_jpeg_debug_enc_max_file_bytes_for.restype = C.c_size_t
    L.ifhip_jpeg_debug_enc_max_file_bytes_for.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                          C.c_size_t]
    one = np.ones(3, np.uint8)
    bw, bh = np.array([j["bw"][0], 0, 0], np.uint32), np.array([j["bh"][0], 0, 0], np.uint32)

    def bound(flags, scan_capacity=0):
        return L.ifhip_jpeg_debug_enc_max_file_bytes_for(512, 512, 1, one.ctypes.data, one.ctypes.data, bw.ctypes.data, bh.ctypes.data, flags,
                                                         scan_capacity)
    for flags in (1, 2, 3):
        assert len(save(img, 100, **FLAGS[flags])) <= bound(flags)
    assert len(data) <= bound(2)
    # flags 0: exactly the baseline stage's bound -- marker segments + every byte of the worst stream (whole chunks) stuffed + EOI
    worst = (64 * 64 * (16 + 11 + 63 * 26) + 7) // 8
    assert bound(0) == 1024 + 2 * ((worst + 4095) // 4096 * 4096) + 2


def test_out_of_range_coefficient_drops_the_file():
    j = twin(photo(40, 40, 5), 90, "4:4:4")
    j["coef"][1] = j["coef"][1].copy()
    j["coef"][1].reshape(-1)[64 * 3 + 5] = 2048                 # 11 magnitude bits after the first AC scan's shift by one
    for flags in (1, 2):
        out, status, _, _ = emulate(j, 90, flags)
        assert out is None and status == 1


def test_file_capacity():
    img = photo(64, 64, 9)
    j = twin(img, 90, "4:2:0")
    data = save(img, 90, "4:2:0", progressive=True)
    out, status, _, _ = emulate(j, 90, 2, capacity=len(data))
    assert out == data and status == 0
    out, status, _, _ = emulate(j, 90, 2, capacity=len(data) - 1)
    assert out is None and status == 4


def test_library_exports_the_flagged_device_coder():
    L = _native.lib()
    for name in ("ifhip_jpeg_encode_flags_batch_device", "ifhip_jpeg_enc_stage_max_file_bytes_for"):
        assert hasattr(L, name)
