"""The lossy WebP coder with IFHIP_VP8_ENC_INTRA4 without a device: csrc/vp8_encode_core.hpp's 4x4 search (vp8e_try_intra4 over the
decoder's own vp8_pred_sub16), the B_PRED record, the sub-mode contexts across macroblock borders, the two Y2 context chains, the
type 3 tokens and the flagged size bound, as tests/vp8_encode_intra4_emulate.cpp runs them in the schedule of
csrc/vp8_encode_intra4.hip.  The contract is DESIGN 4.19's: libwebp 1.6.0 through Pillow decodes every file to EXACTLY the pixels
the emulation expects -- which catches the mode contexts, the Y2 chains, type 3 and `inner` at once -- and the files' SHA-256 are
pinned in tests/vp8_encode_intra4_pins.json.  With flags 0 every byte is tests/vp8_encode_emulate.cpp's.  The modes must pay:
G(q) > 0 against the 16x16 coder at equal size.  The same small cases run again through a stand-alone program under ASan + UBSan."""
import ctypes as C
import hashlib
import json
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests import vp8_encode_emu as E
from tests import vp8_encode_intra4_emu as E4
from tests import vp8_gen as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PINS = os.path.join(HERE, "vp8_encode_intra4_pins.json")
FRAMES = E4.frames()
NAMES = sorted(FRAMES) + ["photo_800x450"]
_CACHE = {}


def frame_of(name):
    return (E.photo_frame(), False) if name == "photo_800x450" else FRAMES[name]


def coded(name, quality, flags=E4.INTRA4):
    """(file, expected BGRA, stats) of a named frame, computed once"""
    if (name, quality, flags) not in _CACHE:
        frame, alpha = frame_of(name)
        _CACHE[name, quality, flags] = E4.encode(frame, quality, alpha, flags)
    return _CACHE[name, quality, flags]


def fnv(data):
    s = 0x811C9DC5
    for b in bytes(data):
        s = ((s ^ b) * 0x01000193) & 0xFFFFFFFF
    return s


@pytest.mark.parametrize("quality", E4.QUALITIES)
@pytest.mark.parametrize("name", NAMES)
def test_libwebp_decodes_the_flagged_file_to_exactly_what_the_coder_reconstructed(name, quality):
    data, expect, st = coded(name, quality)
    frame, alpha = frame_of(name)
    h, w = frame.shape[:2]
    assert st["errors"] == 0 and st["max_level"] <= 2047
    assert st["n_i4"] + st["dc"] + st["tm"] + st["v"] + st["h"] == st["n_mbs"]
    assert len(data) <= E4.max_file_bytes(w, h, alpha), "the flagged bound"
    got, mode = E.pillow_bgra(data)
    assert got.shape == expect.shape and np.array_equal(got, expect), (name, quality, st["n_i4"])
    assert mode == ("RGBA" if st["alpha"] else "RGB")


@pytest.mark.parametrize("name", sorted(E.small_frames()))
def test_without_the_flag_every_byte_is_the_16x16_coders(name):
    frame, alpha = FRAMES[name]
    for q in E4.QUALITIES:
        data, expect, st = coded(name, q, 0)
        old, old_expect, old_st = E.encode(frame, q, alpha)
        assert data == old and np.array_equal(expect, old_expect) and st["n_i4"] == 0, (name, q)
        assert E4.max_file_bytes(frame.shape[1], frame.shape[0], alpha, 0) == int(E.emulator().vp8e_emu_max_file_bytes(frame.shape[1], frame.shape[0], 1 if alpha else 0))


def test_which_macroblocks_take_the_4x4_modes():
    for q in E4.QUALITIES:
        assert coded("flat_40x40", q)[2]["n_i4"] == 0, q                # nothing to gain: the tie, and the penalty, go to 16x16
    for name in sorted(E4.mix_frames()):
        for q in (50, 85, 100):
            st = coded(name, q)[2]
            print(name, q, "n_i4", st["n_i4"], "of", st["n_mbs"], "\n", st["modes"])
            assert 0 < st["n_i4"] < st["n_mbs"], (name, q)
            assert st["row_borders"] > 0 and st["column_borders"] > 0, "B_PRED and 16x16 macroblocks adjacent in both directions"
    st = coded("photo_800x450", 75)[2]
    assert 0 < st["n_i4"] < st["n_mbs"]
    # the texture goes to B_PRED and the flat macroblocks stay 16x16, at every quality of the frames' purpose
    frame = E4.mix_frames()["mix_64x48"][0]
    for q in (50, 85, 100):
        modes = coded("mix_64x48", q)[2]["modes"]
        for y in range(3):
            for x in range(4):
                assert (modes[y, x] == 4) == bool((x + y) & 1), (q, x, y, modes)
    assert frame.shape == (48, 64, 4)


def test_the_y2_contexts_follow_the_two_chains_and_not_the_neighbours_own_bit():
    """A B_PRED macroblock between two 16x16 ones hands the Y2 context on.  Coded with the neighbour's own bit 24 instead (the
    emulation's test-only switch) the token streams differ, and libwebp no longer decodes the file to the expected pixels."""
    frame, alpha = FRAMES["mix_cols_80x32"]
    for q in (50, 85, 100):
        data, expect, st = coded("mix_cols_80x32", q)
        naive, naive_expect, naive_st = E4.encode(frame, q, alpha, E4.INTRA4 | E4.NAIVE_Y2)
        assert np.array_equal(st["modes"], naive_st["modes"]) and np.array_equal(expect, naive_expect), "the same decisions and reconstruction"
        assert G.chunk_body(data, b"VP8 ") != G.chunk_body(naive, b"VP8 "), q
        try:
            wrong = E.pillow_bgra(naive)[0]
        except Exception:                                               # (libwebp may also run out of a partition and give up)
            wrong = None
        assert wrong is None or not np.array_equal(wrong, expect), "the naive contexts are not what a decoder derives"
        assert np.array_equal(E.pillow_bgra(data)[0], expect)


def test_the_flagged_bound_is_computed_from_the_mode_table():
    L = E4.emulator()
    dearest = int(L.vp8e4_emu_dearest_leaf())
    assert int(L.vp8e4_emu_mode_bytes(0)) == 2
    # skip flag 3 bits, the is_i4 bit under 145, sixteen dearest leaves, the dearest chroma mode; vp8e_cost is 256 * log2(256 / p)
    cost = lambda p: 256.0 * np.log2(256.0 / p)
    bits = 3 * 256 + cost(145) + 16 * dearest + cost(256 - 142) + cost(256 - 114) + cost(256 - 183)
    assert abs(int(L.vp8e4_emu_mode_bytes(1)) - bits / 2048.0) <= 1.0
    # the dearest leaf, from the table itself: the most expensive way down the tree over all contexts
    text = open(os.path.join(ROOT, "imageflow_amd", "csrc", "vp8_tables.inc")).read()
    body = re.search(r"kVp8BModesProba\[10\]\[10\]\[9\] = \{(.*?)\};", text, re.S).group(1)
    proba = np.array([int(v) for v in re.findall(r"\d+", body)]).reshape(10, 10, 9)
    tree = [int(v) for v in re.search(r"kVp8BModeTree\[18\] = \{(.*?)\}", text).group(1).replace(" ", "").split(",")]

    def leaves(node, path):
        for bit in (0, 1):
            child = tree[2 * node + bit]
            if child > 0:
                yield from leaves(child, path + [(node, bit)])
            else:
                yield -child, path + [(node, bit)]
    paths = dict(leaves(0, []))
    assert sorted(paths) == list(range(10))
    worst = max(sum(cost(256 - proba[a, l, n] if bit else proba[a, l, n]) for n, bit in paths[m]) for a in range(10) for l in range(10) for m in range(10))
    assert abs(dearest - worst) <= 9.0, (dearest, worst)               # (vp8e_cost truncates each of at most nine terms)
    for w, h, alpha in ((800, 450, 0), (800, 450, 1), (17, 33, 1), (1, 1, 0), (16383, 16383, 0)):
        assert E4.max_file_bytes(w, h, alpha, 1) >= E4.max_file_bytes(w, h, alpha, 0)
    assert E4.max_file_bytes(800, 450, 0, 1) - E4.max_file_bytes(800, 450, 0, 0) == 1450 * (int(L.vp8e4_emu_mode_bytes(1)) - 2)


def test_the_flagged_files_are_the_pinned_bytes():
    pins = json.load(open(PINS))
    assert sorted(pins) == sorted("%s q%d" % (n, q) for n in NAMES for q in E4.QUALITIES)
    for n in NAMES:
        for q in E4.QUALITIES:
            assert hashlib.sha256(coded(n, q)[0]).hexdigest() == pins["%s q%d" % (n, q)], (n, q)


def test_the_same_cases_run_clean_under_asan_and_ubsan():
    """the stand-alone program: its own main, no sanitizer in this process; its output buffer is exactly the flagged bound"""
    d = tempfile.mkdtemp(prefix="vp8_encode_intra4_sanitize_")
    exe, cases = os.path.join(d, "vp8_encode_intra4_emulate"), os.path.join(d, "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DVP8_ENC4_EMU_MAIN", "-Wno-unused-function",
                    E4.SRC, "-o", exe], check=True)
    want = []
    with open(cases, "wb") as f:
        for name in sorted(FRAMES):
            frame, alpha = FRAMES[name]
            for q in E4.QUALITIES:
                data, expect, st = coded(name, q)
                f.write(struct.pack("<IIIII", frame.shape[1], frame.shape[0], 1 if alpha else 0, q, E4.INTRA4) + np.ascontiguousarray(frame).tobytes())
                want.append("0 %d %d %d %d" % (len(data), fnv(data), fnv(expect.tobytes()), st["n_i4"]))
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want


# ---- the modes must pay (the photo-like 800 x 450 frame) ---------------------------------------------------------------------------------
# G(q): the flagged file's PSNR minus the 16x16 coder's at the quality (swept 0..100) whose file is the smallest one not smaller
# than the flagged file -- the old coder gets at least as many bytes.  Both sides are deterministic emulations: G(q) > 0, no margin.
# D(q) against libwebp by the definition of tests/test_vp8_encode_core.py.  Recorded in DESIGN section 6.

def old_curve():
    if "old_curve" not in _CACHE:
        frame = E.photo_frame()
        _CACHE["old_curve"] = [(len(d), E.psnr(x, frame)) for d, x, _ in (E.encode(frame, q, False) for q in range(0, 101))]
    return _CACHE["old_curve"]


def test_the_4x4_modes_pay_at_equal_size_against_the_16x16_coder():
    frame = E.photo_frame()
    gains = {}
    for q in (25, 50, 75, 90):
        data, expect, st = coded("photo_800x450", q)
        mine = E.psnr(expect, frame)
        fits = [(size, p) for size, p in old_curve() if size >= len(data)]
        assert fits
        gains[q] = mine - min(fits)[1]
        print("quality %d: %d bytes (16x16 coder: %d), %.2f dB, %d of %d macroblocks B_PRED, G = %+.3f dB" % (q, len(data), old_curve()[q][0], mine, st["n_i4"], st["n_mbs"], gains[q]))
    for q in (50, 75, 90):
        assert gains[q] > 0, (q, gains)


RECORDED_D = {0: {25: 0.90, 50: 1.15, 75: 1.30, 90: 0.30}, 4: {25: 0.44, 50: 0.48, 75: 0.65, 90: 0.14}}


@pytest.mark.parametrize("method", [0, 4])
def test_psnr_at_equal_size_against_libwebp(method):
    """D(q) of the flagged coder, measured with Pillow 12.2.0 / libwebp 1.6.0 and recorded in DESIGN section 6; asserted as
    tests/test_vp8_encode_core.py asserts the 16x16 coder's: D(q) >= recorded - 0.25 dB, so that a change that costs quality fails
    and a Pillow rebuild does not."""
    from tests import test_vp8_encode_core as OLD
    frame = E.photo_frame()
    for q in (25, 50, 75, 90):
        data, expect, _ = coded("photo_800x450", q)
        mine = E.psnr(expect, frame)
        fits = [(size, p) for size, p in OLD.libwebp_curve(method) if size >= len(data)]
        assert fits, "libwebp has no file as large at any quality"
        d = mine - min(fits)[1]
        print("quality %d: %d bytes, %.2f dB, D = %+.2f dB against method=%d (the 16x16 coder: %+.2f)" % (q, len(data), mine, d, method, OLD.RECORDED_D[method][q]))
        assert d >= RECORDED_D[method][q] - 0.25, (q, method, d)


# ---- entry points without a GPU -------------------------------------------------------------------------------------------------------------

def test_header_bindings_and_library_agree_on_the_flag_entries():
    torch = pytest.importorskip("torch")  # noqa: F841
    from imageflow_amd import _native
    from imageflow_amd.codecs import webp_lossy_encoder as ENC
    extra = open(os.path.join(ROOT, "include", "imageflow_hip_webp_lossy_enc.h")).read()
    bindings = open(os.path.join(ROOT, "bindings", "hip_interop_webp_lossy_enc.rs")).read()
    main = open(os.path.join(ROOT, "include", "imageflow_hip.h")).read()
    L = _native.lib()
    for name in ("ifhip_webp_lossy_enc_stage_create_flags", "ifhip_webp_lossy_encode_flags"):
        assert name + "(" not in main
        assert re.search(r"IFHIP_API [^;]*\b%s\([^;]*uint32_t flags" % name, extra), name
        assert re.search(r"\bpub fn %s\([^;]*flags: u32" % name, bindings), name
        assert getattr(L, name) is not None
    assert re.search(r"#define IFHIP_VP8_ENC_INTRA4 1u\b", extra) and "pub const IFHIP_VP8_ENC_INTRA4: u32 = 1;" in bindings and ENC.VP8_ENC_INTRA4 == 1 == E4.INTRA4
    assert "kVp8eIntra4 = 1;" in open(os.path.join(ROOT, "imageflow_amd", "csrc", "vp8_encode_core.hpp")).read()


def test_an_unknown_flag_is_refused_and_the_bound_answers_for_the_stages_flag():
    pytest.importorskip("torch")
    from imageflow_amd.codecs import webp_lossy_encoder as ENC
    from imageflow_amd.errors import ErrorKind
    L, h = ENC._bind(), C.c_void_p()
    for flags in (2, 3, 0x100, 0x80000000):
        assert L.ifhip_webp_lossy_enc_stage_create_flags(C.byref(h), 64, 48, 0, 1, flags) == int(ErrorKind.InvalidArgument), flags
        assert L.ifhip_last_error_message() == b"InvalidArgument: unknown lossy WebP coder flags 0x%x" % flags and not h.value
    out, n = (C.c_uint8 * 16)(), C.c_size_t(0)
    frame = (C.c_uint8 * (48 * 256))()
    assert L.ifhip_webp_lossy_encode_flags(frame, 64, 48, 256, 0, 75.0, 2, out, 16, C.byref(n)) == int(ErrorKind.InvalidArgument)
    for args, words in (((0, 5, 1, 1, 1), b"InvalidArgument: Bitmap dimensions cannot be zero"), ((5, 5, 1, 0, 1), b"InvalidArgument: 1..65535 images per stage")):
        assert L.ifhip_webp_lossy_enc_stage_create_flags(C.byref(h), *args) == int(ErrorKind.InvalidArgument) and L.ifhip_last_error_message() == words
    for w, hh, alpha in ((800, 450, 0), (800, 450, 1), (17, 33, 1), (1, 1, 0)):
        bounds = []
        for flags in (0, 1):
            assert L.ifhip_webp_lossy_enc_stage_create_flags(C.byref(h), w, hh, alpha, 2, flags) == 0
            bounds.append(int(L.ifhip_webp_lossy_enc_stage_max_file_bytes(h)))
            assert bounds[-1] == E4.max_file_bytes(w, hh, alpha, flags)
            L.ifhip_webp_lossy_enc_stage_destroy(h)
        assert L.ifhip_webp_lossy_enc_stage_create(C.byref(h), w, hh, alpha, 2) == 0           # the old create is flags 0
        assert int(L.ifhip_webp_lossy_enc_stage_max_file_bytes(h)) == bounds[0] <= bounds[1]
        L.ifhip_webp_lossy_enc_stage_destroy(h)


def test_switch_value_2_without_a_gpu_answers_the_gpu_error_of_value_1():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_webp_lossy_encode_intra4.py runs the jobs")
    from imageflow_amd.abi import Context, pack_raw_bgra

    def send(value):
        with Context() as c:
            assert c.L.ifhip_shim_context_set_webp_lossy_encoder(c.p, value)
            c.add_input_buffer(0, pack_raw_bgra(np.zeros((8, 64), np.uint8), 16, 8, alpha_meaningful=False))
            c.add_output_buffer(1)
            status, _ = c.send_json("v1/execute", {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": {"webplossy": {"quality": 80.0}}}}]}})
            return status, c.error_code(), c.error_message()[0] if status != 200 else "", bytes(c.get_output_buffer(1)) if status == 200 else b""
    one, two = send(1), send(2)
    assert two == one and two[0] != 200 and "Gpu" in two[2] and two[3] == b""
    with Context() as c:
        assert c.set_webp_lossy_encoder(True, intra4=True) and c.set_webp_lossy_encoder(True) and c.set_webp_lossy_encoder(False, intra4=True)


def test_the_intra4_kernel_uses_no_scratch_and_holds_what_the_design_table_states():
    pytest.importorskip("torch")
    from imageflow_amd import build as B
    from tests.test_kernel_resources import resource_usage, _int
    rows = resource_usage(os.path.join(B.CSRC, "vp8_encode_intra4.hip"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert sorted(rows) == ["vp8e_code4_kernel"]
    r = rows["vp8e_code4_kernel"]
    assert _int(r, "ScratchSize [bytes/lane]") == 0, r
    assert _int(r, "LDS Size [bytes/block]") <= 64 * 1024, r
    assert _int(r, "VGPRs") <= 512 // (512 // 256), r
    m = re.search(r"\| `vp8e_code4_kernel` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", design)
    assert m and [int(g) for g in m.groups()] == [512, _int(r, "VGPRs"), _int(r, "LDS Size [bytes/block]"), 0], (m and m.groups(), r)
