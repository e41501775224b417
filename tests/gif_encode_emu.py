"""The CPU emulation of the device GIF coder for the tests: tests/gif_encode_emulate.cpp (with the palette quantiser's
emulation, tests/png_quantize_emulate.cpp and tests/png_emulate.cpp) built with g++ once per session, a wrapper around its
entry, the case frames the CPU and the GPU tests share, and the checks of a coded file against Pillow and against this
project's own GIF decoder."""
import ctypes as C
import io
import os
import subprocess
import tempfile

import numpy as np

from tests import png_quantize_emu as Q

HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = {}
FILE_OVERFLOW = 1


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="gif_encode_emulate_")
        so = os.path.join(d, "libgif_encode_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", os.path.join(HERE, "gif_encode_emulate.cpp"),
                        os.path.join(HERE, "png_quantize_emulate.cpp"), os.path.join(HERE, "png_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.gifenc_emu_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gifenc_emu_max_file_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.gifenc_emu_max_file_bytes.restype = C.c_uint64
        lib.gifenc_emu_segment_pixels.restype = C.c_uint32
        _EMU["lib"] = lib
    return _EMU["lib"]


def segment_pixels():
    return int(emulator().gifenc_emu_segment_pixels())


def max_file_bytes(w, h):
    return int(emulator().gifenc_emu_max_file_bytes(w, h))


def encode(rgba, alpha=True, repeat=-1, delay=0, user_input=False, stride=None, cap=None):
    """The emulation on one RGBA frame.  Returns a dict: file (bytes or None), status, palette [count, 4] RGBA in file
    order, indices [h, w], segments, data_bytes, min_code, n_trans."""
    L = emulator()
    h, w, _ = rgba.shape
    rows = Q.bgra_rows(rgba, stride)
    cap = max_file_bytes(w, h) if cap is None else cap
    out = np.zeros(max(cap, 1), np.uint8)
    ln, st = C.c_size_t(0), C.c_uint32(0)
    pal, idx, info = np.zeros(1028, np.uint8), np.zeros((h, w), np.uint8), np.zeros(4, np.uint32)
    rc = L.gifenc_emu_encode(rows.ctypes.data, w, h, rows.shape[1], 1 if alpha else 0, repeat, delay, 1 if user_input else 0, out.ctypes.data, cap,
                             C.byref(ln), C.byref(st), pal.ctypes.data, idx.ctypes.data, info.ctypes.data)
    assert rc == 0, rc
    count = int(pal[1024:].view(np.uint32)[0])
    return {"file": out[:ln.value].tobytes() if ln.value else None, "status": int(st.value), "palette": pal[:1024].reshape(256, 4)[:count].copy(),
            "indices": idx, "segments": int(info[0]), "data_bytes": int(info[1]), "min_code": int(info[2]), "n_trans": int(info[3])}


def normalized(rgba, alpha=True):
    """The frame as the coder sees it (codecs/gif/mod.rs:385-592): meaningful alpha below 16 is 00 00 00 00, every other
    pixel is opaque."""
    out = rgba.copy()
    gone = out[..., 3] < 16 if alpha else np.zeros(out.shape[:2], bool)
    out[..., 3] = 255
    out[gone] = 0
    return out


def pillow_rgba(data):
    """(RGBA [h, w, 4] of the first frame with transparent pixels as 0 0 0 0, indices [h, w], info)"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.format == "GIF" and im.mode == "P", (im.format, im.mode)
    idx = np.asarray(im).copy()
    info = dict(im.info)
    rgba = np.asarray(im.convert("RGBA")).copy()
    rgba[rgba[..., 3] == 0] = 0
    return rgba, idx, info


def decoded(q):
    """what a file of the emulation's taps decodes to: palette[indices], RGBA"""
    return q["palette"][q["indices"]]


def check_file(q, w, h):
    """Pillow and this project's decoder (its oracle and its CPU emulation) read the file as the taps say."""
    from tests import gif_oracle as O
    from tests.test_gif_decode_core import emulate as decoder_emulation
    data = q["file"]
    want = decoded(q)
    rgba, idx, info = pillow_rgba(data)
    assert rgba.shape == (h, w, 4)
    assert np.array_equal(idx, q["indices"]), "Pillow reads the indices the coder chose"
    assert np.array_equal(rgba, want), "Pillow decodes to palette[index], transparent pixels at alpha 0"
    st, screen, P = O.decode(data)
    assert st == O.OK and P["global_palette"] is None and len(P["frames"]) == 1
    fr = P["frames"][0]
    assert (fr["w"], fr["h"], fr["left"], fr["top"], fr["interlace"]) == (w, h, 0, 0, False)
    assert fr["m"] == q["min_code"] and len(fr["stream"]) == q["data_bytes"]
    assert len(fr["palette"]) == max(2, 1 << (len(q["palette"]) - 1).bit_length()), "padded to a power of two"
    assert not fr["palette"][len(q["palette"]):].any(), "padded with black"
    assert fr["transparent"] == (0 if q["n_trans"] else None)
    assert np.array_equal(screen[..., [2, 1, 0, 3]], want)
    st2, screen2, _ = decoder_emulation(data, cap=max(1 << 20, 4 * w * h))
    assert st2 == 0 and np.array_equal(screen2, screen)
    return info


# ---- the case frames ------------------------------------------------------------------------------------------------------------------

def noise_frame(w, h, colours=256, seed=1):
    """seeded noise over `colours` opaque colours: LZW finds next to nothing, the table fills as fast as it can"""
    rng = np.random.default_rng(seed)
    pal = np.concatenate([rng.permutation(256)[:colours, None], rng.integers(0, 256, (colours, 2))], 1).astype(np.uint8)   # distinct in R
    idx = np.concatenate([np.arange(colours) % colours, rng.integers(0, colours, max(0, w * h - colours))])[:w * h]
    rng.shuffle(idx)
    return np.dstack([pal[idx].reshape(h, w, 3), np.full((h, w), 255, np.uint8)])


def alpha_edge_frame():
    """alpha 15 next to alpha 16, 0 and 255, on a few colours"""
    rgba = np.zeros((6, 8, 4), np.uint8)
    rgba[..., 0] = np.arange(8)[None, :] * 30
    rgba[..., 1] = np.arange(6)[:, None] * 40
    rgba[..., 2] = 200
    rgba[..., 3] = np.array([0, 15, 16, 255, 15, 16, 1, 254], np.uint8)[None, :]
    return rgba


def cases():
    """name -> (RGBA frame, alpha_meaningful).  The smallest frames at which the coder can go wrong."""
    S = segment_pixels()
    out = {}
    for w, h in ((1, 1), (1, 2), (3, 5), (17, 40)):
        out[f"photo_{w}x{h}"] = (Q.photo_rgba(w, h, seed=5), False)
    out["one_colour"] = (np.full((7, 9, 4), (10, 20, 30, 255), np.uint8), False)
    two = np.full((7, 9, 4), (10, 20, 30, 255), np.uint8)
    two[2:5, 3:] = (200, 100, 50, 255)
    out["two_colours"] = (two, False)
    out["256_colours"] = (Q.colour_frame(40, 30, 256, seed=2), False)
    out["257_colours"] = (Q.colour_frame(40, 30, 257, seed=9), False)
    out["alpha_edge_meaningful"] = (alpha_edge_frame(), True)
    out["alpha_edge_ignored"] = (alpha_edge_frame(), False)
    gone = Q.photo_rgba(13, 9, seed=1)
    gone[..., 3] = 3
    out["all_transparent"] = (gone, True)
    for d in (-1, 0, 1):
        n = S + d
        w = max(c for c in range(1, 201) if n % c == 0)
        out[f"segment{d:+d}"] = (Q.photo_rgba(w, n // w, seed=11, alpha=d == 1), d == 1)
    out["noise_128x130"] = (noise_frame(128, 130, 256, seed=3), False)
    out["photo_150x130"] = (Q.photo_rgba(150, 130, seed=7), False)
    out["photo_alpha_70x50"] = (Q.photo_rgba(70, 50, seed=4, alpha=True), True)
    return out


def modulo_frames():
    """Three noise frames whose LZW data length is 0, 1 and 254 modulo 255: a seeded search over widths with the emulation."""
    if "mod" not in _EMU:
        found = {}
        for w in range(200, 4000):
            f = noise_frame(w, 3, 4, seed=w)
            r = encode(f, alpha=False)["data_bytes"] % 255
            if r in (0, 1, 254) and r not in found:
                found[r] = f
                if len(found) == 3:
                    break
        assert sorted(found) == [0, 1, 254], sorted(found)
        _EMU["mod"] = found
    return _EMU["mod"]
