"""The animation paths of the GIF decoder and coder for the tests, without a device.

* assemble(): the EXPECTED animation file, put together in plain Python from the per-frame results of the one-frame coder's
  emulation (tests/gif_encode_emu.py): "GIF89a", the logical screen, NETSCAPE2.0 when repeat >= 0, then per frame the
  one-frame file's own graphic control extension .. terminator (with the disposal bits of the rule below), then ';'.
* layout(): the same file as csrc/gif_encode_core.hpp lays it out over the file's dwords, chunk by chunk
  (tests/gif_animation_emulate.cpp), from the same per-frame results.
* decode_frames(): every composed screen of a file in one replay (csrc/gif_decode_core.hpp through the same program).

The disposal rule: a one-frame file carries what the one-frame coder writes (Keep); in a file of more than one frame, frames
of meaningful alpha carry disposal 2 (restore to background), frames without alpha carry Keep."""
import ctypes as C
import io
import os
import subprocess
import tempfile

import numpy as np

from tests import gif_encode_emu as G
from tests import gif_oracle as O
from tests import png_quantize_emu as Q

HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = {}
FILE_OVERFLOW = 1
SCREEN = 13                                   # signature and logical screen descriptor
NETSCAPE = 19


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="gif_animation_emulate_")
        so = os.path.join(d, "libgif_animation_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", os.path.join(HERE, "gif_animation_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.gif_anim_emu_decode_frames.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        lib.gif_anim_emu_decode_frames.restype = C.c_uint32
        lib.gif_anim_emu_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.gif_anim_emu_layout.restype = C.c_uint32
        lib.gif_anim_emu_max_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.gif_anim_emu_max_bytes.restype = C.c_uint64
        _EMU["lib"] = lib
    return _EMU["lib"]


def max_animation_bytes(w, h, n):
    return int(emulator().gif_anim_emu_max_bytes(w, h, n))


def decode_frames(data, stride=None, pad_rows=0, grid_x=3, fill=0x5A):
    """-> (status, screens [n, h, w, 4] BGRA or None, the whole block [n, pitch] as it was left)"""
    P = O.parse(data, 1 << 30)
    w, h = (P["w"], P["h"]) if P else (0, 0)
    n = max(P["frames_seen"], 1) if P else 1
    stride = stride or 4 * w
    pitch = (h + pad_rows) * stride
    src = np.frombuffer(bytes(data) + b"\0", np.uint8).copy()
    out, dims = np.full((n, max(pitch, 1)), fill, np.uint8), np.zeros(3, np.uint32)
    st = emulator().gif_anim_emu_decode_frames(src.ctypes.data, len(data), out.ctypes.data, out.size, pitch, stride, dims[0:].ctypes.data, dims[1:].ctypes.data,
                                               dims[2:].ctypes.data, grid_x)
    if st:
        assert (out == fill).all() and dims[2] == 0, "a damaged file writes no screen"
        return st, None, out
    assert int(dims[2]) == P["frames_seen"]
    return 0, out[:, :h * stride].reshape(n, h, stride)[:, :, :4 * w].reshape(n, h, w, 4).copy(), out


def dispose_of(n_frames, alpha):
    return 2 if n_frames > 1 and alpha else 1


def coded(frames, alpha, delays, user_input):
    """the one-frame coder's emulation on every frame: its dicts, each with "stream" (the LZW data of its file)"""
    out = []
    for f, d, u in zip(frames, delays, user_input):
        q = G.encode(f, alpha=alpha, repeat=-1, delay=d, user_input=u)
        assert q["status"] == 0
        fr = O.parse(q["file"])["frames"][0]
        q["stream"] = fr["stream"]
        assert len(q["stream"]) == q["data_bytes"]
        out.append(q)
    return out


def assemble(frames, alpha, delays, user_input, repeat=-1, per_frame=None):
    """-> (the expected file, the per-frame results)"""
    per_frame = per_frame or coded(frames, alpha, delays, user_input)
    h, w, _ = frames[0].shape
    first = G.encode(frames[0], alpha=alpha, repeat=repeat, delay=delays[0], user_input=user_input[0])["file"]
    out = bytearray(first[:SCREEN + (NETSCAPE if repeat >= 0 else 0)])
    for q in per_frame:
        body = bytearray(q["file"][SCREEN:-1])                              # graphic control extension .. the data's terminator
        assert body[:3] == b"\x21\xF9\x04" and body[3] >> 2 == 1
        body[3] = dispose_of(len(frames), alpha) << 2 | body[3] & 3
        out += body
    return bytes(out + b"\x3B"), per_frame


def layout(frames, alpha, delays, user_input, repeat=-1, chunk=None, cap=None, per_frame=None):
    """csrc/gif_encode_core.hpp's layout over the file's dwords -> (file or None, status)"""
    per_frame = per_frame or coded(frames, alpha, delays, user_input)
    h, w, _ = frames[0].shape
    n = len(frames)
    cap = max_animation_bytes(w, h, n) if cap is None else cap
    pitch = (max(q["data_bytes"] for q in per_frame) + 3) // 4 * 4
    streams = np.full((n, pitch), 0xA5, np.uint8)
    keys, counts, n_trans, data = np.zeros((n, 256), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, q in enumerate(per_frame):
        streams[i, :q["data_bytes"]] = np.frombuffer(q["stream"], np.uint8)
        p = q["palette"].astype(np.uint32)
        keys[i, :len(p)] = p[:, 2] | p[:, 1] << 8 | p[:, 0] << 16 | p[:, 3] << 24
        counts[i], n_trans[i], data[i] = len(p), q["n_trans"], q["data_bytes"]
    d, u = np.asarray(delays, np.uint32), np.asarray([1 if v else 0 for v in user_input], np.uint8)
    out, st = np.zeros(cap + 8, np.uint8), C.c_uint32(0)
    k = emulator().gif_anim_emu_layout(w, h, n, chunk or n, 1 if alpha else 0, repeat, d.ctypes.data, u.ctypes.data, counts.ctypes.data, keys.ctypes.data,
                                       n_trans.ctypes.data, streams.ctypes.data, pitch, data.ctypes.data, out.ctypes.data, cap, C.byref(st))
    assert k != 0xFFFFFFFF
    return (out[:k].tobytes() if k else None), int(st.value)


def pillow_frames(data):
    """-> (frames RGBA [n, h, w, 4] as a viewer shows them, durations in ms, info of the first frame)"""
    from PIL import Image, ImageSequence
    im = Image.open(io.BytesIO(data))
    assert im.format == "GIF"
    info = dict(im.info)
    frames, durations = [], []
    for fr in ImageSequence.Iterator(im):
        durations.append(fr.info.get("duration", 0))
        frames.append(np.asarray(fr.convert("RGBA")).copy())
    return np.stack(frames), durations, info, im.n_frames


# ---- the case frames ------------------------------------------------------------------------------------------------------------------

def photo_frames(w, h, n, alpha, seed=1):
    """photos whose transparent regions (with alpha) lie at another place in every frame: what shows through matters"""
    out = [np.ascontiguousarray(np.roll(Q.photo_rgba(w, h, seed=seed + 7 * k, alpha=alpha), (h // 3) * k, axis=0)) for k in range(n)]
    if alpha:
        masks = [f[..., 3] < 16 for f in out]
        assert all(m.any() and not m.all() for m in masks) and all((masks[k] & ~masks[k - 1]).any() for k in range(1, n))
    return out


def residue_frames():
    """Frames of 9 x 7 whose bodies' lengths cover all four residues modulo 4 (asserted by the test that uses them): every body
    then starts at another byte of a dword.  A seeded search with the emulation."""
    if "res" not in _EMU:
        found = {}
        for seed in range(400):
            f = G.noise_frame(9, 7, 2 + seed % 7, seed=seed)
            q = G.encode(f, alpha=False)
            r = (len(q["file"]) - SCREEN - 1) % 4
            found.setdefault(r, f)
            if len(found) == 4:
                break
        assert sorted(found) == [0, 1, 2, 3]
        _EMU["res"] = [found[1], found[3], found[2], found[0], found[1], found[1], found[2]]
    return _EMU["res"]


def body_lengths(per_frame):
    return [len(q["file"]) - SCREEN - 1 for q in per_frame]
