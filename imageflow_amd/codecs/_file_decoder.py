"""What the front ends of the device file decoders (libpng_decoder, webp_decoder, gif_decoder) share: the body of decode_*_batch
and of the host-buffer drop-in decode_*_host around the library's ifhip_*_info, ifhip_*_decode_batch_device and ifhip_*_decode
(csrc/decode_handoff.hpp is the same hand-off on the C side).  A new reader's front end binds its three functions and calls these."""
import ctypes as C

import numpy as np
import torch

from .. import _native
from ..graphics.bitmaps import Bitmap, get_stride


def decode_batch(info_fn, batch_fn, Info, gets_frame, alpha, files, device, frames, fill, lead=()):
    """gets_frame(info): a file whose header parsed gets a frame; alpha(info): its alpha_meaningful; lead: the arguments of
    batch_fn between the file count and the frames (GIF's frame_index array).  -> (frames, status words)"""
    device = torch.device(device)
    n = len(files)
    bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
    out = list(frames) if frames is not None else [None] * n
    for i, b in enumerate(bufs):
        if out[i] is not None:
            continue
        info = Info()
        if info_fn(b.ctypes.data, b.size, C.byref(info)) != 0 or not gets_frame(info):
            continue
        stride = get_stride(info.width)
        data = torch.full((1, info.height * stride), 0 if fill is None else fill, dtype=torch.uint8, device=device)
        out[i] = Bitmap(data, info.width, info.height, stride, alpha_meaningful=alpha(info))
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    d_frames = (C.c_void_p * n)(*[o.data.data_ptr() if o is not None else None for o in out])
    frame_bytes = (C.c_size_t * n)(*[o.data.shape[1] if o is not None else 0 for o in out])
    strides = (C.c_uint32 * n)(*[o.stride if o is not None else 0 for o in out])
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    with torch.cuda.device(device):
        _native.check(batch_fn(ptrs, lens, n, *lead, d_frames, frame_bytes, strides, status.data_ptr(), C.c_void_p(stream)))
    return out, [int(s) for s in status.cpu().numpy()[:n]]


def decode_frames(info_fn, count_fn, frames_fn, Info, data, device, stride, fill):
    """One file, every screen: count_fn is the host walk (frames, delays, user-input flags), frames_fn the device call that
    writes screen k at k * screen_pitch.  -> (Bitmap of n screens or None, file status word, delays, user-input flags)"""
    device = torch.device(device)
    buf = np.frombuffer(bytes(data), np.uint8)
    info = Info()
    _native.check(info_fn(buf.ctypes.data, buf.size, C.byref(info)))
    n = C.c_uint32(0)
    _native.check(count_fn(buf.ctypes.data, buf.size, C.byref(n), None, None, 0))
    delays, flags = (C.c_uint32 * max(n.value, 1))(), (C.c_uint32 * max(n.value, 1))()
    _native.check(count_fn(buf.ctypes.data, buf.size, C.byref(n), delays, flags, n.value))
    stride = stride or get_stride(info.width)
    screens = torch.full((max(n.value, 1), info.height * stride), 0 if fill is None else fill, dtype=torch.uint8, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    written = C.c_uint32(0)
    stream = torch.cuda.current_stream(device).cuda_stream
    with torch.cuda.device(device):
        _native.check(frames_fn(buf.ctypes.data, buf.size, screens.data_ptr(), screens.stride(0), stride, screens.shape[0], status.data_ptr(), C.byref(written),
                                C.c_void_p(stream)))
    word = int(status.cpu()[0])
    if word:
        return Bitmap(screens, info.width, info.height, stride, alpha_meaningful=True), word, [], []
    assert written.value == n.value
    return Bitmap(screens[:n.value], info.width, info.height, stride, alpha_meaningful=True), 0, list(delays)[:n.value], [bool(f) for f in list(flags)[:n.value]]


def decode_host(info_fn, host_fn, Info, data, stride, out, lead=()):
    """lead: the arguments of host_fn between the file and the bitmap.  -> BGRA rows [h, stride] uint8"""
    buf = np.frombuffer(bytes(data), np.uint8)
    info = Info()
    _native.check(info_fn(buf.ctypes.data, buf.size, C.byref(info)))
    stride = stride or 4 * info.width
    if out is None:
        out = np.zeros((info.height, stride), np.uint8)
    status = C.c_uint32(0)
    _native.check(host_fn(buf.ctypes.data, buf.size, *lead, out.ctypes.data, stride, out.size, C.byref(status)))
    return out
