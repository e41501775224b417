"""What the front ends of the device file coders (libpng_encoder, pngquant, webp_encoder, gif_encoder) share: the stage's handle,
the buffers and the stream hand-off of a batch around the library's ifhip_*_batch_device, the download of the files and the
host-buffer drop-in (csrc/encode_handoff.hpp is the same hand-off on the C side).  A new writer's front end binds its
functions, derives its stage from FileEncodeStage and calls these."""
import ctypes as C

import numpy as np
import torch

from .. import _native


class FileEncodeStage:
    """An ifhip_*_stage of the library: the handle, its bound on a file, the scratch of a batch in flight (one stream at a time)."""

    def _create(self, L, prefix, device, *args):
        """prefix: the stage's C name ("ifhip_png_enc_stage"); args: what its _create takes behind the out-pointer."""
        self.device = torch.device(device)
        self._h = C.c_void_p()
        self._destroy = getattr(L, prefix + "_destroy")
        _native.check(getattr(L, prefix + "_create")(C.byref(self._h), *args))
        self.max_file_bytes = int(getattr(L, prefix + "_max_file_bytes")(self._h))

    def _on_stream(self, fn, *args):
        """fn(*args, stream) on torch's current stream of the stage's device"""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            _native.check(fn(*args, C.c_void_p(stream)))

    def _batch(self, n, call, file_pitch=None, files=None, lengths=None, status=None):
        """call(files, file_pitch, lengths, status) gives the arguments of the batch function and the function itself in front.
        -> (files [n, file_pitch] uint8, lengths [n] int32, status [n] int32), cuda tensors; nothing is synchronised."""
        if file_pitch is None:
            file_pitch = files.shape[1] if files is not None else (self.max_file_bytes + 15) // 16 * 16
        if files is None:
            files = torch.empty((n, file_pitch), dtype=torch.uint8, device=self.device)
        if lengths is None:
            lengths = torch.zeros(n, dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.zeros(n, dtype=torch.int32, device=self.device)
        self._on_stream(*call(files.data_ptr(), file_pitch, lengths.data_ptr(), status.data_ptr()))
        return files, lengths, status

    def __del__(self):
        try:
            if self._h:
                torch.cuda.synchronize(self.device)
                self._destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


def files_as_bytes(files, lengths, status):
    """The n files as bytes (None for an image without one) and the status words as ints."""
    lengths, status = lengths.cpu().numpy(), status.cpu().numpy()
    host = files[:, :max(int(lengths.max()), 1)].cpu().numpy()
    return [host[i, :int(k)].tobytes() if k else None for i, k in enumerate(lengths)], [int(s) for s in status]


def palettes_from_taps(palettes):
    """palettes [n, 1028] uint8 (cuda): per image 256 RGBA entries in file order, then the count -> a list of [count, 4] arrays"""
    pal = palettes.cpu().numpy()
    return [pal[i, :1024].reshape(256, 4)[:int(pal[i, 1024:].view(np.uint32)[0])].copy() for i in range(pal.shape[0])]


def encode_host(L, prefix, stage_args, drop_in, bgra, width, height, stride, middle, tail=()):
    """The host-buffer drop-in (numpy): a stage for one image says how large a file may be (the bound the drop-in itself sizes
    its file by; geometry only, nothing is allocated), then drop_in(bitmap, width, height, stride, *middle, out, capacity,
    &len, *tail).  -> the file's bytes (b"" where there is none)"""
    src = np.ascontiguousarray(bgra, np.uint8)
    n = C.c_size_t(0)
    h = C.c_void_p()
    _native.check(getattr(L, prefix + "_create")(C.byref(h), *stage_args))
    out = np.empty(getattr(L, prefix + "_max_file_bytes")(h), np.uint8)
    getattr(L, prefix + "_destroy")(h)
    _native.check(drop_in(src.ctypes.data, width, height, stride, *middle, out.ctypes.data, out.size, C.byref(n), *tail))
    return out[:n.value].tobytes()
