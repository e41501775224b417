"""Host mirror of GifEncoder::write_frame (imageflow_core/src/codecs/gif/mod.rs:385-592 over the gif crate) on the device GIF
coder of libimageflow_hip.so (csrc/gif_encode.hip): BGRA / BGRX frames that stay in HBM -> complete single-frame GIF89a
files in HBM.  For tests and tools; the job path is the `"gif"` preset of `encode` on a context whose GIF encoder is
switched on (Context.set_gif_encoder, csrc/shim_encode.cpp)."""
import ctypes as C

import torch

from .. import _native
from ..graphics.bitmaps import Bitmap
from ._file_encoder import FileEncodeStage, encode_host, files_as_bytes, palettes_from_taps

GIF_FILE_OVERFLOW = 1                   # include/imageflow_hip.h IFHIP_GIF_FILE_OVERFLOW
SEGMENT_PIXELS = 16384                  # IFHIP_GIF_ENC_SEGMENT_PIXELS
MAX_DIMENSION = 65535                   # size_16()
PALETTE_TAP = 1028                      # 256 RGBA entries in file order, then the count


def _bind():
    L = _native.lib()
    if getattr(L, "_gif_enc_bound", False):
        return L
    L.ifhip_gif_enc_stage_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32]
    L.ifhip_gif_enc_stage_destroy.argtypes = [C.c_void_p]
    L.ifhip_gif_enc_stage_destroy.restype = None
    L.ifhip_gif_enc_stage_max_file_bytes.argtypes = [C.c_void_p]
    L.ifhip_gif_enc_stage_max_file_bytes.restype = C.c_size_t
    L.ifhip_gif_encode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_int,
                                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_gif_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]
    L.ifhip_gif_enc_stage_max_animation_bytes.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_size_t)]
    L.ifhip_gif_encode_animation_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L._gif_enc_bound = True
    return L


class GifEncodeStage(FileEncodeStage):
    """ifhip_gif_enc_stage: one geometry, the scratch of a batch in flight (one stream at a time)."""

    def __init__(self, width, height, max_images=1, device="cuda:0"):
        self.width, self.height, self.max_images = width, height, max_images
        self._create(_bind(), "ifhip_gif_enc_stage", device, width, height, max_images)

    def encode_device(self, frames: Bitmap, repeat=-1, delay=0, needs_user_input=False, file_pitch=None, taps=False):
        """frames: n BGRA frames of the stage's geometry.  Returns (files [n, file_pitch] uint8, lengths [n] int32, status [n]
        int32, palettes [n, 1028] uint8 or None, indices [n, h, w] uint8 or None), all cuda tensors; nothing is synchronised."""
        n = frames.n
        palettes = torch.zeros((n, PALETTE_TAP), dtype=torch.uint8, device=self.device) if taps else None
        indices = torch.zeros((n, self.height, self.width), dtype=torch.uint8, device=self.device) if taps else None
        files, lengths, status = self._batch(n, lambda d_files, pitch, d_lengths, d_status: (
            _bind().ifhip_gif_encode_batch_device, self._h, frames.data.data_ptr(), frames.image_bytes, frames.stride, 1 if frames.alpha_meaningful else 0, n,
            repeat, delay, 1 if needs_user_input else 0, d_files, pitch, d_lengths, d_status, palettes.data_ptr() if taps else None,
            indices.data_ptr() if taps else None), file_pitch)
        return files, lengths, status, palettes, indices

    def encode(self, frames: Bitmap, repeat=-1, delay=0, needs_user_input=False, file_pitch=None, taps=False):
        """The n files as bytes (None for a file that did not fit file_pitch), the status words and, with taps, per image the
        palette [count, 4] RGBA in file order and the indices [h, w]."""
        files, lengths, status, palettes, indices = self.encode_device(frames, repeat, delay, needs_user_input, file_pitch, taps)
        out, words = files_as_bytes(files, lengths, status)
        if not taps:
            return out, words
        idx = indices.cpu().numpy()
        return out, words, palettes_from_taps(palettes), [idx[i] for i in range(frames.n)]

    def max_animation_bytes(self, n_frames):
        n = C.c_size_t(0)
        _native.check(_bind().ifhip_gif_enc_stage_max_animation_bytes(self._h, n_frames, C.byref(n)))
        return int(n.value)

    def encode_animation_device(self, frames: Bitmap, delays, user_input, repeat=-1, capacity=None):
        """frames: n BGRA frames of the stage's geometry, n beyond max_images runs the stage in chunks.  Returns (file
        [capacity] uint8, length [1] int32, status [1] int32), cuda tensors; nothing is synchronised."""
        n = frames.n
        if capacity is None:
            capacity = self.max_animation_bytes(n)
        file = torch.empty((capacity + 3) // 4 * 4, dtype=torch.uint8, device=self.device)
        length = torch.zeros(1, dtype=torch.int32, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        d = (C.c_uint32 * n)(*[int(v) for v in delays])
        u = (C.c_uint8 * n)(*[1 if v else 0 for v in user_input])
        self._on_stream(_bind().ifhip_gif_encode_animation_device, self._h, frames.data.data_ptr(), frames.image_bytes, frames.stride,
                        1 if frames.alpha_meaningful else 0, n, repeat, d, u, file.data_ptr(), capacity, length.data_ptr(), status.data_ptr())
        return file, length, status

    def encode_animation(self, bitmap_batch: Bitmap, delays, user_input, repeat=-1, capacity=None, with_status=False):
        """The n frames as ONE animated GIF89a file: bytes (with_status: (bytes or None, status word))."""
        file, length, status = self.encode_animation_device(bitmap_batch, delays, user_input, repeat, capacity)
        k, word = int(length.cpu()[0]), int(status.cpu()[0])
        data = file[:k].cpu().numpy().tobytes() if k else None
        if with_status:
            return data, word
        if word or data is None:
            raise RuntimeError(f"device GIF coder dropped the animation: status {word}")
        return data


def encode_gif(bitmap: Bitmap, repeat=-1, delay=0, needs_user_input=False):
    """GifEncoder::write_frame on every frame of the bitmap: a file per frame.  Returns the files."""
    stage = GifEncodeStage(bitmap.w, bitmap.h, bitmap.n, bitmap.data.device)
    files, status = stage.encode(bitmap, repeat, delay, needs_user_input)
    if any(status):                                                       # (cannot happen with the stage's own pitch)
        raise RuntimeError(f"device GIF coder dropped images: status {status}")
    return files


def encode_gif_host(bgra, width, height, stride, alpha_meaningful=True, repeat=-1, delay=0, needs_user_input=False):
    """Host-buffer drop-in (numpy): BGRA rows -> the file's bytes."""
    L = _bind()
    return encode_host(L, "ifhip_gif_enc_stage", (width, height, 1), L.ifhip_gif_encode, bgra, width, height, stride,
                       (1 if alpha_meaningful else 0, repeat, delay, 1 if needs_user_input else 0))
