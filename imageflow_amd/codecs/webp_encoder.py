"""Host mirror of the lossless half of WebPEncoder (imageflow_core/src/codecs/webp.rs:281-345 over libwebp's
WebPEncodeLosslessBGRA / WebPEncodeLosslessBGR; chosen in codecs/auto.rs:282-319) on the device WebP coder of
libimageflow_hip.so (csrc/webp_encode.hip): BGRA / BGRX frames that stay in HBM -> complete lossless WebP (VP8L) files in
HBM.  For tests and tools; the job path is the `webplossless` preset of `encode` (csrc/shim_encode.cpp)."""
import ctypes as C

import numpy as np

from .. import _native
from ..graphics.bitmaps import Bitmap
from ._file_encoder import FileEncodeStage, encode_host, files_as_bytes

WEBP_FILE_OVERFLOW = 1                  # include/imageflow_hip.h IFHIP_WEBP_FILE_OVERFLOW
MAX_DIMENSION = 16384                   # 14 bits of width - 1 and height - 1
WEBP_ENC_COLOR_INDEXING = 1             # include/imageflow_hip.h IFHIP_WEBP_ENC_COLOR_INDEXING: stage flag, frames of at most 256 colours may be indexed


def _bind():
    L = _native.lib()
    if getattr(L, "_webp_enc_bound", False):
        return L
    L.ifhip_webp_enc_stage_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
    L.ifhip_webp_enc_stage_create_flags.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32]
    L.ifhip_webp_enc_stage_destroy.argtypes = [C.c_void_p]
    L.ifhip_webp_enc_stage_destroy.restype = None
    L.ifhip_webp_enc_stage_max_file_bytes.argtypes = [C.c_void_p]
    L.ifhip_webp_enc_stage_max_file_bytes.restype = C.c_size_t
    L.ifhip_webp_encode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_webp_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L._webp_enc_bound = True
    return L


class _WithFlags:
    """the stage functions as FileEncodeStage._create names them, the create being the one that takes flags"""

    def __init__(self, L):
        self.ifhip_webp_enc_stage_create = L.ifhip_webp_enc_stage_create_flags
        self.ifhip_webp_enc_stage_destroy = L.ifhip_webp_enc_stage_destroy
        self.ifhip_webp_enc_stage_max_file_bytes = L.ifhip_webp_enc_stage_max_file_bytes


class WebpEncodeStage(FileEncodeStage):
    """ifhip_webp_enc_stage: one geometry and alpha mode, the scratch of a batch in flight (one stream at a time).
    color_indexing: IFHIP_WEBP_ENC_COLOR_INDEXING, a frame of at most 256 colours is written with a colour table where that
    is the smaller file."""

    def __init__(self, width, height, alpha_meaningful=True, max_images=1, device="cuda:0", color_indexing=False):
        self.width, self.height, self.alpha_meaningful, self.max_images = width, height, bool(alpha_meaningful), max_images
        self.color_indexing = bool(color_indexing)
        self._create(_WithFlags(_bind()), "ifhip_webp_enc_stage", device, width, height, 1 if alpha_meaningful else 0, max_images,
                     WEBP_ENC_COLOR_INDEXING if color_indexing else 0)

    def encode_device(self, frames: Bitmap, file_pitch=None, files=None, lengths=None, status=None):
        """frames: n BGRA frames of the stage's geometry.  Returns (files [n, file_pitch] uint8, lengths [n] int32, status [n]
        int32), all cuda tensors; nothing is synchronised."""
        return self._batch(frames.n, lambda d_files, pitch, d_lengths, d_status: (
            _bind().ifhip_webp_encode_batch_device, self._h, frames.data.data_ptr(), frames.image_bytes, frames.stride, frames.n, d_files, pitch, d_lengths,
            d_status), file_pitch, files, lengths, status)

    def encode(self, frames: Bitmap, file_pitch=None):
        """The n files as bytes (None for a file that did not fit file_pitch) and the status words."""
        return files_as_bytes(*self.encode_device(frames, file_pitch))


def encode_webp_lossless(bitmap: Bitmap, color_indexing=False):
    """WebPEncoder::write_frame for EncoderPreset::WebPLossless on every frame of the bitmap: BGRA when the frame's alpha is
    meaningful, else BGR (the file then says alpha_is_used = 0 and decodes to alpha 255); no matte.  Returns the files."""
    stage = WebpEncodeStage(bitmap.w, bitmap.h, bitmap.alpha_meaningful, bitmap.n, bitmap.data.device, color_indexing=color_indexing)
    files, status = stage.encode(bitmap)
    if any(status):                                                       # (cannot happen with the stage's own pitch)
        raise RuntimeError(f"device WebP coder dropped images: status {status}")
    return files


def encode_webp_host(bgra, width, height, stride, alpha_meaningful=True, color_indexing=False, device="cuda:0"):
    """Host-buffer drop-in (numpy): BGRA rows -> the file's bytes.  The C drop-in's stage carries no flags, so with
    color_indexing the rows go through a flagged stage of one image on `device` instead."""
    L = _bind()
    if color_indexing:
        rows = np.ascontiguousarray(bgra, np.uint8).reshape(1, height, stride)
        return encode_webp_lossless(Bitmap.from_numpy(rows, width, height, stride, device, alpha_meaningful=bool(alpha_meaningful)), color_indexing=True)[0]
    alpha = 1 if alpha_meaningful else 0
    return encode_host(L, "ifhip_webp_enc_stage", (width, height, alpha, 1), L.ifhip_webp_encode, bgra, width, height, stride, (alpha,))
