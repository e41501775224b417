"""Host mirror of PngquantEncoder (imageflow_core/src/codecs/pngquant.rs:35-139 over lode.rs:162-195) on the device palette
coder of libimageflow_hip.so (csrc/png_quantize.hip): BGRA / BGRX frames that stay in HBM -> 8-bit palette PNG files in HBM
-- colour histogram, palette growth and Lloyd refinement, nearest-entry remap with Floyd-Steinberg dithering, deflate, the
chunks and their CRCs.  A frame whose quantisation misses minimum_quality is written losslessly by the truecolour coder
(codecs/libpng_encoder.py), as the reference falls back.  For tests and tools; the job path is the `pngquant` preset of
`encode` (csrc/shim_encode.cpp)."""
import ctypes as C

import torch

from .. import _native
from ..graphics.bitmaps import Bitmap
from . import libpng_encoder
from ._file_encoder import FileEncodeStage, encode_host, files_as_bytes, palettes_from_taps

PNG_FILE_OVERFLOW, PNG_QUALITY_TOO_LOW = 1, 2   # include/imageflow_hip.h IFHIP_PNG_*
MAX_COLORS = 256
PALETTE_TAP = 4 * MAX_COLORS + 4                # per image: 256 RGBA entries in file order, then the count (u32le)
DEFAULT_ZLIB_LEVEL = 6                          # lode.rs:162-195: zlib level 6, or 9 under maximum_deflate


def _bind():
    L = _native.lib()
    if getattr(L, "_png_quant_bound", False):
        return L
    L.ifhip_png_quant_stage_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32]
    L.ifhip_png_quant_stage_destroy.argtypes = [C.c_void_p]
    L.ifhip_png_quant_stage_destroy.restype = None
    L.ifhip_png_quant_stage_max_file_bytes.argtypes = [C.c_void_p]
    L.ifhip_png_quant_stage_max_file_bytes.restype = C.c_size_t
    L.ifhip_png_quantize_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                                  C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_png_quantize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]
    L._png_quant_bound = True
    return L


def _opt(v):
    """An absent Option<u8> travels as -1."""
    return -1 if v is None else int(v)


class PngQuantStage(FileEncodeStage):
    """ifhip_png_quant_stage: one geometry, the scratch of a batch in flight (one stream at a time)."""

    def __init__(self, width, height, max_images=1, device="cuda:0"):
        self.width, self.height, self.max_images = width, height, max_images
        self._create(_bind(), "ifhip_png_quant_stage", device, width, height, max_images)

    def quantize_device(self, frames: Bitmap, quality=None, minimum_quality=None, speed=None, max_colors=MAX_COLORS, dither=True,
                        zlib_level=DEFAULT_ZLIB_LEVEL, alpha_meaningful=None, file_pitch=None, taps=False):
        """frames: n BGRA frames of the stage's geometry.  Returns a dict of cuda tensors: files [n, file_pitch] uint8, lengths
        [n] int32, status [n] int32, and with taps palettes [n, 1028] uint8, indices [n, h, w] uint8, mse [n] float64.
        Nothing is synchronised."""
        n = frames.n
        if alpha_meaningful is None:
            alpha_meaningful = frames.alpha_meaningful
        out = {}
        if taps:
            out["palettes"] = torch.zeros((n, PALETTE_TAP), dtype=torch.uint8, device=self.device)
            out["indices"] = torch.zeros((n, self.height, self.width), dtype=torch.uint8, device=self.device)
            out["mse"] = torch.zeros(n, dtype=torch.float64, device=self.device)
        ptr = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
        out["files"], out["lengths"], out["status"] = self._batch(n, lambda d_files, pitch, d_lengths, d_status: (
            _bind().ifhip_png_quantize_batch_device, self._h, frames.data.data_ptr(), frames.image_bytes, frames.stride, 1 if alpha_meaningful else 0, n,
            _opt(quality), _opt(minimum_quality), _opt(speed), int(max_colors), 1 if dither else 0, int(zlib_level), d_files, pitch, d_lengths, d_status,
            ptr("palettes"), ptr("indices"), ptr("mse")), file_pitch)
        return out

    def quantize(self, frames: Bitmap, **kw):
        """The n files as bytes (None for an image without one), the status words, and with taps=True a list of
        (palette [count, 4] RGBA, indices [h, w], mse) per image."""
        out = self.quantize_device(frames, **kw)
        files, status = files_as_bytes(out["files"], out["lengths"], out["status"])
        taps = None
        if "palettes" in out:
            idx, mse = out["indices"].cpu().numpy(), out["mse"].cpu().numpy()
            taps = [(pal, idx[i], float(mse[i])) for i, pal in enumerate(palettes_from_taps(out["palettes"]))]
        return files, status, taps


def encode_pngquant(bitmap: Bitmap, quality=None, minimum_quality=None, speed=None, maximum_deflate=None):
    """PngquantEncoder::write_frame on every frame of the bitmap: no matte (auto.rs:98-110), a palette file where the
    quantisation reaches minimum_quality, else a lossless RGBA / RGB file by alpha_meaningful (pngquant.rs:105-139).
    Returns the files."""
    level = 9 if maximum_deflate else DEFAULT_ZLIB_LEVEL
    stage = PngQuantStage(bitmap.w, bitmap.h, bitmap.n, bitmap.data.device)
    files, status, _ = stage.quantize(bitmap, quality=quality, minimum_quality=minimum_quality, speed=speed, zlib_level=level)
    if any(s not in (0, PNG_QUALITY_TOO_LOW) for s in status):           # (cannot happen with the stage's own pitch)
        raise RuntimeError(f"device palette coder dropped images: status {status}")
    if any(s == PNG_QUALITY_TOO_LOW for s in status):
        lossless = libpng_encoder.PngEncodeStage(bitmap.w, bitmap.h, libpng_encoder.color_type_for(bitmap.alpha_meaningful), bitmap.n, bitmap.data.device)
        plain, plain_status = lossless.encode(bitmap, level)
        if any(plain_status):
            raise RuntimeError(f"device PNG coder dropped images: status {plain_status}")
        files = [plain[i] if s == PNG_QUALITY_TOO_LOW else f for i, (f, s) in enumerate(zip(files, status))]
    return files


def quantize_png_host(bgra, width, height, stride, alpha_meaningful=True, quality=None, minimum_quality=None, speed=None):
    """Host-buffer form (numpy): BGRA rows -> (the file's bytes or None, the status word)."""
    L = _bind()
    status = C.c_uint32(0)
    data = encode_host(L, "ifhip_png_quant_stage", (width, height, 1), L.ifhip_png_quantize, bgra, width, height, stride,
                       (1 if alpha_meaningful else 0, _opt(quality), _opt(minimum_quality), _opt(speed)), (C.byref(status),))
    return (data or None), int(status.value)
