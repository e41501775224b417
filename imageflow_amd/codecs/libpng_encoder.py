"""Host mirror of LibPngEncoder (imageflow_core/src/codecs/libpng_encoder.rs:43-72,134-160 over
c_components/lib/codec_png_wrapper.c:349-430) on the device PNG coder of libimageflow_hip.so (csrc/png_encode.hip): BGRA /
BGRX frames that stay in HBM -> complete PNG files in HBM -- row filters with libpng's default choice, deflate, the chunks
and their CRCs.  For tests and tools; the job path is the `libpng` preset of `encode` (csrc/shim_encode.cpp)."""
import ctypes as C

from .. import _native
from ..graphics.bitmaps import Bitmap
from ._file_encoder import FileEncodeStage, encode_host, files_as_bytes

PNG_RGB, PNG_RGBA = 2, 6                # include/imageflow_hip.h IFHIP_PNG_*
PNG_FILE_OVERFLOW = 1
DEFAULT_ZLIB_LEVEL = 6                  # codecs/auto.rs:265 -> codec_png_wrapper.c:380-387: absent means zlib's default


def _bind():
    L = _native.lib()
    if getattr(L, "_png_enc_bound", False):
        return L
    L.ifhip_png_enc_stage_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
    L.ifhip_png_enc_stage_destroy.argtypes = [C.c_void_p]
    L.ifhip_png_enc_stage_destroy.restype = None
    L.ifhip_png_enc_stage_max_file_bytes.argtypes = [C.c_void_p]
    L.ifhip_png_enc_stage_max_file_bytes.restype = C.c_size_t
    L.ifhip_png_encode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_png_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L._png_enc_bound = True
    return L


class PngEncodeStage(FileEncodeStage):
    """ifhip_png_enc_stage: one geometry and colour type, the scratch of a batch in flight (one stream at a time)."""

    def __init__(self, width, height, color_type=PNG_RGBA, max_images=1, device="cuda:0"):
        self.width, self.height, self.color_type, self.max_images = width, height, color_type, max_images
        self._create(_bind(), "ifhip_png_enc_stage", device, width, height, color_type, max_images)

    def encode_device(self, frames: Bitmap, zlib_level=DEFAULT_ZLIB_LEVEL, file_pitch=None, files=None, lengths=None, status=None):
        """frames: n BGRA frames of the stage's geometry.  Returns (files [n, file_pitch] uint8, lengths [n] int32, status [n]
        int32), all cuda tensors; nothing is synchronised."""
        return self._batch(frames.n, lambda d_files, pitch, d_lengths, d_status: (
            _bind().ifhip_png_encode_batch_device, self._h, frames.data.data_ptr(), frames.image_bytes, frames.stride, frames.n, int(zlib_level), d_files, pitch,
            d_lengths, d_status), file_pitch, files, lengths, status)

    def encode(self, frames: Bitmap, zlib_level=DEFAULT_ZLIB_LEVEL, file_pitch=None):
        """The n files as bytes (None for a file that did not fit file_pitch) and the status words."""
        return files_as_bytes(*self.encode_device(frames, zlib_level, file_pitch))


def color_type_for(alpha_meaningful, depth=None):
    """codec_png_wrapper.c:402-410: RGB when the frame's alpha is not meaningful or depth is png_24, else RGBA."""
    if depth not in (None, "png_32", "png_24"):
        raise ValueError(f"unknown PNG depth {depth!r}")
    return PNG_RGB if (not alpha_meaningful or depth == "png_24") else PNG_RGBA


def encode_png(bitmap: Bitmap, depth=None, zlib_compression=None, matte=None):
    """LibPngEncoder::write_frame on every frame of the bitmap: the matte only when given (libpng_encoder.rs:55-57; an
    opaque one clears alpha_meaningful), the colour type from alpha_meaningful and depth, zlib_compression as the reference
    clamps it (auto.rs:265: 0..255; above 9 -> the default).  Returns the files."""
    if matte is not None:
        from ..graphics.blend import apply_matte
        apply_matte(bitmap, matte)
        if (matte >> 24) == 0xFF:
            bitmap.alpha_meaningful = False
    level = DEFAULT_ZLIB_LEVEL if zlib_compression is None else min(255, max(0, int(zlib_compression)))
    if level > 9:
        level = -1
    stage = PngEncodeStage(bitmap.w, bitmap.h, color_type_for(bitmap.alpha_meaningful, depth), bitmap.n, bitmap.data.device)
    files, status = stage.encode(bitmap, level)
    if any(status):                                                       # (cannot happen with the stage's own pitch)
        raise RuntimeError(f"device PNG coder dropped images: status {status}")
    return files


def encode_png_host(bgra, width, height, stride, color_type=PNG_RGBA, zlib_level=DEFAULT_ZLIB_LEVEL):
    """Host-buffer drop-in (numpy): BGRA rows -> the file's bytes."""
    L = _bind()
    return encode_host(L, "ifhip_png_enc_stage", (width, height, color_type, 1), L.ifhip_png_encode, bgra, width, height, stride, (color_type, int(zlib_level)))
