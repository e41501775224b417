"""Host mirror of the lossy half of WebPEncoder (imageflow_core/src/codecs/webp.rs over libwebp's WebPEncodeBGRA / WebPEncodeBGR,
EncoderPreset::WebPLossy) on the device lossy WebP coder of libimageflow_hip.so (csrc/vp8_encode.hip): BGRA / BGRX frames that
stay in HBM -> complete lossy WebP files (`VP8 `, with `VP8X` + `ALPH` for a frame with alpha) in HBM.  For tests and tools; the
job path is the `webplossy` preset of `encode` behind Context.set_webp_lossy_encoder (csrc/shim_encode.cpp)."""
import ctypes as C

from .. import _native
from ..graphics.bitmaps import Bitmap
from ._file_encoder import FileEncodeStage, encode_host, files_as_bytes

VP8_ENC_INTRA4 = 1                      # include/imageflow_hip_webp_lossy_enc.h IFHIP_VP8_ENC_INTRA4: stage flag, the sixteen 4x4 luma modes
VP8_ENC_FILE_OVERFLOW = 1               # include/imageflow_hip_webp_lossy_enc.h IFHIP_VP8_ENC_FILE_OVERFLOW
MAX_DIMENSION = 16383                   # 14 bits of width and height


def _bind():
    L = _native.lib()
    if getattr(L, "_webp_lossy_enc_bound", False):
        return L
    L.ifhip_webp_lossy_enc_stage_create.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
    L.ifhip_webp_lossy_enc_stage_create_flags.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32]
    L.ifhip_webp_lossy_enc_stage_destroy.argtypes = [C.c_void_p]
    L.ifhip_webp_lossy_enc_stage_destroy.restype = None
    L.ifhip_webp_lossy_enc_stage_max_file_bytes.argtypes = [C.c_void_p]
    L.ifhip_webp_lossy_enc_stage_max_file_bytes.restype = C.c_size_t
    L.ifhip_webp_lossy_encode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_size_t,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_webp_lossy_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ifhip_webp_lossy_encode_flags.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_size_t,
                                                C.POINTER(C.c_size_t)]
    L._webp_lossy_enc_bound = True
    return L


class _WithFlags:
    """the stage functions as FileEncodeStage._create and encode_host name them, the create being the one that takes flags"""

    def __init__(self, L):
        self.ifhip_webp_lossy_enc_stage_create = L.ifhip_webp_lossy_enc_stage_create_flags
        self.ifhip_webp_lossy_enc_stage_destroy = L.ifhip_webp_lossy_enc_stage_destroy
        self.ifhip_webp_lossy_enc_stage_max_file_bytes = L.ifhip_webp_lossy_enc_stage_max_file_bytes


class WebpLossyEncodeStage(FileEncodeStage):
    """ifhip_webp_lossy_enc_stage: one geometry and alpha mode, the scratch of a batch in flight (one stream at a time).
    intra4: IFHIP_VP8_ENC_INTRA4, macroblocks may take the sixteen 4x4 luma modes."""

    def __init__(self, width, height, alpha_meaningful=True, max_images=1, device="cuda:0", intra4=False):
        self.width, self.height, self.alpha_meaningful, self.max_images, self.intra4 = width, height, bool(alpha_meaningful), max_images, bool(intra4)
        self._create(_WithFlags(_bind()), "ifhip_webp_lossy_enc_stage", device, width, height, 1 if alpha_meaningful else 0, max_images, VP8_ENC_INTRA4 if intra4 else 0)

    def encode_device(self, frames: Bitmap, quality, file_pitch=None, files=None, lengths=None, status=None):
        """frames: n BGRA frames of the stage's geometry.  Returns (files [n, file_pitch] uint8, lengths [n] int32, status [n]
        int32), all cuda tensors; nothing is synchronised."""
        return self._batch(frames.n, lambda d_files, pitch, d_lengths, d_status: (
            _bind().ifhip_webp_lossy_encode_batch_device, self._h, frames.data.data_ptr(), frames.image_bytes, frames.stride, frames.n, float(quality), d_files,
            pitch, d_lengths, d_status), file_pitch, files, lengths, status)

    def encode(self, frames: Bitmap, quality, file_pitch=None):
        """The n files as bytes (None for a file that did not fit file_pitch) and the status words."""
        return files_as_bytes(*self.encode_device(frames, quality, file_pitch))


def encode_webp_lossy(bitmap: Bitmap, quality, intra4=False):
    """WebPEncoder::write_frame for EncoderPreset::WebPLossy on every frame of the bitmap: BGRA when the frame's alpha is
    meaningful, else BGR; no matte.  Returns the files."""
    stage = WebpLossyEncodeStage(bitmap.w, bitmap.h, bitmap.alpha_meaningful, bitmap.n, bitmap.data.device, intra4=intra4)
    files, status = stage.encode(bitmap, quality)
    if any(status):                                                       # (the first partition of a very large frame: see the header)
        raise RuntimeError(f"device lossy WebP coder dropped images: status {status}")
    return files


def encode_webp_lossy_host(bgra, width, height, stride, quality, alpha_meaningful=True, intra4=False):
    """Host-buffer drop-in (numpy): BGRA rows -> the file's bytes."""
    L = _bind()
    alpha = 1 if alpha_meaningful else 0
    flags = VP8_ENC_INTRA4 if intra4 else 0
    return encode_host(_WithFlags(L), "ifhip_webp_lossy_enc_stage", (width, height, alpha, 1, flags), L.ifhip_webp_lossy_encode_flags, bgra, width, height, stride,
                       (alpha, C.c_float(float(quality)), flags))
