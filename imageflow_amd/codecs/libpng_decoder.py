"""Host mirror of LibPngDecoder (imageflow_core/src/codecs/libpng_decoder.rs:36-104,297-299,340-383 over
c_components/lib/codec_png_wrapper.c:131-212,215-246,266-292) on the device PNG decoder of libimageflow_hip.so
(csrc/png_read.cpp, csrc/png_decode.hip): PNG files -> 8-bit BGRA frames in HBM -- inflate, un-filter, libpng's transforms
and the Adam7 scatter on the GPU.  For tests and tools; the job path is `decode` with a PNG io_id (csrc/shim_decode.cpp)."""
import ctypes as C

import numpy as np

from .. import _native
from ..errors import ErrorKind, FlowError
from ._file_decoder import decode_batch, decode_host

# include/imageflow_hip.h IFHIP_PNG_DEC_*
STATUS = {0: "ok", 1: "truncated", 2: "block_type", 3: "stored_length", 4: "code_lengths", 5: "bad_code", 6: "distance", 7: "zlib_header",
          8: "adler", 9: "too_little", 10: "filter", 11: "container"}
COLOR_NONE, COLOR_SRGB, COLOR_OTHER = 0, 1, 2


class PngFileInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "bit_depth", "color_type", "interlace", "alpha_used", "uses_palette")] + [("color_kind", C.c_int32)]


def _bind():
    L = _native.lib()
    if getattr(L, "_png_dec_bound", False):
        return L
    L.ifhip_png_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(PngFileInfo)]
    L.ifhip_png_decode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_png_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_size_t, C.POINTER(C.c_uint32)]
    L._png_dec_bound = True
    return L


def png_info(data):
    """get_unscaled_image_info (= get_scaled_image_info, libpng_decoder.rs:36-52) plus the file's own facts.  Host only."""
    L = _bind()
    buf = np.frombuffer(bytes(data), np.uint8)
    info = PngFileInfo()
    _native.check(L.ifhip_png_info(buf.ctypes.data, buf.size, C.byref(info)))
    out = {n: int(getattr(info, n)) for n, _ in PngFileInfo._fields_}
    out["alpha_used"], out["uses_palette"] = bool(out["alpha_used"]), bool(out["uses_palette"])
    out.update(preferred_mime_type="image/png", preferred_extension="png", image_width=out["width"], image_height=out["height"],
               frame_decodes_into="bgra_32" if out["alpha_used"] else "bgr_32", exif_rotation_flag=None)
    return out


def decode_png_batch(files, device="cuda:0", frames=None, fill=None):
    """files: n PNG files (bytes) of any geometry, type and depth, decoded in one batch (three launches).  Returns (frames,
    status): frames[i] a Bitmap of one frame (None where the file's chunks did not parse), status[i] the file's status word.
    frames: Bitmaps to decode into (their strides are honoured); fill: a byte the new frames are filled with first."""
    L = _bind()
    return decode_batch(L.ifhip_png_info, L.ifhip_png_decode_batch_device, PngFileInfo, lambda info: True, lambda info: bool(info.alpha_used),
                        files, device, frames, fill)


def decode_png(data, device="cuda:0"):
    """LibPngDecoder::read_frame: one file -> a Bitmap (alpha_meaningful = alpha_used).  A damaged stream raises ImageMalformed-style."""
    frames, status = decode_png_batch([data], device)
    if status[0]:
        raise FlowError(ErrorKind.InvalidArgument, f"ImageMalformed: LibPNG error: {STATUS.get(status[0], status[0])}")
    return frames[0]


def decode_png_host(data, stride=None, out=None):
    """Host-buffer drop-in (numpy): the file -> BGRA rows [h, stride] uint8."""
    L = _bind()
    return decode_host(L.ifhip_png_info, L.ifhip_png_decode, PngFileInfo, data, stride, out)
