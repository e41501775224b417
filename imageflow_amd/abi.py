"""ctypes binding of the libimageflow C-ABI subset that libimageflow_hip.so re-exports (include/imageflow_abi_subset.h,
csrc/abi_shim.cpp) -- written the way a language binding over bindings/headers/imageflow_default.h is written:
create a context, add buffers, send a JSON job, read the response, fetch the outputs.  Host logic only."""
import ctypes as C
import json
import struct

import numpy as np

from . import _native

ABI_MAJOR, ABI_MINOR = 3, 2
RAW_MAGIC = b"IFBGRA1\x00"


def _bind():
    L = _native.lib()
    if getattr(L, "_abi_bound", False):
        return L
    vp, u8pp, szp = C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)
    L.imageflow_abi_compatible.argtypes = [C.c_uint32, C.c_uint32]
    L.imageflow_abi_compatible.restype = C.c_bool
    L.imageflow_abi_version_major.restype = C.c_uint32
    L.imageflow_abi_version_minor.restype = C.c_uint32
    L.imageflow_context_create.argtypes = [C.c_uint32, C.c_uint32]
    L.imageflow_context_create.restype = vp
    L.imageflow_context_destroy.argtypes = [vp]
    L.imageflow_context_destroy.restype = None
    for name in ("has_error", "error_recoverable", "error_try_clear", "begin_terminate"):
        f = getattr(L, "imageflow_context_" + name)
        f.argtypes, f.restype = [vp], C.c_bool
    for name in ("error_code", "error_as_exit_code", "error_as_http_code"):
        f = getattr(L, "imageflow_context_" + name)
        f.argtypes, f.restype = [vp], C.c_int32
    L.imageflow_context_error_write_to_buffer.argtypes = [vp, C.c_char_p, C.c_size_t, szp]
    L.imageflow_context_error_write_to_buffer.restype = C.c_bool
    L.imageflow_context_send_json.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t]
    L.imageflow_context_send_json.restype = vp
    L.imageflow_json_response_read.argtypes = [vp, vp, C.POINTER(C.c_int64), u8pp, szp]
    L.imageflow_json_response_read.restype = C.c_bool
    L.imageflow_json_response_destroy.argtypes = [vp, vp]
    L.imageflow_json_response_destroy.restype = C.c_bool
    L.imageflow_context_add_input_buffer.argtypes = [vp, C.c_int32, C.c_char_p, C.c_size_t, C.c_int]
    L.imageflow_context_add_input_buffer.restype = C.c_bool
    L.imageflow_context_add_output_buffer.argtypes = [vp, C.c_int32]
    L.imageflow_context_add_output_buffer.restype = C.c_bool
    L.imageflow_context_get_output_buffer_by_id.argtypes = [vp, C.c_int32, u8pp, szp]
    L.imageflow_context_get_output_buffer_by_id.restype = C.c_bool
    L.imageflow_context_take_output_buffer.argtypes = [vp, C.c_int32, u8pp, szp]
    L.imageflow_context_take_output_buffer.restype = C.c_bool
    L.imageflow_buffer_free.argtypes = [C.POINTER(C.c_uint8), C.c_size_t]
    L.imageflow_buffer_free.restype = C.c_bool
    L.imageflow_context_request_cancellation.argtypes = [vp]
    L.imageflow_context_request_cancellation.restype = None
    L.imageflow_context_print_and_exit_if_error.argtypes = [vp]
    L.imageflow_context_print_and_exit_if_error.restype = C.c_bool
    L.ifhip_shim_request_cancellation_after_n_polls.argtypes = [vp, C.c_int64]
    L.ifhip_shim_request_cancellation_after_n_polls.restype = None
    L.ifhip_shim_cancellation_polls_remaining.argtypes = [vp]
    L.ifhip_shim_cancellation_polls_remaining.restype = C.c_int64
    L.ifhip_shim_fused_decode_resamples.argtypes = [vp]
    L.ifhip_shim_fused_decode_resamples.restype = C.c_int64
    L.ifhip_shim_device_coded_files.argtypes = [vp]
    L.ifhip_shim_device_coded_files.restype = C.c_int64
    L.ifhip_shim_coalesced_decodes.argtypes = [vp]
    L.ifhip_shim_coalesced_decodes.restype = C.c_int64
    L.ifhip_shim_spread_contexts.argtypes = [C.c_int]
    L.ifhip_shim_spread_contexts.restype = None
    L.ifhip_shim_context_set_device.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_device.restype = C.c_bool
    L.ifhip_shim_context_device.argtypes = [vp]
    L.ifhip_shim_context_device.restype = C.c_int
    L.ifhip_shim_context_set_color_management.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_color_management.restype = C.c_bool
    L.ifhip_shim_context_set_color_profile_kinds.argtypes = [vp, C.c_uint32]
    L.ifhip_shim_context_set_color_profile_kinds.restype = C.c_bool
    L.ifhip_shim_color_links_built.argtypes = [vp]
    L.ifhip_shim_color_links_built.restype = C.c_int64
    L.ifhip_shim_context_set_webp_lossy_decoder.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_webp_lossy_decoder.restype = C.c_bool
    L.ifhip_shim_context_set_device_progressive_decoder.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_device_progressive_decoder.restype = C.c_bool
    L.ifhip_shim_device_progressive_decodes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.ifhip_shim_device_progressive_decodes.restype = C.c_int64
    L.ifhip_shim_context_set_webp_lossy_encoder.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_webp_lossy_encoder.restype = C.c_bool
    L.ifhip_shim_context_set_webp_lossless_flags.argtypes = [vp, C.c_uint32]
    L.ifhip_shim_context_set_webp_lossless_flags.restype = C.c_bool
    L.ifhip_shim_context_set_gif_encoder.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_gif_encoder.restype = C.c_bool
    L.ifhip_shim_context_set_gif_animation.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_gif_animation.restype = C.c_bool
    L.ifhip_shim_context_set_device_jpeg_options.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_device_jpeg_options.restype = C.c_bool
    L.ifhip_shim_context_set_encoder_selection.argtypes = [vp, C.c_int]
    L.ifhip_shim_context_set_encoder_selection.restype = C.c_bool
    L.ifhip_shim_querystring_encoder_preset.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, szp]
    L.ifhip_shim_querystring_encoder_preset.restype = C.c_int
    L.ifhip_shim_resolve_encoder_preset.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p,
                                                    C.c_size_t, szp]
    L.ifhip_shim_resolve_encoder_preset.restype = C.c_int
    L.imageflow_context_memory_allocate.argtypes = [vp, C.c_size_t, C.c_char_p, C.c_int32]
    L.imageflow_context_memory_allocate.restype = vp
    L.imageflow_context_memory_free.argtypes = [vp, vp, C.c_char_p, C.c_int32]
    L.imageflow_context_memory_free.restype = C.c_bool
    L._abi_bound = True
    return L


def pack_raw_bgra(rows, w, h, alpha_meaningful=True):
    """EXTENSION container the shim's decode accepts: rows = uint8 [h][stride]."""
    rows = np.ascontiguousarray(rows, np.uint8)
    return RAW_MAGIC + struct.pack("<IIII", w, h, rows.shape[1], int(alpha_meaningful)) + rows.tobytes()


def unpack_raw_bgra(buf):
    """-> (uint8 [h][stride], w, h, alpha_meaningful)"""
    assert buf[:8] == RAW_MAGIC, buf[:8]
    w, h, stride, alpha = struct.unpack("<IIII", buf[8:24])
    return np.frombuffer(buf, np.uint8, h * stride, 24).reshape(h, stride), w, h, bool(alpha)


SELECT_REFUSED, SELECT_INVALID, SELECT_INVALID_JSON = 2, 3, 4        # include/imageflow_hip_encoder_select.h IFHIP_SELECT_*
SOURCE_KINDS = {None: 0, "raw": 0, "jpeg": 1, "png": 2, "gif": 3, "webp": 4}   # IFHIP_SELECT_SOURCE_*


class EncoderSelectError(ValueError):
    """A refusal of the two host-only entry points below: .status is IFHIP_SELECT_REFUSED (ActionNotSupported), _INVALID
    (InvalidArgument) or _INVALID_JSON (InvalidJson); the message is the library's."""

    def __init__(self, status, message):
        self.status = status
        super().__init__(message)


def _select_call(f, *args):
    L = _bind()
    needed = C.c_size_t()
    buf = C.create_string_buffer(4096)
    rc = f(*args, buf, len(buf), C.byref(needed))
    if rc == 0 and needed.value > len(buf):
        buf = C.create_string_buffer(needed.value)
        rc = f(*args, buf, len(buf), C.byref(needed))
    if rc != 0:
        raise EncoderSelectError(rc, (L.ifhip_last_error_message() or b"").decode("utf-8", "replace"))
    return json.loads(buf.value.decode())


def querystring_encoder_preset(value):
    """The EncoderPreset ({"auto": ..} or {"format": ..}) the reference's querystring layer makes of a querystring's output
    keys (ifhip_shim_querystring_encoder_preset; host only)."""
    return _select_call(_bind().ifhip_shim_querystring_encoder_preset, value.encode())


def resolve_encoder_preset(preset, source=None, source_lossless=False, source_frames=1, alpha_meaningful=False, w=1, h=1):
    """What an `auto` / `format` preset comes to for a source ("jpeg" | "png" | "gif" | "webp" | None) and a final frame:
    {"format", "coder", "params", "matte"} (ifhip_shim_resolve_encoder_preset; host only)."""
    body = preset if isinstance(preset, (bytes, bytearray)) else json.dumps(preset).encode()
    return _select_call(_bind().ifhip_shim_resolve_encoder_preset, body, len(body), SOURCE_KINDS[source], int(bool(source_lossless)), source_frames,
                        int(bool(alpha_meaningful)), w, h)


class Context:
    def __init__(self):
        self.L = _bind()
        self.p = self.L.imageflow_context_create(ABI_MAJOR, ABI_MINOR)
        if not self.p:
            raise RuntimeError("imageflow_context_create failed")
        self._keep = []

    def close(self):
        if self.p:
            self.L.imageflow_context_destroy(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def add_input_buffer(self, io_id, data: bytes, outlives_context=True):
        self._keep.append(data)
        return self.L.imageflow_context_add_input_buffer(self.p, io_id, data, len(data), 1 if outlives_context else 0)

    def add_output_buffer(self, io_id):
        return self.L.imageflow_context_add_output_buffer(self.p, io_id)

    def send_json(self, method, message):
        """-> (http status, parsed response or None)"""
        body = message if isinstance(message, (bytes, bytearray)) else json.dumps(message).encode()
        r = self.L.imageflow_context_send_json(self.p, method.encode(), body, len(body))
        if not r:
            return None, None
        status, buf, n = C.c_int64(), C.POINTER(C.c_uint8)(), C.c_size_t()
        assert self.L.imageflow_json_response_read(self.p, r, C.byref(status), C.byref(buf), C.byref(n))
        text = C.string_at(buf, n.value).decode()
        try:
            parsed = json.loads(text)
        except ValueError:
            parsed = text
        self.L.imageflow_json_response_destroy(self.p, r)
        return status.value, parsed

    def get_output_buffer(self, io_id):
        buf, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        if not self.L.imageflow_context_get_output_buffer_by_id(self.p, io_id, C.byref(buf), C.byref(n)):
            return None
        return C.string_at(buf, n.value)

    def take_output_buffer(self, io_id):
        """imageflow_context_take_output_buffer + imageflow_buffer_free: the bytes, owned by the caller; None on error."""
        buf, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        if not self.L.imageflow_context_take_output_buffer(self.p, io_id, C.byref(buf), C.byref(n)):
            return None
        data = C.string_at(buf, n.value)
        assert self.L.imageflow_buffer_free(buf, n.value)
        return data

    def set_device(self, ordinal):
        """Bind the context's jobs to a device ordinal (-1: the calling thread's current device); False + a context error otherwise."""
        return self.L.ifhip_shim_context_set_device(self.p, ordinal)

    def set_color_management(self, on):
        """EXTENSION, off by default: convert every input whose ICC profile or PNG gAMA + cHRM is not sRGB to sRGB on the device
        behind its decode, instead of refusing the job (the decoder command "convert_color_profile" does it for one input;
        "discard_color_profile" wins over both)."""
        return self.L.ifhip_shim_context_set_color_management(self.p, 1 if on else 0)

    def set_color_profile_kinds(self, gray=False, lut=False):
        """EXTENSION, both off by default: where colour management acts, also convert grey frames with a GRAY profile (`gray`) and
        frames with a LUT-based RGB profile (`lut`, A2B0) through a colour link, instead of refusing them."""
        return self.L.ifhip_shim_context_set_color_profile_kinds(self.p, (1 if gray else 0) | (2 if lut else 0))

    def color_links_built(self):
        """Diagnostic: colour links this context's jobs built from profile bytes (a profile met again comes from the cache)."""
        return self.L.ifhip_shim_color_links_built(self.p)

    def set_webp_lossy_decoder(self, on):
        """EXTENSION, off by default: lossy WebP inputs (`VP8 `, with or without `ALPH`) are decoded on the device to exactly
        libwebp's pixels -- `decode`, `watermark`, `command_string` and v1/get_image_info take them -- instead of being
        ImageTypeNotSupported."""
        return self.L.ifhip_shim_context_set_webp_lossy_decoder(self.p, 1 if on else 0)

    def set_device_progressive_decoder(self, on):
        """EXTENSION, off by default: progressive JPEG inputs are entropy-decoded on the device; a file its front end refuses,
        or one whose status word is not 0, goes to the host reader as ever.  Outputs are the same bytes either way."""
        return self.L.ifhip_shim_context_set_device_progressive_decoder(self.p, 1 if on else 0)

    def device_progressive_decodes(self):
        """-> (decodes of this context that took the device path, decodes that fell back to the host reader)"""
        back = C.c_int64()
        return int(self.L.ifhip_shim_device_progressive_decodes(self.p, C.byref(back))), int(back.value)

    def set_webp_lossy_encoder(self, on, intra4=False):
        """EXTENSION, off by default: `encode` with the preset {"webplossy": {"quality": q}} writes a lossy WebP file on the device
        (image/webp) instead of the raw BGRA container; the bare string and a missing or non-numeric quality are then InvalidJson."""
        return self.L.ifhip_shim_context_set_webp_lossy_encoder(self.p, (2 if intra4 else 1) if on else 0)

    def set_webp_lossless_flags(self, color_indexing=False):
        """EXTENSION, all off by default: the stage flags of the "webplossless" preset's coder.  color_indexing
        (IFHIP_WEBP_ENC_COLOR_INDEXING): frames of at most 256 colours are written with a colour table where that is smaller."""
        return self.L.ifhip_shim_context_set_webp_lossless_flags(self.p, 1 if color_indexing else 0)

    def set_gif_encoder(self, on):
        """EXTENSION, off by default: `encode` with the preset "gif" writes a GIF89a file on the device (image/gif) instead of
        the raw BGRA container; a GIF input of the job hands on its loop count, delay and user-input flag."""
        return self.L.ifhip_shim_context_set_gif_encoder(self.p, 1 if on else 0)

    def set_gif_animation(self, on):
        """EXTENSION, off by default: with the GIF encoder on as well, a job whose `decode` reads a GIF of more than one frame
        (no select_frame told) and whose "gif" `encode` lies downstream runs once per frame and writes ONE animated GIF;
        every other encoder of the job takes frame 0.  Every other job is what it is with the switch off.  With encoder
        selection on, an `auto` / `format` encode that comes to GIF counts as a "gif" encode, GIF encoder switch or not."""
        return self.L.ifhip_shim_context_set_gif_animation(self.p, 1 if on else 0)

    def set_device_jpeg_options(self, on):
        """EXTENSION, off by default: entropy-code the libjpeg_turbo preset's progressive / optimize_huffman_coding files on the
        device instead of by the host writer (the same bytes; only the file leaves the device)."""
        return self.L.ifhip_shim_context_set_device_jpeg_options(self.p, 1 if on else 0)

    def set_encoder_selection(self, on):
        """EXTENSION, off by default: `encode` with the preset {"auto": ..} or {"format": ..} is resolved as the reference
        resolves it (format, coder and quality from its tables, against the job's first input and the final frame) and written
        as a real file -- JPEG, PNG, palette PNG, WebP or GIF -- instead of the raw BGRA container; `command_string` reads the
        output keys of its querystring (format, qp, qp.dpr, lossless, accept.*, quality, jpeg.*, webp.*, png.*) instead of
        refusing them, and a string without one keeps the source's format."""
        return self.L.ifhip_shim_context_set_encoder_selection(self.p, 1 if on else 0)

    @property
    def device(self):
        return self.L.ifhip_shim_context_device(self.p)

    def request_cancellation(self):
        self.L.imageflow_context_request_cancellation(self.p)

    def has_error(self):
        return self.L.imageflow_context_has_error(self.p)

    def error_code(self):
        return self.L.imageflow_context_error_code(self.p)

    def error_message(self, cap=2048):
        b = C.create_string_buffer(cap)
        n = C.c_size_t()
        whole = self.L.imageflow_context_error_write_to_buffer(self.p, b, cap, C.byref(n))
        return b.value.decode("utf-8", "replace"), whole
