"""The host code that the PNG, pngquant, WebP and GIF device coders share around their kernels (csrc/encode_handoff.hpp, the
member of csrc/abi_shim.cpp that writes one coded frame, and codecs/_file_encoder.py): the opening checks of
ifhip_*_batch_device and the refusals of the host-buffer drop-in ifhip_* answer every coder in the same words and in the same
order -- the texts are written out below -- and, on a GPU, one batch gives the CPU emulation's bytes on the default stream, on
a side stream and into buffers the caller supplies, the drop-in gives the batch's file, and a job per preset writes it too."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra  # noqa: E402
from imageflow_amd.codecs import gif_encoder, libpng_encoder, pngquant, webp_encoder  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import gif_encode_emu as G  # noqa: E402
from tests import png_quantize_emu as Q  # noqa: E402
from tests import webp_emulation as WE  # noqa: E402

INVALID = int(ErrorKind.InvalidArgument)
NO_GPU = (int(ErrorKind.GpuUnavailable), int(ErrorKind.GpuError))
DEV = "cuda:0"
CODERS = ["png", "pngquant", "webp", "gif"]
W, H = 37, 23
STRIDE = 4 * W + 8
P_IN, P_OUT, P_LEN = 0x7F0000000000, 0x7F0000100000, 0x7F0000200000      # made up, 16-byte aligned, never dereferenced


class Coder:
    """one coder's module and entry points: batch(...) and host(...) take what the four have in common, `own` switches on the
    coder's first own refusal (its text: own_text)"""
    def __init__(self, name):
        self.name = name
        self.mod = {"png": libpng_encoder, "pngquant": pngquant, "webp": webp_encoder, "gif": gif_encoder}[name]
        self.L = self.mod._bind()
        stage = {"png": "png_enc", "pngquant": "png_quant", "webp": "webp_enc", "gif": "gif_enc"}[name]
        self.create_fn = getattr(self.L, "ifhip_%s_stage_create" % stage)
        self.destroy_fn = getattr(self.L, "ifhip_%s_stage_destroy" % stage)
        self.bound_fn = getattr(self.L, "ifhip_%s_stage_max_file_bytes" % stage)
        self.batch_fn = getattr(self.L, {"png": "ifhip_png_encode_batch_device", "pngquant": "ifhip_png_quantize_batch_device",
                                         "webp": "ifhip_webp_encode_batch_device", "gif": "ifhip_gif_encode_batch_device"}[name])
        self.host_fn = getattr(self.L, {"png": "ifhip_png_encode", "pngquant": "ifhip_png_quantize", "webp": "ifhip_webp_encode", "gif": "ifhip_gif_encode"}[name])
        self.own_text = {"png": b"InvalidArgument: zlib_level is -1 or 0..9", "pngquant": b"InvalidArgument: max_colors is 2..256",
                         "webp": b"InvalidArgument: d_files must be 4-byte aligned", "gif": b"InvalidArgument: repeat is -1 (none) or 0..65535"}[name]

    def stage(self, max_images=1):
        h = C.c_void_p()
        args = {"png": (W, H, libpng_encoder.PNG_RGBA, max_images), "webp": (W, H, 1, max_images)}.get(self.name, (W, H, max_images))
        assert self.create_fn(C.byref(h), *args) == 0                  # (geometry only: the scratch comes with the first batch)
        return h

    def batch(self, stage, images=P_IN, image_bytes=H * STRIDE, stride=STRIDE, n=1, files=P_OUT, lengths=P_LEN, own=False):
        pitch = (self.bound_fn(stage) + 15) // 16 * 16 if stage else 1 << 20
        if self.name == "png":
            rc = self.batch_fn(stage, images, image_bytes, stride, n, 10 if own else 6, files, pitch, lengths, None, None)
        elif self.name == "pngquant":
            rc = self.batch_fn(stage, images, image_bytes, stride, 1, n, -1, -1, -1, 1 if own else 256, 1, 6, files, pitch, lengths, None, None, None, None, None)
        elif self.name == "webp":
            rc = self.batch_fn(stage, images, image_bytes, stride, n, files + 2 if own and files else files, pitch, lengths, None, None)
        else:
            rc = self.batch_fn(stage, images, image_bytes, stride, 1, n, -2 if own else -1, 0, 0, files, pitch, lengths, None, None, None, None)
        return rc, self.L.ifhip_last_error_message()

    def host(self, bitmap=True, w=W, h=H, stride=STRIDE, length=True, status=None):
        frame, out, n = (C.c_uint8 * (H * STRIDE))(), (C.c_uint8 * 16)(), C.c_size_t(0)
        head = (frame if bitmap else None, w, h, stride)
        tail = (out, 16, C.byref(n) if length else None)
        if self.name == "png":
            rc = self.host_fn(*head, libpng_encoder.PNG_RGBA, 6, *tail)
        elif self.name == "pngquant":
            rc = self.host_fn(*head, 1, -1, -1, -1, *tail, C.byref(status) if status is not None else None)
        elif self.name == "webp":
            rc = self.host_fn(*head, 1, *tail)
        else:
            rc = self.host_fn(*head, 1, -1, 0, 0, *tail)
        return rc, self.L.ifhip_last_error_message()


def refusals(c):
    """case -> ((status code, message), the text the parent commit's source gives for it); each case breaks the named check
    and, where it says so, one that comes later as well: the earlier check answers"""
    s = c.stage()
    short = (H - 1) * STRIDE + 4 * W - 4                               # one row short by four bytes: still a multiple of 4
    misaligned = b"InvalidArgument: image rows must be 4-byte aligned and stride >= 4*w"
    told = {
        "batch: a null stage, of no images": (c.batch(None, n=0), b"InvalidArgument: null stage"),
        "batch: 2 images in a stage of 1, null images": (c.batch(s, n=2, images=None), b"InvalidArgument: 2 images exceed the stage capacity 1"),
        "batch: null images, null files": (c.batch(s, images=None, files=None), b"InvalidArgument: null image pointer"),
        "batch: stride 4*w - 4": (c.batch(s, stride=4 * W - 4), misaligned),
        "batch: stride + 2": (c.batch(s, stride=STRIDE + 2), misaligned),
        "batch: image_bytes + 2": (c.batch(s, image_bytes=H * STRIDE + 2), misaligned),
        "batch: images + 2": (c.batch(s, images=P_IN + 2), misaligned),
        "batch: one row short, null lengths": (c.batch(s, image_bytes=short, lengths=None),
                                               b"InvalidArgument: image_bytes %d is smaller than %d rows of stride %d" % (short, H, STRIDE)),
        "batch: null files, the coder's own": (c.batch(s, files=None, own=True), b"InvalidArgument: null pointer"),
        "batch: null lengths, the coder's own": (c.batch(s, lengths=None, own=True), b"InvalidArgument: null pointer"),
        "host: a null length, no dimensions": (c.host(length=False, w=0), b"InvalidArgument: null length out-pointer"),
        "host: width 0, a null bitmap": (c.host(w=0, bitmap=False), b"InvalidArgument: Bitmap dimensions cannot be zero"),
        "host: height 0": (c.host(h=0), b"InvalidArgument: Bitmap dimensions cannot be zero"),
        "host: a null bitmap, stride + 2": (c.host(bitmap=False, stride=STRIDE + 2), b"InvalidArgument: null bitmap pointer"),
        "host: stride 4*w - 4": (c.host(stride=4 * W - 4), b"InvalidArgument: stride smaller than a BGRA row or not a multiple of 4"),
        "host: stride + 2": (c.host(stride=STRIDE + 2), b"InvalidArgument: stride smaller than a BGRA row or not a multiple of 4"),
    }
    c.destroy_fn(s)
    return told


@pytest.mark.parametrize("name", CODERS)
def test_every_refused_argument_is_invalid_argument_in_the_words_of_the_source(name):
    for case, ((rc, message), want) in refusals(Coder(name)).items():
        assert rc == INVALID, (name, case, rc)
        assert message == want, (name, case, message)


def test_the_four_coders_refuse_in_the_same_words():
    told = {name: refusals(Coder(name)) for name in CODERS}
    for case in told["png"]:
        texts = {told[name][case][0][1] for name in CODERS}
        assert len(texts) == 1, (case, texts)


@pytest.mark.parametrize("name", CODERS)
def test_an_empty_batch_is_ok_and_the_coders_own_checks_follow_the_common_ones(name):
    c = Coder(name)
    s = c.stage()
    assert c.batch(s, n=0, images=None, files=None, lengths=None, own=True)[0] == 0, "an empty batch is answered before its pointers are looked at"
    assert c.batch(s, own=True) == (INVALID, c.own_text)
    if not torch.cuda.is_available():                                  # (with a GPU the made-up pointers must not reach a kernel)
        assert c.batch(s)[0] in NO_GPU, "a well-formed call reaches the device check"
    c.destroy_fn(s)


@pytest.mark.parametrize("name", CODERS)
def test_the_drop_in_refuses_before_the_device_is_asked_for(name):
    """Every refusal of refusals() is InvalidArgument with or without a GPU; without one, a well-formed call is the first to
    be told so, with one it is coded.  The palette coder's status word is cleared once the length's pointer is known to be there."""
    c = Coder(name)
    if not torch.cuda.is_available():
        assert c.host()[0] in NO_GPU
    else:                                                              # (a real bitmap: the file is coded and does not fit 16 bytes)
        rc, message = c.host()
        assert rc == INVALID and message.startswith(b"InvalidArgument: the file needs ") and message.endswith(b" bytes, the buffer has 16"), message
    if name == "pngquant":
        word = C.c_uint32(77)
        assert c.host(length=False, status=word)[0] == INVALID and word.value == 77
        assert c.host(w=0, status=word)[0] == INVALID and word.value == 0


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------
def frames_of(w, h):
    """RGBA frames [h, w, 4] of one geometry: a photo with alpha and noise (which no palette of 256 colours reaches exactly)"""
    return [Q.photo_rgba(w, h, seed=31, alpha=True), np.random.default_rng(32).integers(0, 256, (h, w, 4), dtype=np.uint8)]


def emulated(name, rgba, stride):
    """the file of the CPU emulation that the coder's own GPU test compares with"""
    if name == "png":
        from tests.test_gpu_png_device_bytes import emulated_file
        return emulated_file(rgba, 6)[0]
    if name == "pngquant":
        return Q.quantize(rgba, alpha=True, stride=stride)["file"]
    if name == "webp":
        return WE.encode(np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]), True)[0]
    return G.encode(rgba, alpha=True, stride=stride)["file"]


def new_stage(name, w, h, n):
    if name == "png":
        return libpng_encoder.PngEncodeStage(w, h, libpng_encoder.PNG_RGBA, n, DEV)
    if name == "pngquant":
        return pngquant.PngQuantStage(w, h, n, DEV)
    if name == "webp":
        return webp_encoder.WebpEncodeStage(w, h, True, n, DEV)
    return gif_encoder.GifEncodeStage(w, h, n, DEV)


def batch(name, stage, frames, supplied=None):
    """(files, lengths, status) as cuda tensors; supplied: the caller's three buffers, for the front ends that take them"""
    if name == "png":
        return stage.encode_device(frames, 6, None, *(supplied or ()))
    if name == "webp":
        return stage.encode_device(frames, None, *(supplied or ()))
    assert supplied is None
    if name == "pngquant":
        out = stage.quantize_device(frames)
        return out["files"], out["lengths"], out["status"]
    return stage.encode_device(frames)[:3]


def downloaded(files, lengths, status, n):
    files, lengths, status = files.cpu().numpy(), lengths.cpu().numpy(), status.cpu().numpy()
    return [files[i, :int(lengths[i])].tobytes() for i in range(n)], [int(s) for s in status[:n]]


def host_file(name, rows, w, h, stride):
    if name == "png":
        return libpng_encoder.encode_png_host(rows, w, h, stride, libpng_encoder.PNG_RGBA)
    if name == "pngquant":
        data, word = pngquant.quantize_png_host(rows, w, h, stride, True)
        assert word == 0
        return data
    if name == "webp":
        return webp_encoder.encode_webp_host(rows, w, h, stride, True)
    return gif_encoder.encode_gif_host(rows, w, h, stride, True)


def job_file(rows, w, h, preset, mime, ext):
    with Context() as c:
        assert c.set_gif_encoder(True) is True
        c.add_input_buffer(0, pack_raw_bgra(np.ascontiguousarray(rows[:, :4 * w]), w, h, alpha_meaningful=True))
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": preset}}]}})
        assert status == 200, (status, r, c.error_message())
        enc = r["data"]["job_result"]["encodes"][0]
        assert (enc["preferred_mime_type"], enc["preferred_extension"], enc["w"], enc["h"]) == (mime, ext, w, h)
        return bytes(c.get_output_buffer(1))


GEOMETRIES = {"png": [(W, H, STRIDE), (1, 1, 4)], "pngquant": [(W, H, STRIDE), (1, 1, 4)], "webp": [(W, H, STRIDE), (1, 1, 4)],
              "gif": [(W, H, STRIDE), (1, 1, 4), (129, 128, 4 * 129)]}     # 129 x 128: a second LZW segment (16384 pixels a segment)
_FILES = {}


def batch_files(name, w, h, stride):
    """The files of the geometry's two frames by the batch path, the same on the default stream, on a side stream and, where
    the front end takes them, in the caller's buffers; each equal to the emulation's.  Computed once per coder and geometry."""
    key = (name, w, h)
    if key in _FILES:
        return _FILES[key]
    rgba = frames_of(w, h) if (w, h) != (129, 128) else frames_of(w, h)[:1]
    n = len(rgba)
    rows = np.stack([Q.bgra_rows(f, stride) for f in rgba])
    frames = Bitmap.from_numpy(np.ascontiguousarray(rows), w, h, stride, DEV, alpha_meaningful=True)
    stage = new_stage(name, w, h, n)
    runs = [downloaded(*batch(name, stage, frames), n)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = batch(name, stage, frames)
    side.synchronize()
    runs.append(downloaded(*on_side, n))
    if name in ("png", "webp"):
        pitch = (stage.max_file_bytes + 15) // 16 * 16 + 32
        own = (torch.full((n, pitch), 0x5C, dtype=torch.uint8, device=DEV), torch.full((n + 3,), -7, dtype=torch.int32, device=DEV),
               torch.full((n + 3,), -9, dtype=torch.int32, device=DEV))
        got = batch(name, stage, frames, own)
        torch.cuda.synchronize()
        assert all(a is b for a, b in zip(got, own)), "the caller's buffers come back"
        assert own[1][n:].cpu().tolist() == [-7] * 3 and own[2][n:].cpu().tolist() == [-9] * 3
        runs.append(downloaded(*own, n))
    for k, (files, status) in enumerate(runs):
        assert status == [0] * n, (name, k, status)
        assert files == runs[0][0], (name, k, "the same bytes on every run")
    for i in range(n):
        assert runs[0][0][i] == emulated(name, rgba[i], stride), (name, w, h, i, "the emulation's file")
    _FILES[key] = (rows, runs[0][0])
    return _FILES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CODERS)
def test_one_batch_on_the_default_stream_a_side_stream_and_into_supplied_buffers(name):
    """The side-stream run is a smoke test: it shows that the hand-off is ordered on the caller's stream and does not deadlock;
    it does not prove the absence of a race.  tests/test_gpu_stream_order.py does, for every coder: the frames arrive late on
    a stream that is held up on purpose, and a launch that left that stream would code the decoy."""
    for w, h, stride in GEOMETRIES[name]:
        rows, files = batch_files(name, w, h, stride)
        assert all(files), (name, w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CODERS)
def test_the_drop_in_returns_the_batchs_file(name):
    for w, h, stride in GEOMETRIES[name]:
        rows, files = batch_files(name, w, h, stride)
        assert host_file(name, rows[0], w, h, stride) == files[0], (name, w, h)


PRESETS = {"libpng": ("png", 0, {"libpng": {}}, "image/png", "png"), "pngquant": ("pngquant", 0, {"pngquant": {}}, "image/png", "png"),
           "pngquant below minimum_quality": ("png", 1, {"pngquant": {"minimum_quality": 100}}, "image/png", "png"),      # noise: the lossless file
           "webplossless": ("webp", 0, "webplossless", "image/webp", "webp"), "gif": ("gif", 0, "gif", "image/gif", "gif")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(PRESETS))
def test_a_job_writes_the_batchs_file(case):
    name, i, preset, mime, ext = PRESETS[case]
    rows, files = batch_files(name, W, H, STRIDE)
    assert job_file(rows[i], W, H, preset, mime, ext) == files[i], case
