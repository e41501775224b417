"""The host code that the PNG, WebP and GIF device decoders share around their kernels (csrc/decode_handoff.hpp and
codecs/_file_decoder.py): the argument checks of ifhip_*_decode_batch_device and of the host-buffer drop-in ifhip_*_decode
answer every decoder in the same words -- the texts are written out below, and only the numbers in them follow the fixture's
size -- and, on a GPU, one batch of two good files around one that does not parse gives the oracle's pixels and the same
status words on the default stream, on a side stream and into frames the caller supplies."""
import ctypes as C
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.codecs import gif_decoder, libpng_decoder, webp_decoder  # noqa: E402
from imageflow_amd.errors import ErrorKind  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap, get_stride  # noqa: E402
from tests import gif_fixtures as GX  # noqa: E402
from tests import gif_oracle as GO  # noqa: E402
from tests import png_decode_oracle as PO  # noqa: E402
from tests import webp_decode_fixtures as WX  # noqa: E402

INVALID = int(ErrorKind.InvalidArgument)
DEV = "cuda:0"
NOT_A_FILE = b"neither a PNG, a WebP nor a GIF"
DECODERS = ["png", "webp", "gif"]


def png_file(ct, depth, w, h):
    rng = np.random.default_rng(ct * 17 + depth)
    return PO.write_png(PO.random_samples(rng, w, h, ct, depth), ct, depth)


class Decoder:
    """one decoder's module, entry points, two smallest good fixtures with the oracle's BGRA, and its CONTAINER word"""
    def __init__(self, name):
        self.name = name
        if name == "png":
            self.mod, self.container, self.lead = libpng_decoder, 11, ()
            files = [png_file(2, 8, 37, 23), png_file(6, 8, 7, 5)]
            self.good = [(f, PO.decode(f)[0]) for f in files]
        elif name == "webp":
            self.mod, self.container, self.lead = webp_decoder, 9, ()
            self.good = [(WX.good_files()[n], WX.expected_bgra(n)[0]) for n in ("w17", "1x1")]
        else:
            self.mod, self.container, self.lead = gif_decoder, GO.CONTAINER, (None,)
            self.good = [(GX.good_files()[n][0], GX.expected(n)) for n in ("m4_noise", "size_1x1")]
        self.L = self.mod._bind()
        self.batch_fn = getattr(self.L, "ifhip_%s_decode_batch_device" % name)
        self.host_fn = getattr(self.L, "ifhip_%s_decode" % name)
        self.batch = getattr(self.mod, "decode_%s_batch" % name)
        self.info = getattr(self.mod, "%s_info" % name)
        self.h, self.w = self.good[0][1].shape[:2]

    def call_batch(self, frame_bytes, stride, frame=0x7F0000000000, files=True, file=True, n=1):
        """the pointers to device memory are made up: every call made here fails a check on the host"""
        buf = np.frombuffer(self.good[0][0], np.uint8)
        ptrs, lens = (C.c_void_p * 1)(buf.ctypes.data if file else None), (C.c_size_t * 1)(buf.size)
        frames, fb, st = (C.c_void_p * 1)(frame), (C.c_size_t * 1)(frame_bytes), (C.c_uint32 * 1)(stride)
        rc = self.batch_fn(ptrs if files else None, lens, n, *self.lead, frames, fb, st, 0x7F0000200000, None)
        return rc, self.L.ifhip_last_error_message()

    def call_host(self, stride, capacity, bitmap=True, file=True):
        buf = np.frombuffer(self.good[0][0], np.uint8)
        out, st = np.zeros(self.h * (4 * self.w + 16), np.uint8), C.c_uint32(0)
        lead = (0,) if self.lead else ()
        rc = self.host_fn(buf.ctypes.data if file else None, buf.size, *lead, out.ctypes.data if bitmap else None, stride, capacity, C.byref(st))
        return rc, self.L.ifhip_last_error_message()


_DECODERS = {}


def decoder(name):
    if name not in _DECODERS:
        _DECODERS[name] = Decoder(name)
    return _DECODERS[name]


def refusals(d):
    """case -> ((status code, message), the text the parent commit's source gives for it)"""
    w, h, stride = d.w, d.h, 4 * d.w + 8
    short = (h - 1) * stride + 4 * w - 4                               # one row short by four bytes: still a multiple of 4
    return {
        "batch: a null array": (d.call_batch(h * stride, stride, files=False), b"InvalidArgument: null pointer"),
        "batch: a null file pointer": (d.call_batch(h * stride, stride, file=False), b"InvalidArgument: null file pointer (file 0)"),
        "batch: 65536 files": (d.call_batch(h * stride, stride, n=65536), b"InvalidArgument: 1..65535 files per batch"),
        "batch: stride 4*w - 4": (d.call_batch(h * stride, 4 * w - 4), b"InvalidArgument: frame rows must be 4-byte aligned and stride >= 4*w"),
        "batch: stride + 2": (d.call_batch(h * stride, stride + 2), b"InvalidArgument: frame rows must be 4-byte aligned and stride >= 4*w"),
        "batch: one row short": (d.call_batch(short, stride), b"InvalidArgument: image_bytes %d is smaller than %d rows of stride %d" % (short, h, stride)),
        "batch: a null frame": (d.call_batch(h * stride, stride, frame=None), b"InvalidArgument: null frame pointer"),
        "host: a null file pointer": (d.call_host(stride, h * stride, file=False), b"InvalidArgument: null file pointer"),
        "host: stride 4*w - 4": (d.call_host(4 * w - 4, h * stride), b"InvalidArgument: stride smaller than a BGRA row or not a multiple of 4"),
        "host: stride + 2": (d.call_host(stride + 2, h * stride), b"InvalidArgument: stride smaller than a BGRA row or not a multiple of 4"),
        "host: one row short": (d.call_host(stride, (h - 1) * stride),
                                b"InvalidArgument: the frame needs %d bytes, the buffer has %d" % ((h - 1) * stride + 4 * w, (h - 1) * stride)),
        "host: a null bitmap": (d.call_host(stride, h * stride, bitmap=False), b"InvalidArgument: null bitmap pointer"),
    }


@pytest.mark.parametrize("name", DECODERS)
def test_every_refused_argument_is_invalid_argument_in_the_words_of_the_source(name):
    for case, ((rc, message), want) in refusals(decoder(name)).items():
        assert rc == INVALID, (name, case, rc)
        assert message == want, (name, case, message)


def test_the_three_decoders_refuse_in_the_same_words():
    """byte for byte, but for the numbers that follow the fixture's own size"""
    told = {name: refusals(decoder(name)) for name in DECODERS}
    for case in told["png"]:
        texts = {re.sub(rb"\d+", b"N", told[name][case][0][1]) if "short" in case else told[name][case][0][1] for name in DECODERS}
        assert len(texts) == 1, (case, texts)


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------
def own_frames(d, files, extra_stride, fill):
    out = []
    for data in files:
        try:
            info = d.info(data)
        except Exception:
            out.append(None)
            continue
        stride = get_stride(info["width"]) + extra_stride
        out.append(Bitmap(torch.full((1, info["height"] * stride), fill, dtype=torch.uint8, device=DEV), info["width"], info["height"], stride,
                          alpha_meaningful=True))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", DECODERS)
def test_one_batch_on_the_default_stream_a_side_stream_and_into_supplied_frames(name):
    """Two good files around one whose container does not parse.  The side-stream run is a smoke test: it shows that the
    hand-off is ordered on the caller's stream and does not deadlock; it does not prove the absence of a race.
    tests/test_gpu_stream_order.py does, for every decoder: the 0xA5 pre-fill of the frames arrives late on a stream that is
    held up on purpose, so a decode that ran ahead of that stream is overwritten."""
    d = decoder(name)
    files = [d.good[0][0], NOT_A_FILE, d.good[1][0]]
    wants = [d.good[0][1], None, d.good[1][1]]
    runs = [d.batch(files, device=DEV)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(d.batch(files, device=DEV))
    side.synchronize()
    runs.append(d.batch(files, device=DEV, frames=own_frames(d, files, 64, 0xA5)))
    torch.cuda.synchronize()
    for k, (frames, status) in enumerate(runs):
        assert status == [0, d.container, 0], (name, k, status)
        assert frames[1] is None, (name, k)
        for i in (0, 2):
            got, w = frames[i].to_numpy()[0], frames[i].w
            assert got.shape[0] == wants[i].shape[0] and w == wants[i].shape[1], (name, k, i)
            assert np.array_equal(got[:, :4 * w].reshape(wants[i].shape), wants[i]), (name, k, i)
    for i in (0, 2):                                                   # the third run: stride + 64, the padding still 0xA5
        got, w = runs[2][0][i].to_numpy()[0], runs[2][0][i].w
        assert got.shape[1] == get_stride(w) + 64 and (got[:, 4 * w:] == 0xA5).all(), (name, i)
