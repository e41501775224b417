"""ifhip_jpeg_entropy_prepare (pinned staging: it needs the device) behind the one marker walk: on small files of
tests/golden/make_jpeg_marker_golden.py's corpus -- whole ones and mutated ones -- it answers as ifhip_jpeg_parse_headers does,
its handle reports the same frame, and a batch decoded from prepared handles holds the coefficients the host reader
(ifhip_jpeg_read_coefficients_host) reads: the unified un-stuffing walk feeds the kernels the words it always did."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd.codecs import mozjpeg_decoder as D  # noqa: E402
from tests.test_jpeg_marker_walk import _generator  # noqa: E402
from tests.test_jpeg_progressive import read_host  # noqa: E402

DEV = "cuda:0"
SIDE = 100                            # the files sent to prepare are at most this many pixels a side (or refused by the parser)
OWN_REFUSALS = ("ends after", "more than 512 MB of scan data")     # what prepare adds behind the parse


def _headers(L, data):
    w, h, n, ri = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_uint32()
    hs, vs = np.zeros(3, np.uint8), np.zeros(3, np.uint8)
    rc = L.ifhip_jpeg_parse_headers(np.frombuffer(data, np.uint8).ctypes.data, len(data), C.addressof(w), C.addressof(h), C.addressof(n), hs.ctypes.data, vs.ctypes.data, None, None,
                                    None, C.addressof(ri))
    msg = (L.ifhip_last_error_message() or b"").decode() if rc else ""
    return rc, msg, (w.value, h.value, n.value, hs.tolist(), vs.tolist())


def test_prepare_answers_as_the_header_parse_does():
    M = _generator()
    L = D._bind_entropy()
    L.ifhip_jpeg_prepared_info.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    cases = M.corpus()
    small = []
    for name, data in cases:
        rc, msg, frame = _headers(L, data)
        if rc != 0 or max(frame[0], frame[1]) <= SIDE:
            small.append((name, data, rc, msg, frame))
    plain = [c for c in small if not c[0].startswith(("mutated:", "hand:"))]
    mutated = [c for c in small if c[0].startswith("mutated:")]
    mutated = mutated[::max(1, len(mutated) // 50)][:50]
    assert len(plain) >= 100 and len(mutated) == 50
    prepared = refused = own = 0
    with torch.cuda.device(DEV):
        for name, data, rc, msg, frame in plain + mutated:
            h = C.c_void_p()
            got = L.ifhip_jpeg_entropy_prepare(C.byref(h), np.frombuffer(data, np.uint8).ctypes.data, len(data))
            got_msg = (L.ifhip_last_error_message() or b"").decode() if got else ""
            try:
                if rc == 0 and got != 0 and any(t in got_msg for t in OWN_REFUSALS):
                    own += 1
                    continue
                assert (got, got_msg) == (rc, msg), name
                if got != 0:
                    refused += 1
                    continue
                prepared += 1
                w, hh, n = C.c_uint32(), C.c_uint32(), C.c_int()
                hs, vs = np.zeros(3, np.uint8), np.zeros(3, np.uint8)
                assert L.ifhip_jpeg_prepared_info(h, C.addressof(w), C.addressof(hh), C.addressof(n), hs.ctypes.data, vs.ctypes.data) == 0
                assert (w.value, hh.value, n.value, hs.tolist(), vs.tolist()) == frame, name
            finally:
                if h:
                    L.ifhip_jpeg_prepared_destroy(h)
    assert prepared >= 100 and refused >= 10, (prepared, refused, own)     # both answers are met, whole files and mutated ones


@pytest.mark.parametrize("name", ["jpeg_entropy_cases.npz:97x61_gradient_4:2:0_q75_optimize=False_restart_marker_rows=1", "crafted:std_gray",
                                  "jpeg_entropy_cases.npz:97x61_waves_4:4:4_q85_optimize=True"])
def test_prepared_batch_holds_the_host_readers_coefficients(name):
    """a 4:2:0 file with a restart interval, a grey one, one with optimised tables: two of each in a batch of prepared handles"""
    M = _generator()
    data = dict(M.plain_cases(M.corpus()))[name]
    want = read_host(data)
    ent = D.JpegEntropyBatch([data, data], DEV, prepared=True)
    coef = ent.read_coefficients()
    assert (ent.width, ent.height, ent.ncomp) == (want["width"], want["height"], want["ncomp"])
    assert (name.endswith("rows=1")) == (ent.n_segments > 2)
    for c in range(ent.ncomp):
        for k in range(2):
            assert np.array_equal(coef[c][k].cpu().numpy(), want["coef"][c]), (name, c, k)
        assert np.array_equal(ent.qt[0][c], want["qt"][c]), (name, c)
