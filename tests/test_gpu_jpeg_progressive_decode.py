"""The device progressive JPEG decoder (csrc/jpeg_progressive_decode.hip) on the GPU: its planes equal the CPU emulation's
(tests/jpeg_progressive_emulate.cpp) and the host reader's (ifhip_jpeg_read_coefficients_host) byte for byte -- padding blocks
included -- on the corpus of tests/jpeg_prog_gen.py, Pillow's progressive files and this library's own progressive writer's;
a damaged file in the middle of a batch of mixed geometries gets the emulation's status word and disturbs neither its
neighbours nor a byte behind any plane; the host-buffer call returns the same planes and tables."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd.codecs import jpeg_progressive_decoder as D  # noqa: E402
from tests import jpeg_prog_fixtures as X  # noqa: E402
from tests import jpeg_prog_gen as G  # noqa: E402

DEV = "cuda:0"
GUARD = 256
ACCEPTED = sorted(X.accepted_files())


def guarded(nbytes):
    """a device block of nbytes + GUARD bytes, all 0xA5 -> (whole block, the data part)"""
    t = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return t, t[:nbytes]


def run_batch(files):
    """files through ONE device call, every plane and the status array with a guard behind it
    -> [(status, planes as numpy)], and asserts the guards"""
    prepared = [D.PreparedProgressive(f) for f in files]
    blocks, coef = [], []
    for p in prepared:
        planes = []
        for c in range(p.ncomp):
            whole, data = guarded(int(np.prod(p.plane_shape(c))) * 2)
            blocks.append(whole)
            planes.append(data.view(torch.int16).view(p.plane_shape(c)))
        coef.append(planes)
    swhole, sdata = guarded(4 * len(files))
    status = sdata.view(torch.int32)
    D.decode_batch_device(prepared, coef, status, DEV)
    torch.cuda.synchronize()
    for whole in blocks + [swhole]:
        assert bool((whole[-GUARD:] == 0xA5).all()), "a write behind a plane or the status array"
    words = status.cpu().numpy()
    return [(int(words[i]) & 0xFFFFFFFF, [t.cpu().numpy() for t in coef[i]]) for i in range(len(files))], prepared


@pytest.fixture(scope="module")
def decoded():
    """every accepted file -- every size, sampling and script, the 1024 x 1024 frame among them -- through one batch"""
    files = X.accepted_files()
    got, prepared = run_batch([files[n] for n in ACCEPTED])
    assert max(p.n_levels for p in prepared) == 4
    return dict(zip(ACCEPTED, got))


@pytest.fixture(scope="module")
def emulated():
    files = X.accepted_files()
    out = {}
    for i in range(0, len(ACCEPTED), 16):
        names = ACCEPTED[i:i + 16]
        out.update(zip(names, X.emulate_batch([files[n] for n in names])))
    return out


@pytest.mark.parametrize("name", ACCEPTED)
def test_the_device_planes_equal_the_emulations_and_the_host_readers(name, decoded, emulated):
    status, planes = decoded[name]
    assert status == 0, (name, status)
    rc, want, _ = X.host_planes(name)
    erc, estatus, eplanes = emulated[name]
    assert rc == 0 and erc == 0 and estatus == 0 and len(planes) == len(want)
    for c in range(len(want)):
        assert planes[c].shape == want[c].shape
        assert np.array_equal(planes[c], eplanes[c]), (name, c, "emulation")
        assert np.array_equal(planes[c], want[c]), (name, c, "host reader")


def test_a_stream_longer_than_the_stage_is_among_them():
    rc, facts = X.emu_prepare(G.entry("long_stream_64x48_444")[0])
    assert rc == 0 and facts["max_stream_bits"] > facts["stage_words"] * 32 == G.STAGE_BITS


def test_a_damaged_file_in_a_mixed_batch():
    damaged = X.damaged_files()
    emu = dict(zip(sorted(damaged), X.emulate_batch([damaged[n] for n in sorted(damaged)])))
    bad = [n for n in sorted(damaged) if emu[n][0] == 0 and emu[n][1] != 0]
    assert len(bad) >= 3
    good = ["gray_8x8", "odd_24x24_420", "pillow_100x75_422_q90_rst3", "enc_24x24_444", "writer_64x48_444_flags3", "restarts_17x9_440"]
    order = [good[0], good[1], bad[0], good[2], bad[1], good[3], bad[2], good[4], good[5]]
    files = X.accepted_files()
    got, prepared = run_batch([damaged[n] if n in damaged else files[n] for n in order])
    assert len({(p.width, p.height, tuple(p.h_samp)) for p in prepared}) >= 5 and len({p.n_levels for p in prepared}) >= 3
    for name, (status, planes) in zip(order, got):
        if name in damaged:
            assert status == emu[name][1] != 0, (name, status, emu[name][1])
        else:
            assert status == 0, name
            want = X.host_planes(name)[1]
            assert all(np.array_equal(planes[c], want[c]) for c in range(len(want))), name


def test_the_host_buffer_call_returns_the_same_planes_and_tables():
    for name in ("odd_17x9_422", "pillow_100x75_420_q90_rst2", "gray_8x8"):
        planes, qt, status = D.decode_host(X.accepted_files()[name])
        _, want, want_qt = X.host_planes(name)
        assert status == 0 and len(planes) == len(want)
        assert all(np.array_equal(planes[c], want[c]) for c in range(len(want))), name
        assert np.array_equal(qt[:len(want)], want_qt[:len(want)])
