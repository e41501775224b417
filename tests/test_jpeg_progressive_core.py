"""The device progressive JPEG decoder's algorithm without a device: csrc/jpeg_progressive_read.cpp (the front end: scans,
streams, dependency levels) and csrc/jpeg_progressive_core.hpp (the four block decoders, the walk of a stream by a wave, the
CPU form of every launch).  tests/jpeg_progressive_emulate.cpp runs the batch as loops with exactly the device's block sizes
over a block of exactly the device's size, the workgroup's scratch pre-filled with 0xA5.  The yardstick is the host reader
(ifhip_jpeg_read_coefficients_host): its planes, byte for byte, padding blocks included.  The same cases run a second time
through a stand-alone program built with ASan + UBSan (its own main; no sanitizer in this process)."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests import jpeg_prog_fixtures as X
from tests import jpeg_prog_gen as G

ACCEPTED = sorted(X.accepted_files())
DAMAGED = sorted(X.damaged_files())


def checksum(planes):
    s = 0
    for p in planes:
        for v in np.ascontiguousarray(p).view(np.uint16).ravel().tolist():
            s = ((s * 0x01000193) & 0xFFFFFFFF) ^ v
    return s


@pytest.fixture(scope="module")
def emulated():
    """every accepted and damaged file through the emulation, in batches of mixed geometries: name -> (rc, status, planes)"""
    names = ACCEPTED + DAMAGED
    files = X.accepted_files()
    files = [files[n] if n in files else X.damaged_files()[n] for n in names]
    out = {}
    for i in range(0, len(names), 16):
        for name, r in zip(names[i:i + 16], X.emulate_batch(files[i:i + 16])):
            out[name] = r
    return out


@pytest.mark.parametrize("name", ACCEPTED)
def test_the_planes_equal_the_host_readers(name, emulated):
    rc, status, planes = emulated[name]
    assert rc == 0 and status == 0, (name, rc, status)
    hrc, want, _ = X.host_planes(name)
    assert hrc == 0 and len(planes) == len(want)
    for c in range(len(want)):
        assert planes[c].shape == want[c].shape and np.array_equal(planes[c], want[c]), (name, c)


def test_the_latched_tables_and_the_facts():
    for name in ("odd_17x9_420", "pillow_100x75_420_q30_rst0", "writer_97x61_420_flags3"):
        rc, facts = X.emu_prepare(X.accepted_files()[name])
        _, want, qt = X.host_planes(name)
        assert rc == 0 and np.array_equal(facts["qt"][:facts["ncomp"]], qt[:facts["ncomp"]])
        assert [facts["bh"][c] for c in range(facts["ncomp"])] == [p.shape[0] for p in want]
    assert X.emu_prepare(X.pillow_files()["pillow_321x203_420_q30_rst0"])[1]["levels"] == 3     # libjpeg's script: three levels, ten scans
    assert X.emu_prepare(G.entry("odd_24x24_444")[0])[1]["levels"] == G.entry("odd_24x24_444")[3]["levels"] == 4


def test_refused_files_answer_method_not_implemented():
    for name, data in G.refused().items():
        assert X.emu_prepare(data)[0] == X.METHOD_NOT_IMPLEMENTED, name
    base = X.save(X.image(40, 30, 1), quality=80)
    assert X.emu_prepare(base)[0] == X.METHOD_NOT_IMPLEMENTED and X.emu_prepare(b"\xff\xd8\xff\xd9")[0] == X.METHOD_NOT_IMPLEMENTED
    cmyk_like = bytearray(G.entry("gray_8x8")[0])
    assert X.emu_prepare(bytes(cmyk_like[:40]))[0] == X.METHOD_NOT_IMPLEMENTED       # cut in the tables: no scan


def test_the_library_front_end_gives_the_same_answers():
    """ifhip_jpeg_progressive_prepare (no device needed): refusals, and the facts of a prepared file"""
    from imageflow_amd.codecs import jpeg_progressive_decoder as D
    for name, data in G.refused().items():
        with pytest.raises(Exception) as e:
            D.PreparedProgressive(data)
        assert "MethodNotImplemented" in str(e.value), name
    for name in ("odd_17x9_420", "pillow_gray_150x90"):
        p = D.PreparedProgressive(X.accepted_files()[name])
        rc, facts = X.emu_prepare(X.accepted_files()[name])
        assert (p.width, p.height, p.ncomp, p.n_scans, p.n_streams, p.n_levels) == tuple(facts[k] for k in ("width", "height", "ncomp", "scans", "streams", "levels"))
        assert p.blocks_w == facts["bw"] and p.blocks_h == facts["bh"] and np.array_equal(p.qt, facts["qt"])
        p.close()


def test_damaged_files_raise_a_status_or_decode_as_the_host_reader_does(emulated):
    raised = exact = refused = 0
    for name in DAMAGED:
        rc, status, planes = emulated[name]
        if rc:
            assert rc == X.METHOD_NOT_IMPLEMENTED, name
            refused += 1
        elif status:
            assert 0 < status < 32, (name, status)
            raised += 1
        else:
            hrc, want, _ = X.host_planes(name)
            assert hrc == 0, "the emulation decoded a file the host reader refuses: %s" % name
            assert all(np.array_equal(planes[c], want[c]) for c in range(len(want))), name
            exact += 1
    assert raised > 20 and exact > 0, (raised, exact, refused)


def test_every_case_again_under_asan_and_ubsan(emulated):
    d = tempfile.mkdtemp(prefix="jpeg_progressive_sanitize_")
    exe, cases = os.path.join(d, "jpeg_progressive_emulate"), os.path.join(d, "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DJPEG_PROG_EMU_MAIN", X.SRC, "-o", exe], check=True)
    want = []
    everything = dict(X.damaged_files())
    everything.update(X.accepted_files())
    everything.update(G.refused())
    names = sorted(everything)
    with open(cases, "wb") as f:
        for name in names:
            data = everything[name]
            f.write(struct.pack("<I", len(data)) + data)
            if name in emulated:
                rc, status, planes = emulated[name]
                want.append("%d %d %d" % (rc, status if not rc else 0, checksum(planes) if not rc and not status else 0))
            else:
                want.append("%d 0 0" % X.METHOD_NOT_IMPLEMENTED)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want
