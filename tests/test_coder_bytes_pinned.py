"""The bytes the CPU emulations of the device coders write, pinned: SHA-256 of every file of tests/webp_frames.cases() and
of the zlib stream of every entry of test_png_device_coder.STREAMS at levels 6 and 0 (tests/coder_bytes_pinned.json,
recorded before the code construction moved to csrc/prefix_code_core.hpp).  The emulators compile the headers the kernels
are built from, and the GPU tests hold the kernels to the emulators' bytes, so a change of a single bit in either coder's
output shows here."""
import hashlib
import json
import os

import pytest

from tests import webp_emulation as W
from tests import webp_frames as F
from tests.test_png_device_coder import STREAMS, deflate

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "coder_bytes_pinned.json")) as _f:
    PINNED = json.load(_f)
LEVELS = (6, 0)


def webp_digest(name):
    frame, alpha = F.cases()[name]
    return hashlib.sha256(W.encode(frame, alpha)[0]).hexdigest()


def png_digest(name, level):
    stream, pitch = STREAMS[name]()
    return hashlib.sha256(deflate(stream, 3, pitch, level)[0]).hexdigest()


def test_every_case_is_pinned():
    assert sorted(PINNED["webp"]) == sorted(F.cases())
    assert sorted(PINNED["png"]) == sorted("%s/%d" % (n, l) for n in STREAMS for l in LEVELS)


@pytest.mark.parametrize("name", sorted(F.cases()))
def test_webp_emulation_writes_the_pinned_file(name):
    assert webp_digest(name) == PINNED["webp"][name]


@pytest.mark.parametrize("name", sorted(STREAMS))
@pytest.mark.parametrize("level", LEVELS)
def test_png_emulation_writes_the_pinned_stream(name, level):
    assert png_digest(name, level) == PINNED["png"]["%s/%d" % (name, level)]


if __name__ == "__main__":      # python -m tests.test_coder_bytes_pinned: print the digests of the tree as it stands
    print(json.dumps({"webp": {n: webp_digest(n) for n in sorted(F.cases())},
                      "png": {"%s/%d" % (n, l): png_digest(n, l) for n in sorted(STREAMS) for l in LEVELS}}, indent=1))
