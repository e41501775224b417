"""The truecolour PNG coder's kernels write the CPU emulation's file, byte for byte (ifhip_png_encode_batch_device against
png_emu_filter -> png_emu_deflate -> png_emu_file of tests/png_emulate.cpp, whose bytes tests/test_coder_bytes_pinned.py
pins).  The other GPU tests of the coder check pixels and sizes; this one holds the kernels and the emulation to the
same parse, the same codes and the same bit placement: a fixed block, dynamic blocks whose second chunk searches the
first chunk's window, and stored blocks."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.codecs import libpng_encoder as PNG  # noqa: E402
from tests import png_oracle as P  # noqa: E402
from tests.test_gpu_png_encode import DEV, bgra_from_rgba, bitmap  # noqa: E402
from tests.test_png_device_coder import deflate, emulator, filtered  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = {
    "1x1_rgba": lambda: np.array([[[200, 30, 77, 128]]], np.uint8),                                  # one fixed block
    "photo_rgb": lambda: P.photo_frame(120, 100),                                                  # 36,100 bytes: two chunks, dynamic blocks
    "noise_rgb": lambda: np.random.default_rng(21).integers(0, 256, (100, 120, 3), dtype=np.uint8),   # stored blocks
}


def emulated_file(px, level):
    h, w, bpp = px.shape
    color_type = PNG.PNG_RGBA if bpp == 4 else PNG.PNG_RGB
    z, st = deflate(filtered(px), bpp, 1 + w * bpp, level)
    out = np.zeros(len(z) + 256, np.uint8)
    n = emulator().png_emu_file(np.frombuffer(z, np.uint8).ctypes.data, len(z), w, h, color_type, out.ctypes.data)
    return out[:n].tobytes(), st


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_the_device_writes_the_emulations_file(name):
    px = FRAMES[name]()
    h, w, bpp = px.shape
    want, st = emulated_file(px, 6)
    print(name, len(want), "bytes", st)
    if name == "1x1_rgba":
        assert (st["stored"], st["fixed"], st["dynamic"]) == (0, 1, 0)
    elif name == "photo_rgb":
        assert (st["stored"], st["fixed"], st["dynamic"]) == (0, 0, 2)
    else:
        assert (st["stored"], st["fixed"], st["dynamic"]) == (2, 0, 0)
    stage = PNG.PngEncodeStage(w, h, PNG.PNG_RGBA if bpp == 4 else PNG.PNG_RGB, 1, DEV)
    files, status = stage.encode(bitmap(bgra_from_rgba(px)[None], w, h), zlib_level=6)
    assert status == [0]
    assert files[0] == want
