"""The format constants of csrc/vp8_tables.inc (RFC 6386) against an independent copy: each table occurs verbatim -- as bytes,
the AC quantiser table as 16-bit words -- in the libwebp shared object that Pillow loads."""
import glob
import os

import numpy as np
import pytest

from tests import vp8_gen as G

TABLES = ["kVp8DcTable", "kVp8AcTable", "kVp8CoeffProba0", "kVp8CoeffUpdateProba", "kVp8BModesProba", "kVp8Zigzag", "kVp8Bands",
          "kVp8Cat3", "kVp8Cat4", "kVp8Cat5", "kVp8Cat6", "kVp8BModeTree"]
SHAPES = {"kVp8DcTable": (128,), "kVp8AcTable": (128,), "kVp8CoeffProba0": (4, 8, 3, 11), "kVp8CoeffUpdateProba": (4, 8, 3, 11),
          "kVp8BModesProba": (10, 10, 9), "kVp8Zigzag": (16,), "kVp8Bands": (17,), "kVp8BModeTree": (18,)}


def libwebp_object():
    try:
        import PIL
    except ImportError:
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(PIL.__file__)))
    found = sorted(glob.glob(os.path.join(root, "pillow.libs", "libwebp-*.so*")) + glob.glob(os.path.join(root, "Pillow.libs", "libwebp-*.so*")))
    return found[0] if found else None


def test_the_tables_have_their_shapes_and_ranges():
    T = G.tables()
    assert sorted(T) == sorted(TABLES)
    for name, shape in SHAPES.items():
        assert T[name].shape == shape, name
    assert sorted(T["kVp8Zigzag"]) == list(range(16)) and T["kVp8Bands"].max() == 7
    assert (np.diff(T["kVp8DcTable"]) >= 0).all() and (np.diff(T["kVp8AcTable"]) > 0).all()
    assert T["kVp8DcTable"][0] == 4 and T["kVp8DcTable"][127] == 157 and T["kVp8AcTable"][127] == 284
    for name in ("kVp8CoeffProba0", "kVp8CoeffUpdateProba", "kVp8BModesProba"):
        assert T[name].min() >= 1 and T[name].max() <= 255, name
    tree = T["kVp8BModeTree"]
    assert sorted(-int(v) for i, v in enumerate(tree) if v <= 0 and not (v == 0 and i != 0)) == list(range(10))      # every mode is a leaf once


@pytest.mark.parametrize("name", TABLES)
def test_each_table_occurs_verbatim_in_the_libwebp_that_pillow_loads(name):
    path = libwebp_object()
    if path is None:
        pytest.skip("the libwebp shared object bundled with Pillow (pillow.libs/libwebp-*.so*) was not found")
    blob = open(path, "rb").read()
    t = G.tables()[name].reshape(-1)
    raw = t.astype("<u2").tobytes() if name == "kVp8AcTable" else t.astype(np.int8 if name == "kVp8BModeTree" else np.uint8).tobytes()
    assert raw in blob, name
