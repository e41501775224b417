"""tests/vp8l_gen.py before any test relies on it: every legal file it writes is decoded by libwebp (through Pillow), and
tests/vp8l_reader.py agrees with libwebp on it; the writer's counts show that the files hold what they are there for; and
every damaged file is refused by libwebp."""
import numpy as np
import pytest

from tests import vp8l_gen as G
from tests import webp_frames as F
from tests.vp8l_reader import FormatError, read_vp8l
from tests.webp_decode_fixtures import pillow_refuses

LEGAL = sorted(G.legal_files())


@pytest.mark.parametrize("name", LEGAL)
def test_libwebp_decodes_the_file_and_the_reader_agrees(name):
    data, _ = G.legal_files()[name]
    rgba, mode = F.pillow_decode(data)
    mine, info = read_vp8l(data)
    assert mine.shape == rgba.shape
    assert np.array_equal(mine[..., :3], rgba[..., :3])
    if mode == "RGBA":
        assert np.array_equal(mine, rgba)
    assert (info["bits"] + 7) // 8 == info["payload_bytes"]


def test_the_files_hold_what_they_are_there_for():
    files = G.legal_files()
    counts = {n: c for n, (_, c) in files.items()}
    infos = {n: read_vp8l(d)[1] for n, (d, _) in files.items()}
    assert infos["predictor_after_indexing"]["transforms"] == ["color_indexing", "predictor", "cross_color", "subtract_green"]
    assert counts["predictor_after_indexing"]["predictor_after_indexing"] == 1
    assert infos["indexing_last"]["transforms"][-1] == "color_indexing"
    assert set().union(*(c.get("modes", set()) for c in counts.values())) == set(range(14))
    bits = [b for i in infos.values() for b, t in zip(i["tile_bits"], i["transforms"]) if t in ("predictor", "cross_color")]
    assert 2 in bits and 9 in bits
    assert infos["tile_bits_9_cache_11"]["color_cache_bits"] == 11 and infos["meta_groups_cache_11"]["color_cache_bits"] == 11
    assert counts["codes"]["lone_long"] >= 1 and counts["codes"]["max_symbol"] >= 1 and counts["codes"]["len15"] >= 1
    assert counts["codes"]["distance_1_length_4096"] >= 1
    assert any(length == 4096 and dist == 1 for _, length, dist in infos["codes"]["matches"])
    for name in ("distance_map_w3", "distance_map_w1", "distance_map_w23"):
        assert set(range(1, 121)) <= counts[name]["distance_codes"], name
    assert counts["distance_map_w3"]["clamped"] >= 1 and counts["distance_map_w1"]["clamped"] >= 1
    assert infos["meta_groups"]["groups"] == 7 and infos["meta_groups"]["prefix_bits"] == 2
    assert counts["meta_groups"]["copy_into_other_group"] >= 1 and counts["meta_groups"]["copy_into_other_group_mid_tile"] >= 1
    assert any(c.get("overlapping", 0) for c in counts.values())
    wrapped = files["vp8x_wrapped"][0]
    assert wrapped[12:16] == b"VP8X" and b"EXIF" in wrapped and b"ABCD\x03\x00\x00\x00\x01\x02\x03\x00" in wrapped        # an odd chunk with its padding byte


def test_libwebp_decodes_the_files_the_reader_does_not_read():
    for name, (data, _) in G.files_beyond_the_reader().items():
        rgba, mode = F.pillow_decode(data)
        assert mode == "RGBA" and rgba.shape == (7, 9, 4), name
        with pytest.raises(IndexError):                                # (why Pillow alone is their yardstick)
            read_vp8l(data)


@pytest.mark.parametrize("name", sorted(G.damaged_files()))
def test_libwebp_refuses_the_damaged_file(name):
    data, _status = G.damaged_files()[name]
    assert pillow_refuses(data)
    with pytest.raises((FormatError, IndexError)):                     # (IndexError: a simple code's symbol beyond the alphabet)
        read_vp8l(data)
