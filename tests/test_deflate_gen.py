"""The inflate of csrc/png_decode_core.hpp against deflate streams that zlib's encoder never writes, without a device.
tests/deflate_gen.py writes them from fixed seeds; zlib.decompress, the decoder that accepts all of RFC 1951, says what they
hold (a failure THERE is a bug of the generator), and the CPU emulation (tests/png_decode_emulate.cpp) must give the same
bytes at the full size and at sizes that end early.  `stats` says what every stream contains, so the coverage the names
promise is asserted here.  Everything that tests/test_gpu_png_inflate_streams.py sends to a GPU -- deflate_gen.device_cases()
-- goes through the ASan + UBSan build of the emulation here, with the status the GPU test expects."""
import random
import struct
import zlib

import pytest

from tests import deflate_gen as G
from tests.test_png_decode_core import OK, inflate, run_under_sanitizers

NAMES = G.names()


def first_bytes(z, cap):
    """what zlib's decoder gives for the first `cap` bytes of a stream (the checksum of a longer stream is never reached)"""
    return zlib.decompressobj().decompress(z, cap) if cap else b""


# ---- the generator against zlib ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_zlib_inflates_every_corpus_stream_to_its_data(name):
    data, z, stats = G.entry(name)
    assert zlib.decompress(z) == data
    assert (stats["inflated"], stats["compressed"]) == (len(data), len(z)) and len(data) <= 128 * 1024


def test_the_entry_points_and_that_a_seed_gives_the_same_stream_again():
    data, z, stats = G.random_stream(random.Random(3), 5000)
    assert 4000 < len(data) <= 5000 and data[0] == 0 and zlib.decompress(z) == data
    assert G.random_stream(random.Random(3), 5000)[1] == z and G.random_stream(random.Random(4), 5000)[1] != z
    text = b"how much wood would a woodchuck chuck if a woodchuck could chuck wood? " * 40
    z, stats = G.reencode(text, random.Random(3))
    assert zlib.decompress(z) == text and len(z) < len(text) // 2 and sum(stats["matches"].values()) > 0
    assert zlib.decompress(G.reencode(b"", random.Random(1))[0]) == b""


def test_length_limited_codes_are_complete_and_within_the_limit():
    rng = random.Random(9)
    for trial in range(300):
        n, limit = rng.randint(2, 286), rng.choice((7, 15))
        if limit == 7:
            n = min(n, 19)
        w = {s: rng.choice((1, rng.random(), 2.0 ** rng.randint(0, 40), G._fib(40)[rng.randrange(40)])) for s in range(n)}
        lens = G.limited_lengths(w, limit)
        assert sorted(lens) == list(range(n)) and 1 <= min(lens.values()) and max(lens.values()) <= limit
        assert sum(1 << (limit - l) for l in lens.values()) == 1 << limit, (trial, n, limit)


def test_the_corpus_has_the_sizes_that_matter():
    sizes = [(G.entry(n)[2]["inflated"], G.entry(n)[2]["compressed"]) for n in NAMES]
    assert sum(a for a, _ in sizes) <= 8 << 20
    assert sum(a > 32768 + 8192 for a, _ in sizes) >= 30                 # the ring wraps and several flushes happen
    assert sum(a > 65535 for a, _ in sizes) >= 20
    assert sum(b > 4096 for _, b in sizes) >= 20                           # tokens straddle the staged-input refill
    assert sum(b > 3 * 4096 for _, b in sizes) >= 10


# ---- coverage: asserted, not hoped for ----------------------------------------------------------------------------------------------
def test_the_coverage_the_names_promise():
    st = {n: G.entry(n)[2] for n in NAMES}
    m = st["overlaps"]["matches"]
    assert m["dist 1..63, n > dist"] >= 80 and m["dist 64..257, n > dist"] >= 40 and m["dist == n"] >= 18 and m["dist == n + 1"] >= 18
    m = st["ring_wraps"]["matches"]
    assert m["source wraps the ring"] >= 3 and m["destination wraps the ring"] >= 3 and m["dist + n > 32768 above 32768"] >= 10
    m = st["flush_thresholds"]["matches"]
    assert m["ends on a flush threshold"] >= 3 and m["crosses a flush threshold"] >= 2 and m["dist + n > 32768 above 32768"] >= 2
    m = st["across_blocks"]["matches"]
    assert m["into a stored block"] >= 3 and m["across a block of another type"] >= 2
    s = st["stored_bit_offsets"]
    assert sorted(s["stored_bit_offsets"]) == list(range(8)) and all(s["stored_lengths"][n] for n in G.STORED_LENGTHS)
    s = st["input_boundaries"]
    assert s["headers"]["stored header across an input boundary"] == 1 and s["headers"]["dynamic header across an input boundary"] == 1
    assert s["matches"]["token across an input boundary"] == 1
    for pad in range(8):
        assert st["final_padding_%d" % pad]["final_pad_bits"] == pad
    for kind in ("stored", "fixed", "dynamic"):
        s = st["empty_last_%s" % kind]
        assert s["first_block_empty"] and s["empty_blocks"][(kind, "last")] == 1
        assert all(s["empty_blocks"][(k, "not last")] >= 3 for k in ("stored", "fixed", "dynamic"))
    s = st["deep_codes"]
    assert s["max_ll_code_used"] == 15 and s["max_d_code_used"] == 15 and s["walk_uses"] >= 500      # (of some 1700 codes)
    s = st["header_shapes"]
    for shape in ("one distance code of one bit", "no distance code", "HLIT padded", "HDIST padded", "HCLEN padded", "HCLEN 5", "HCLEN 19"):
        assert s["headers"][shape] >= 1, shape
    assert s["runs_across_hlit"] >= 3 and s["matches"]["258 as symbol 284 + 31"] >= 1 and s["matches"]["258 as symbol 285"] >= 1


def test_the_random_streams_reach_every_class_on_their_own():
    """the named constructions are the floor; the random streams must meet the same classes in other company"""
    s = G.merge_stats(G.entry(n)[2] for n in NAMES if n.startswith("random_"))
    assert all(s["blocks"][k] >= 40 for k in ("stored", "fixed", "dynamic"))
    assert all(s["empty_blocks"][(k, last)] >= 1 for k in ("stored", "fixed", "dynamic") for last in ("last", "not last"))
    assert sorted(s["stored_bit_offsets"]) == list(range(8))
    assert all(s["stored_lengths"][n] >= 1 for n in G.STORED_LENGTHS)
    for k in ("dist 1..63, n > dist", "dist 64..257, n > dist", "dist == n", "dist == n + 1", "source wraps the ring", "destination wraps the ring",
              "dist + n > 32768 above 32768", "crosses a flush threshold", "into a stored block", "across a block of another type",
              "258 as symbol 284 + 31", "258 as symbol 285", "token across an input boundary"):
        assert s["matches"][k] >= 5, k
    for k in ("one distance code of one bit", "no distance code", "HLIT padded", "HDIST padded", "HCLEN padded",
              "literal/length code of 15 bits", "distance code of 15 bits"):
        assert s["headers"][k] >= 5, k
    assert s["max_ll_code_used"] == 15 and s["max_d_code_used"] == 15 and s["walk_uses"] >= 1000 and s["runs_across_hlit"] >= 10


def test_the_reencoded_images_are_real_filtered_streams_in_a_foreign_parse():
    for name, (ct, depth, w, h, inter) in G.IMAGES.items():
        data, z, stats = G.entry(name)
        assert len(data) == G.O.inflated_size(w, h, ct, depth, inter) and stats["blocks"]["dynamic"] >= 1
        assert G.O.parse(G.image_file(name))["idat"] == z
    assert {(v[0], v[1]) for v in G.IMAGES.values()} == {(6, 8), (2, 16), (3, 4), (0, 1), (4, 8)}
    assert sum(sum(G.entry(n)[2]["matches"].values()) for n in G.IMAGES) >= 1000


# ---- the emulation against zlib --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_emulation_gives_zlibs_bytes_at_the_full_size_and_at_sizes_that_end_early(name):
    data, z, stats = G.entry(name)
    caps = [len(data), len(data) - 1, len(data) // 2] + [c for c in (stats["inside_match"], stats["inside_stored"]) if c is not None]
    for cap in caps:
        st, got = inflate(z, cap)
        assert st == OK and got == data[:cap], (cap, st, next((i for i, (a, b) in enumerate(zip(got, data)) if a != b), None))


def test_every_corpus_stream_ends_early_inside_a_match_or_a_stored_block():
    for name in NAMES:
        stats = G.entry(name)[2]
        assert stats["inside_match"] is not None or stats["inside_stored"] is not None, name
    for name in G.SURPLUS:
        assert len(G.surplus_caps(name)) >= 3
    assert any(G.entry(n)[2]["inside_match"] and G.entry(n)[2]["inside_stored"] for n in G.SURPLUS)


@pytest.mark.parametrize("name", sorted(G.damaged()))
def test_damaged_streams_give_their_status(name):
    z, cap, want = G.damaged()[name]
    with pytest.raises(zlib.error):
        zlib.decompress(z)
    assert inflate(z, cap)[0] == want


def test_a_wrong_checksum_is_met_only_at_the_exact_size():
    z, data = G.wrong_adler("random_05")
    with pytest.raises(zlib.error):
        zlib.decompress(z)
    assert inflate(z, len(data))[0] == G.ADLER
    assert inflate(z, len(data) - 1) == (OK, data[:-1])


def test_the_hosts_inflate_reads_an_iccp_profile_that_the_generator_compressed():
    """csrc/png_read.cpp inflates a compressed iCCP profile on the host with the same core: the colour verdict of png_info"""
    pytest.importorskip("torch")
    from imageflow_amd.codecs import libpng_decoder as D
    from tests.test_jpeg_headers import P3_XYZ, make_icc
    import numpy as np
    for seed in range(8):
        for profile, want in ((make_icc(), D.COLOR_SRGB), (make_icc(xyz=P3_XYZ), D.COLOR_OTHER)):
            z, stats = G.reencode(profile, random.Random(seed))
            assert zlib.decompress(z) == profile
            data = G.O.write_png(np.zeros((3, 3, 3), np.uint32), 2, 8, ancillary=G.O.chunk(b"iCCP", b"icc\0\0" + z))
            assert D.png_info(data)["color_kind"] == want, seed


# ---- everything that goes to a GPU, under ASan + UBSan first ----------------------------------------------------------------------------
def test_under_sanitizers_everything_that_goes_to_a_device():
    cases = G.device_cases()
    labels = [c[0] for c in cases]
    assert set(NAMES) <= set(labels) and set(G.damaged()) <= set(labels) and len(set(labels)) == len(labels)
    lines = run_under_sanitizers([struct.pack("<III", 0, len(z), cap) + z for _, z, cap, _ in cases])
    for (label, z, cap, want), line in zip(cases, lines):
        st, n, crc = (int(v) for v in line.split())
        assert st == want, (label, st, want)
        if want == OK:
            assert n == cap and crc == zlib.crc32(first_bytes(z, cap)), label
