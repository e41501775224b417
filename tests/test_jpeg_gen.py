"""The crafted baseline JPEG corpus (tests/jpeg_gen.py) on the host, before any of it reaches a GPU: for every entry the
oracle's serial decoder returns exactly the coefficients and quantisation tables the writer encoded, libjpeg-turbo (Pillow)
decodes the in-range entries to the bytes of the oracle's pixel stage, and the host mirror of the device decoder's tables and
walks (ifhip_jpeg_debug_scan_report) starts exactly the writer's blocks, ends on its DC values and passes through the same state
at every sub-sequence boundary with the plain, the pair and the count tables.  What the corpus is FOR -- codes of 16 bits,
blocks of 1 665 bits, sub-sequences without a block start, a second-level pool that overflows without a test hook, blocks
across sub-sequence 512 and 1 008 -- is asserted from the writer's statistics and the report, not assumed.

Entries with coefficients of +-512..1023 at quantiser 1 are compared coefficient for coefficient only: far outside 0..255 the
oracle's pixel stage and libjpeg-turbo's SIMD IDCT differ, which is no entropy matter (a candidate for a later issue).

`accepts(name)` is what tests/jpeg_gen.device_cases() asks: only entries that pass here go to a device."""
import functools
import hashlib
import io

import numpy as np
import pytest

from oracle import oracle as O
from tests import jpeg_gen as G
from tests.test_jpeg_headers import _scan_report

# SHA-256 over the concatenated files of the corpus, in names() order: a writer that drifts is noticed
CORPUS_SHA256 = "345dec4bef7d4f8878772e8f58d4eb64d8bcd6ee7e3856d5ce19be68516a9cbb"


def check_entry(name):
    """every per-entry check; -> the host scan report"""
    data, planes, qt, st = G.entry(name)
    j = O.jpeg_read_coefficients(data)
    n = len(planes)
    assert j["ncomp"] == n and (j["width"], j["height"]) == (st["width"], st["height"]), name
    assert np.array_equal(j["qt"][:n], qt), name
    for c in range(n):
        assert j["coef"][c].shape == planes[c].shape and np.array_equal(j["coef"][c], planes[c]), (name, c)
    r = _scan_report(data)
    assert r.scan_complete == 1 and r.segments == st["segments"] and r.sub_sequences == st["n_sub"], name
    assert (r.segments_with_wrong_block_count, r.segments_with_invalid_codes) == (0, 0), name
    assert (r.pair_walk_mismatches, r.count_walk_mismatches) == (0, 0), name
    assert r.blocks == st["blocks"] == sum(p.shape[0] * p.shape[1] for p in planes), name
    assert list(r.dc_last_segment)[:n] == [int(p[-1, -1, 0]) for p in planes], name
    return r


def pillow_pixels_match(name):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFile
    data, planes, qt, st = G.entry(name)
    keep = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = st["tail"] == b""                # no EOI: libjpeg supplies one, Pillow has to be told
    try:
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = keep
    h, w = ref.shape[:2]
    px = O.jpeg_idct_color(O.jpeg_read_coefficients(data))[:, :4 * w].reshape(h, w, 4)
    return (h, w) == (st["height"], st["width"]) and np.array_equal(px[..., [2, 1, 0]], ref)


@functools.lru_cache(maxsize=None)
def _checked(name):
    try:
        r = check_entry(name)
        if G.entry(name)[3]["in_range"]:
            try:
                import PIL.Image  # noqa: F401
            except ImportError:
                pass
            else:
                assert pillow_pixels_match(name), f"{name}: libjpeg-turbo's pixels differ from the oracle's"
        return True, r
    except (AssertionError, RuntimeError) as e:
        return False, e


def accepts(name):
    return _checked(name)[0]


@pytest.mark.parametrize("name", G.names())
def test_entry_reads_back_and_the_host_walks_agree(name):
    ok, r = _checked(name)
    if not ok:
        raise r


@pytest.mark.parametrize("name", [n for n in G.names() if G.CORPUS[n].get("in_range")])
def test_libjpeg_turbo_decodes_the_in_range_entries_to_the_oracles_pixels(name):
    pytest.importorskip("PIL.Image")
    assert pillow_pixels_match(name)


def test_device_cases_are_the_whole_corpus():
    assert G.device_cases() == G.names()


def test_corpus_bytes_are_pinned():
    h = hashlib.sha256()
    for name in G.names():
        h.update(G.entry(name)[0])
    assert h.hexdigest() == CORPUS_SHA256


def _stats(name):
    return G.entry(name)[3]


def test_coverage_long_codes_long_blocks_and_empty_sub_sequences():
    st = {n: _stats(n) for n in G.names()}
    assert max(s["longest_block"] for s in st.values()) == 16 + 11 + 63 * 26 > 1536
    assert max(sum(s["subs_without_block_start"]) for s in st.values()) >= 100
    assert st["long_gray"]["longest_code"] == 16 and st["long_gray"]["long_symbols"] == 64 * st["long_gray"]["blocks"]
    # a block across three sub-sequences: the lane of the middle one enters inside the block and leaves inside it
    starts = st["long_gray"]["block_starts"][0]
    ends = starts[1:] + [st["long_gray"]["seg_bits"][0]]
    assert any((e - 1) // G.SUB_BITS - a // G.SUB_BITS >= 2 for a, e in zip(starts, ends))
    for name in ("maximal_gray", "spread_420", "gappy_444", "flat256_422", "ac256x16_gray", "limits_all16_gray"):
        assert st[name]["longest_code"] == 16 and st[name]["long_symbols"] > 0, name
    # blocks without an EOB, three ZRLs in a row, a ZRL directly before an EOB, DC-and-EOB blocks beside long ones
    for name in ("mixed_gray", "mixed_420", "mixed_spread_444"):
        s = st[name]
        assert s["blocks_without_eob"] > 0 and s["zrl"] >= 3 and s["zrl_before_eob"] > 0 and s["longest_block"] > 1536, name
        assert s["dc_and_eob_blocks"] > 0, name
    assert st["silent_zrl_past_63_gray"]["zrl_past_63"] > 0
    # DC category 11 with the extreme differences, AC category 10 with the extreme values
    for name in ("limits_all16_gray", "spread_limits_gray"):
        p = G.entry(name)[1][0].reshape(-1, 64).astype(np.int64)
        assert {2047, -2047} <= set(np.diff(p[:, 0]).tolist()) and p[:, 1:].max() == 1023 and p[:, 1:].min() == -1023, name
    # the 16-bit code 1111111111111110 is written
    data = G.entry("maximal_gray")[0]
    assert G.codes_of(G.maximal(list(range(16))))[15] == (0xFFFE, 16) and st["maximal_gray"]["longest_code"] == 16
    assert st["maximal_gray"]["stuffed"] > 0 and b"\xff\x00" in data          # byte stuffing falls out of the bits


def test_coverage_pool_overflow_without_a_hook():
    """3 x (128 + 2 x 128) second-level entries wanted, 768 there: some long prefixes sit in the pool, others are left to the
    serial search, in one image and with no test hook set."""
    r = _checked("pool_six_tables_444")[1]
    assert r.pool_entries_used == 768 and r.prefixes_left_to_search == 3
    r = _checked("pool_six_tables_long_444")[1]
    assert r.pool_entries_used > 0 and r.prefixes_left_to_search > 0
    r = _checked("pool_last_ac_444")[1]                                  # only the last component's AC table overflows
    assert r.pool_entries_used == 768 and r.prefixes_left_to_search == 2
    assert _checked("all16_444")[1].prefixes_left_to_search == 0


def test_coverage_boundaries_of_the_write_chunk_and_the_synchronisation_workgroup():
    """A block starts in front of sub-sequence 512 (the write pass's chunk) / 1 008 (what a synchronisation workgroup owns)
    and ends behind it; with restart intervals a segment begins AT 1 008, one ends in sub-sequence 512 and the next begins at
    513, and segments of the other file begin next to both."""
    a, b = _stats("bound_512_gray"), _stats("bound_1008_gray")
    assert a["n_sub"] > 1008 and b["n_sub"] > 1008 and a["segments"] == b["segments"] == 1
    assert G.straddles(a, 512) and G.straddles(b, 1008) and G.straddles(b, 512) and G.straddles(a, 1008)
    r = _stats("bound_restart_gray")
    assert 1008 in r["seg_first_sub"] and 513 in r["seg_first_sub"] and 504 in r["seg_first_sub"] and r["n_sub"] > 1100
    assert G.straddles(r, 512)                                             # inside the segment of sub-sequences 504..512
    m = _stats("bound_restart_mixed_gray")
    for edge in (512, 1008):
        assert min(abs(f - edge) for f in m["seg_first_sub"]) <= 1 and G.straddles(m, edge), (edge, m["seg_first_sub"])


def test_coverage_geometry_restarts_pads_and_headers():
    st = {n: _stats(n) for n in G.names()}
    assert {s["sampling"] for s in st.values()} == {"gray", "444", "422", "440", "420"}
    assert any(s["width"] % 16 and s["height"] % 16 for s in st.values() if s["sampling"] == "420")
    assert any(s["width"] % 8 and s["height"] % 8 for s in st.values() if s["sampling"] == "444")
    ri = {n: s["ri"] for n, s in st.items()}
    assert 0 in ri.values() and 1 in ri.values()
    assert any(r > 1 and s["mcus_w"] % r and r < s["mcus"] for r, s in zip(ri.values(), st.values()))     # divides no MCU row
    assert st["ri7_of_5_wide_420"]["mcus_w"] == 5 and ri["ri7_of_5_wide_420"] == 7
    assert ri["ri60000_440"] == 60000 > st["ri60000_440"]["mcus"] and st["ri60000_440"]["segments"] == 1
    assert st["ri1_tiny_gray"]["segments"] == st["ri1_tiny_gray"]["n_sub"] >= 300                         # one sub-sequence each
    s = st["ri1_long_420"]
    assert s["segments"] == s["mcus"] and min(b - a for a, b in zip(s["seg_first_sub"], s["seg_first_sub"][1:])) >= 9
    assert st["ri1_fill3_long_gray"]["fill_bytes"] == 3 * (st["ri1_fill3_long_gray"]["segments"] - 1)
    assert 0 < st["ri1_long_420"]["fill_bytes"] < 3 * s["segments"]
    assert {s["pad"] for s in st.values() if s["ri"]} == {"ones", "zeros", "random"}
    assert {s["sof"] for s in st.values()} == {0xC0, 0xC1}
    assert st["sof1_ids23_420"]["td"] == (2, 3, 3) and st["sof1_ids23_420"]["ta"] == (3, 2, 2) and st["sof1_ids23_420"]["tq"] == (2, 3, 3)
    qt = G.entry("wide_dqt_444")[2]
    assert qt[1].max() > 900 and qt[1].min() == 3 and qt[0].max() < 256      # a 16-bit DQT beside an 8-bit one
    assert G.entry("no_eoi_422")[0][-2:] != b"\xff\xd9" and G.entry("junk_after_eoi_gray")[0].count(b"\xff\xd9") >= 1
    assert any(s["stuffed"] > 0 for s in st.values())


def test_slow_synchronisation_entry_keeps_a_decoder_off_the_grid():
    """Every symbol of `slow_sync_gray` is 12 bits long, every 12-bit pattern but 1111... is a code, and no nibble of the data
    is 1111; a sub-sequence starts 4 t bits off the symbol grid (mod 12), block 0 is one symbol short so that no block starts
    on a sub-sequence boundary: a decoder that starts at a sub-sequence boundary never meets the true decode."""
    data, planes, qt, st = G.entry("slow_sync_gray")
    assert st["segments"] == 1 and st["n_sub"] >= 300 and st["longest_code"] == 4
    starts = st["block_starts"][0]
    assert starts[1] == 756 and all(b - a == 768 for a, b in zip(starts[1:], starts[2:]))
    assert not any(s % G.SUB_BITS == 0 for s in starts[1:])
    sos = data.index(b"\xff\xda") + 10
    scan = data[sos:-2]
    assert b"\xff" not in scan and not any((v >> 4) == 15 or (v & 15) == 15 for v in scan[:-1])       # (the last byte ends in pad bits)


def test_generator_is_quick():
    import time
    G.entry.cache_clear()
    t = time.perf_counter()
    G.entry("bound_512_gray")                                               # a 1.1 Mbit scan
    one = time.perf_counter() - t
    for n in G.names():
        G.entry(n)
    assert one < 2.0 and time.perf_counter() - t < 20.0


if __name__ == "__main__":      # python -m tests.test_jpeg_gen: print the digest of the corpus as the writer stands
    h = hashlib.sha256()
    for name in G.names():
        h.update(G.entry(name)[0])
    print(h.hexdigest())
