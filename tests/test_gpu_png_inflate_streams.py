"""png_inflate_kernel on an MI355X against deflate streams that zlib's ENCODER never writes (libdeflate, zopfli, 7-zip, oxipng and
pngcrush do): the seeded corpus of tests/deflate_gen.py -- random parses, matches at the window's far end and across the ring's
end, short repeating patterns, 15-bit codes, padded and run-length coded headers, stored blocks at every bit offset, empty
blocks -- as PNG files of one gray-8 row, and real images whose filtered streams were re-encoded.  zlib's DECODER says what
every stream holds; every comparison is byte for byte, with no tolerance anywhere, and a frame's padding, pre-filled with
0xA5, must come back untouched.

tests/test_deflate_gen.py (no GPU) checks the same streams on the CPU emulation first, asserts the coverage from the
generator's `stats`, and takes everything that is sent to a device here -- deflate_gen.device_cases() -- through the ASan +
UBSan build of the emulation with the status expected here."""
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.codecs import libpng_decoder as D  # noqa: E402
from tests import deflate_gen as G  # noqa: E402
from tests import png_decode_oracle as O  # noqa: E402
from tests.test_gpu_png_decode import DEV, MIXED, decode_and_check, run_job  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS = [n for n in G.names() if n not in G.IMAGES]                      # the streams whose data is one gray-8 row


def check_rows(rows, expect_status=None):
    """rows: [(zlib stream, the image data's size, the bytes zlib gives)] as one-row files, in batches of at most 64; the oracle's
    BGRA is zlib's bytes, and here they are held against the generator's own data as well"""
    out = []
    for i in range(0, len(rows), 64):
        part = rows[i:i + 64]
        status = None if expect_status is None else expect_status[i:i + 64]
        got, _ = decode_and_check([G.gray_row_file(z, cap) for z, cap, _ in part], status)
        for k, (z, cap, data) in enumerate(part):
            if status is None or status[k] == 0:
                assert np.array_equal(got[k][0, 0:4 * (cap - 1):4], np.frombuffer(data[1:cap], np.uint8)), i + k
        out += got
    return out


def test_the_corpus_inflates_to_zlibs_bytes():
    check_rows([(G.entry(n)[1], len(G.entry(n)[0]), G.entry(n)[0]) for n in ROWS])


def test_reencoded_real_images_decode_like_the_oracle():
    """a foreign parse of real filtered streams, through the un-filter and the expansion: colour type / depth 6/8, 2/16, 3/4, 0/1 and
    4/8, two of them interlaced"""
    decode_and_check([G.image_file(n) for n in sorted(G.IMAGES)])


def test_zlibs_own_streams_of_the_core_tests_run_on_the_device_too():
    """stored, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, forty full-flush blocks, this project's own coder: each behind one stored byte 0"""
    own = G.zlibs_own_streams()
    assert len(own) >= 20 and {"stored", "fixed", "huffman_only", "rle", "many_blocks", "own_coder"} <= set(own)
    check_rows([(z, len(data), data) for z, data in own.values()])


def test_data_beyond_the_size_the_header_needs_is_ignored():
    """the same stream under an IHDR that needs one byte less, half, and a size that ends inside a match and inside a stored block"""
    rows = [(G.entry(n)[1], cap, G.entry(n)[0]) for n in G.SURPLUS for cap in G.surplus_caps(n)]
    assert len(rows) >= 12
    check_rows(rows)


def test_a_wrong_checksum_is_met_only_at_the_exact_size():
    """at the exact size the stream is refused and its frame stays untouched; with one surplus byte the checksum is never reached
    (zlib.decompress, and so the oracle, cannot read this stream: the generator's own data is the yardstick here)"""
    z, data = G.wrong_adler("random_05")
    frames, status = D.decode_png_batch([G.gray_row_file(z, len(data)), G.gray_row_file(z, len(data) - 1)], DEV, fill=0xA5)
    torch.cuda.synchronize()
    assert status == [G.ADLER, 0]
    exact, short = frames[0].to_numpy()[0], frames[1].to_numpy()[0]
    w = len(data) - 2
    assert (exact == 0xA5).all() and short.shape[0] == 1 and (short[:, 4 * w:] == 0xA5).all()
    want = np.frombuffer(data[1:-1], np.uint8)
    assert np.array_equal(short[0, :4 * w].reshape(w, 4), np.stack([want, want, want, np.full(w, 255, np.uint8)], axis=1))


def test_damaged_streams_between_good_neighbours():
    """every refusal of a dynamic header and streams cut at token boundaries, with the statuses of the emulation; a damaged file's
    frame stays untouched, its neighbours are exact"""
    good = [n for n in ROWS if len(G.entry(n)[0]) < 30000]
    rows, status = [], []
    for i, (name, (z, cap, st)) in enumerate(sorted(G.damaged().items())):
        data = G.entry(good[i % len(good)])
        rows += [(data[1], len(data[0]), data[0]), (z, cap, None)]
        status += [0, st]
    rows.append(rows[0])
    status.append(0)
    assert len(set(status)) == 3 and len(rows) >= 40
    check_rows(rows, status)


def test_a_file_gives_the_same_bytes_alone_first_and_last_in_a_batch():
    probe = G.gray_row_file(G.entry("ring_wraps")[1], len(G.entry("ring_wraps")[0]))
    others = [G.gray_row_file(G.entry(n)[1], len(G.entry(n)[0])) for n in ("overlaps", "random_01", "across_blocks")]
    alone, _ = decode_and_check([probe])
    first, _ = decode_and_check([probe] + others)
    last, _ = decode_and_check(others + [probe])
    assert np.array_equal(alone[0], first[0]) and np.array_equal(alone[0], last[-1])


def test_a_job_decodes_a_reencoded_file_and_the_libpng_preset_reproduces_the_pixels():
    data = G.image_file("image_rgba8")
    want, info = O.decode(data)
    outs, r = run_job({0: data}, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": {"libpng": {}}}}])
    got, out_info = O.decode(outs[0])
    assert info["alpha_used"] and out_info["color_type"] == 6 and np.array_equal(got, want)


def test_an_srgb_iccp_that_the_generator_compressed_decodes_like_the_plain_file():
    """the host's use of the same inflate (csrc/png_read.cpp): the profile is a stream of the generator's"""
    from tests.test_jpeg_headers import P3_XYZ, make_icc
    rng = np.random.default_rng(17)
    s = O.random_samples(rng, 60, 40, 2, 8, smooth=True)
    steps = [{"decode": {"io_id": 0}}, {"encode": {"io_id": 9, "preset": "gif"}}]
    want = run_job({0: O.write_png(s, 2, 8, filters=MIXED)}, steps)[0][0]
    for seed in range(4):
        z, stats = G.reencode(make_icc(), random.Random(seed))
        srgb = O.write_png(s, 2, 8, filters=MIXED, ancillary=O.chunk(b"iCCP", b"sRGB\0\0" + z))
        assert D.png_info(srgb)["color_kind"] == D.COLOR_SRGB
        assert run_job({0: srgb}, steps)[0][0] == want
    p3 = O.write_png(s, 2, 8, filters=MIXED, ancillary=O.chunk(b"iCCP", b"P3\0\0" + G.reencode(make_icc(xyz=P3_XYZ), random.Random(1))[0]))
    code, r = run_job({0: p3}, steps, expect=400)
    assert code == 8 and "ICC profile" in r["message"]
