"""tests/gif_gen.py checked against Pillow's decoder byte for byte: every class of LZW stream the GIF corpus uses -- clears
anywhere, none at all, two in a row, no leading clear, no end code, bytes behind it -- decodes in Pillow to the indices that
went in.  The classes Pillow itself refuses are NAMED below, each with the sentence of GIF89a that makes it legal; they are
checked against the oracle alone.  Nothing is skipped silently: a good file that Pillow refuses and that is not on the list
fails this test."""
import io

import numpy as np
import pytest

from tests import gif_fixtures as X
from tests import gif_gen as G
from tests import gif_oracle as O

PIL = pytest.importorskip("PIL.Image")

# name prefix -> why the file is legal although Pillow 12 refuses it
PILLOW_REFUSES = {
    "m1_": "GIF89a appendix F: 'the first byte of the Compressed Data stream is a value indicating the minimum number of bits required to "
           "represent the set of actual pixel values' -- one bit for two colours; the advice to write 2 for bilevel images binds encoders. "
           "Pillow reads such a stream with other code widths and reports a truncated file.",
    "zero_size_frame": "GIF89a section 20: Image Width and Height are 'in pixels', 0..65535, with no lower bound; the reference pins such a file "
                       "(tests/crash_repro/gif_zero_size_frame.gif).  Pillow refuses to build an image without pixels.",
    "frame_beyond_the_corner": "GIF89a section 20: Image Left / Top Position are 16-bit unsigned column and row numbers with no upper bound but the field's; "
                               "the reference clips such a frame to the canvas (gif/screen.rs:59-63, tests/crash_repro/gif_overflow_frame_pos.gif).  "
                               "Pillow grows its canvas to hold the frame and refuses the size.",
}
SINGLE = sorted(n for n, (_, target) in X.good_files().items() if target == 0 and O.parse(X.good_files()[n][0], 8)["frames_seen"] == 1)


def pillow_first_frame(data):
    im = PIL.open(io.BytesIO(data))
    im.load()
    return im


@pytest.mark.parametrize("name", SINGLE)
def test_every_single_frame_file_decodes_in_pillow_to_what_went_in(name, monkeypatch):
    monkeypatch.setattr(PIL, "MAX_IMAGE_PIXELS", 89478485)                # Pillow's own default, whatever another test module left there
    data, _ = X.good_files()[name]
    P = O.parse(data)
    fr = P["frames"][0]
    st, idx = O.frame_indices(fr)
    assert st == O.OK
    listed = [k for k in PILLOW_REFUSES if name.startswith(k)]
    try:
        im = pillow_first_frame(data)
    except Exception as e:                                                # noqa: BLE001
        assert listed, (name, repr(e))
        return
    assert not listed, "Pillow reads %s: take it off the list" % name
    if (fr["w"], fr["h"], fr["left"], fr["top"]) != (P["w"], P["h"], 0, 0) or fr["transparent"] is not None:
        return                                                             # (Pillow composes such a frame itself: the screens are the oracle's business)
    assert im.mode in ("P", "L")
    assert np.array_equal(np.asarray(im), idx), name


def test_the_writer_is_seeded():
    assert X.good_files.__wrapped__()["m5_noise"] == X.good_files()["m5_noise"]
    assert G.width_at(8, 0) == 9 and G.width_at(8, 254) == 9 and G.width_at(8, 255) == 10 and G.width_at(8, 3838) == 12 and G.width_at(8, 100000) == 12
    assert G.width_at(2, 0) == 3 and G.width_at(2, 2) == 3 and G.width_at(2, 3) == 4


def test_the_corpus_holds_the_streams_it_is_there_for():
    def tokens(name):
        fr = O.parse(X.good_files()[name][0])["frames"][0]
        m, acc, pos, k, out = fr["m"], int.from_bytes(fr["stream"], "little"), 0, 0, []
        while pos + G.width_at(m, k) <= len(fr["stream"]) * 8:
            w = G.width_at(m, k)
            c = (acc >> pos) & ((1 << w) - 1)
            pos += w
            if c == 1 << m:
                out.append(("clear", k))
                k = 0
                continue
            if c == (1 << m) + 1:
                out.append(("end", k))
                break
            k += 1
        else:
            out.append(("ran_out", k))
        return out
    t = tokens("deferred_m8_long_tail")
    assert [x[0] for x in t] == ["clear", "end"] and t[1][1] > 3838 + 2 * 4096          # one segment, a tail of more than two chunks
    t = tokens("widths_m8_clear_at_full")
    assert len(t) > 3 and all(k == 3839 for kind, k in t[1:-1])                        # a clear exactly when the table is full
    assert [k for _, k in tokens("clear_at_64")[1:4]] == [64, 64, 64]
    assert tokens("end_at_65") == [("clear", 0), ("end", 65)]
    assert tokens("two_clears_in_a_row")[1:3] == [("clear", 700), ("clear", 0)]
    assert tokens("no_leading_clear")[0][1] > 0
    assert tokens("no_end_code")[-1][0] == "ran_out"
    assert tokens("clear_at_5121")[1] == ("clear", 5121)
    assert tokens("flat_kwkwk_chain")[-1][1] < 400                                     # 60 000 pixels in a few hundred codes: chains hundreds long
