"""The CPU restatement of graphics/whitespace.rs (tests/whitespace_oracle.py) against the reference's own stored output
ids, and the properties of its sequential search that a whole-frame reduction does not have.  No GPU needed."""
import numpy as np
import pytest

from imageflow_amd.errors import FlowError
from imageflow_amd.flow.nodes.clone_crop_fill_expand import crop_whitespace_rect
from tests import whitespace_oracle as W
from tests.seahash import bitmap_checksum, checksum_id_digits


def canvas(w, h, bg, rect, color):
    a = np.zeros((h, w, 4), np.uint8)
    a[:] = bg
    x1, y1, x2, y2 = rect
    a[y1:y2, x1:x2] = color
    return a


WHITE, CLEAR = [255, 255, 255, 255], [0, 0, 0, 0]
# visuals/trim.rs:51-129 -> trim.checksums (colours as B, G, R, A of the JSON hex RRGGBBAA)
TRIM_CASES = {
    "blue_dot_trimmed": ((200, 200, WHITE, (80, 80, 120, 120), [255, 0, 0, 255]), 80, 0.0, "d644bbfa1c"),
    "blue_dot_padded_10pct": ((200, 200, WHITE, (80, 80, 120, 120), [0, 0, 255, 255]), 80, 10.0, "3770a32548"),
    "green_on_transparent": ((300, 300, CLEAR, (100, 100, 200, 200), [0, 255, 0, 255]), 1, 0.0, "19ee17aa3e"),
}


@pytest.mark.parametrize("name", list(TRIM_CASES))
def test_restatement_plus_padding_reproduces_the_reference_ids(name):
    spec, thr, pad, want = TRIM_CASES[name]
    src = canvas(*spec)
    x1, y1, x2, y2 = W.crop_whitespace_rect(src, True, thr, pad)
    out = np.ascontiguousarray(src[y1:y2, x1:x2])
    assert checksum_id_digits(out) == want, bitmap_checksum(out)


def test_trim_then_resize_source_is_the_orange_square():
    """visuals/trim.rs:131-158: what the resample of a185811359 reads (tests/reference_canvases.py _trim_source)"""
    src = canvas(400, 400, WHITE, (50, 50, 150, 150), [0x00, 0x55, 0xFF, 0xFF])
    assert W.crop_whitespace_rect(src, True, 80, 0.0) == (50, 50, 150, 150)


def test_windowed_answer_differs_from_the_full_frame_box():
    """The full scan's rectangle is floor(1.0 * (w - 1)) wide and tall (:214-232); on a 700x50 frame its windows
    (292x7, stepping 290x5) end before column 699 and row 49, so a mark there is invisible to the reference -- not to a
    one-pass reduction.  (On narrow frames the 3-px minimum window of :371-372 can still reach the last column.)"""
    src = canvas(700, 50, WHITE, (699, 20, 700, 21), [0, 0, 0, 255])
    assert W.detect_content(src, False, 80) == (0, 0, 700, 50)
    assert W.full_frame_box(src, False, 80) == (699, 20, 700, 21)
    src = canvas(700, 50, WHITE, (10, 49, 11, 50), [0, 0, 0, 255])
    assert W.detect_content(src, False, 80) == (0, 0, 700, 50)
    assert W.full_frame_box(src, False, 80) == (10, 49, 11, 50)


def test_random_frames_differ_from_the_full_frame_box():
    rng = np.random.default_rng(5)
    differ = 0
    for _ in range(60):
        w, h = int(rng.integers(3, 90)), int(rng.integers(3, 90))
        f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        t = int(rng.choice([0, 5, 20, 80, 200]))
        differ += W.detect_content(f, False, t) != W.full_frame_box(f, False, t)
    assert differ > 0


@pytest.mark.parametrize("w,h", [(1, 1), (2, 50), (50, 2), (2, 2)])
def test_frames_below_three_pixels_are_all_content(w, h):
    rng = np.random.default_rng(w * 100 + h)
    assert W.detect_content(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), True, 0) == (0, 0, w, h)    # :288-290


def test_blank_frame_is_all_content():
    assert W.detect_content(canvas(120, 90, WHITE, (0, 0, 1, 1), WHITE), False, 0) == (0, 0, 120, 90)     # :326-333


def test_quick_strips_are_empty_and_the_full_scan_always_runs():
    """Every quick region has x1% == x2% or y1% == y2%, so get_search_rect returns None before any widening (:257-259);
    the box is still empty at the area test, 4wh > wh, and the non-directional full scan is the branch taken."""
    rng = np.random.default_rng(1)
    for w, h in ((3, 3), (7, 9), (200, 100), (3840, 2160)):
        s = W.Search(w, h, 80)
        assert all(s.get_search_rect(r) is None for r in W.QUICK)
        trace = []
        W.detect_content_gray(rng.integers(0, 256, (min(h, 64), min(w, 64)), dtype=np.uint8) if w < 64 else np.full((h, w), 255, np.uint8), 80, trace)
        assert ("branch", "full") in trace


def test_full_scan_windows_are_292_by_7_with_an_overlap_of_two():
    trace = []
    W.detect_content_gray(np.full((100, 700), 255, np.uint8), 80, trace)
    wins = [t[1:] for t in trace if t[0] == "window"]
    assert wins[:3] == [(0, 0, 292, 7), (290, 0, 292, 7), (580, 0, 119, 7)]


def test_grey_formulas():
    px = np.array([[[10, 200, 30, 128], [255, 255, 255, 255]]], np.uint8)
    s = np.array([233 * 10 + 1197 * 200 + 610 * 30, 2040 * 255])
    assert W.approximate_grayscale(px, True).tolist() == [[-(-(s[0] * 128) // 524288), -(-(s[1] * 255) // 524288)]]
    assert W.approximate_grayscale(px, False).tolist() == [[s[0] // 2048, s[1] // 2048]]


def test_node_padding_mirror_matches_the_restatement():
    for rect, pad in (((80, 80, 120, 120), 10.0), ((0, 0, 5, 7), 0.5), ((3, 4, 100, 50), 250.0), ((3, 4, 100, 50), -10.0)):
        try:
            want = W.padded_rect(rect, 120, 90, pad)
        except ValueError:
            want = None
        try:
            got = crop_whitespace_rect(120, 90, rect, pad)
        except FlowError:
            got = None
        assert got == want
    with pytest.raises(FlowError):
        crop_whitespace_rect(120, 90, (10, 10, 9, 20), 0.0)                                # an empty box is InvalidState
