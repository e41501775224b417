"""The JPEG host front end -- the marker walk and segment readers of csrc/jpeg_markers.hpp under parse_jpeg, the EXIF and ICC
readers (csrc/jpeg_parse.cpp) and read_jpeg (csrc/jpeg_read.cpp) -- against the answers recorded in
tests/golden/jpeg_marker_results.json: return code, message and a digest of every output buffer of every host entry point,
for every file of tests/golden/make_jpeg_marker_golden.py's corpus (whole files, seeded mutations, hand-made refusals).  And
the header alone, in a program of its own, over the same bytes under the host sanitizers."""
import importlib.util
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_jpeg_marker_golden", os.path.join(HERE, "golden", "make_jpeg_marker_golden.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return M


@pytest.fixture(scope="module")
def corpus():
    M = _generator()
    return M, M.corpus()


def test_every_entry_point_answers_as_recorded(corpus):
    M, cases = corpus
    recorded = M.load_recorded(cases)
    L = M.library()
    results = {}
    for name, data in cases:
        results[name] = M.answers(L, data)
        got = [results[name][ep] for ep in M.ENTRY_POINTS]
        if got != recorded[name]:
            diff = [(ep, w, g) for ep, w, g in zip(M.ENTRY_POINTS, recorded[name], got) if w != g]
            raise AssertionError(f"{name}: " + "; ".join(f"{ep} recorded {w!r}, now {g!r}" for ep, w, g in diff))
    M.check_conditions(cases, results)                          # every refusal text is still reached, the mutations still bite


def test_marker_header_alone_under_the_host_sanitizers(corpus, tmp_path):
    """tests/jpeg_markers_sanitize.cpp drives the stepper and every segment reader over every case the way the strict and the
    lenient walks do; ASan + UBSan abort on the first bad read.  Its counts of accepted frames are the library's own."""
    M, cases = corpus
    exe, blob = str(tmp_path / "jpeg_markers_sanitize"), str(tmp_path / "cases.bin")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(HERE, "..", "imageflow_amd", "csrc"), os.path.join(HERE, "jpeg_markers_sanitize.cpp"), "-o", exe]
    probe = subprocess.run(cmd[:-3] + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime links here: " + probe.stderr.strip().splitlines()[-1])
    subprocess.run(cmd, check=True)
    M.write_sanitizer_corpus(blob, cases)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    files, parse_ok, read_ok, lenient_segments, _ = (int(v) for v in r.stdout.split())
    assert files == len(cases) and lenient_segments > files
    recorded = M.load_recorded(cases)
    # the frames the stand-alone strict walks take are the ones the library's take: the same walk, the same questions
    for ep, ok in (("parse_headers", parse_ok), ("frame_info", read_ok)):
        assert ok == sum(v[M.ENTRY_POINTS.index(ep)].startswith("0:") for v in recorded.values()), ep
