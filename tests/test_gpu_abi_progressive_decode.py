"""Jobs with the device progressive JPEG decoder switched on (Context.set_device_progressive_decoder, csrc/shim_decode.cpp):
`decode -> resample_2d -> encode` on a Pillow progressive file and on a file of this library's own `mozjpeg` preset returns
the bytes of the same job with the switch off, and the context's counter shows the device path; a script the front end
refuses and a file damaged inside a scan give the switch-off answer -- bytes or error -- and the counter shows the
fall-back; with the switch off both counters stay zero."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd.abi import Context  # noqa: E402
from tests import jpeg_prog_fixtures as X  # noqa: E402
from tests import jpeg_prog_gen as G  # noqa: E402

STEPS = [{"decode": {"io_id": 0}}, {"resample_2d": {"w": 40, "h": 30, "hints": {"down_filter": "robidoux", "up_filter": "robidoux"}}},
         {"encode": {"io_id": 1, "preset": {"libjpeg_turbo": {"quality": 90}}}}]


def run_job(data, on, steps=STEPS):
    """-> (status, output bytes or (error code, message), (device decodes, fall-backs))"""
    with Context() as c:
        if on:
            assert c.set_device_progressive_decoder(True)
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", {"framewise": {"steps": steps}})
        counts = c.device_progressive_decodes()
        if status != 200:
            return status, (c.error_code(), c.error_message()[0]), counts
        return status, c.get_output_buffer(1), counts


def mozjpeg_preset_file():
    pixels = X.save(X.image(160, 120, 7), quality=95)
    status, out, _ = run_job(pixels, False, [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": {"mozjpeg": {"quality": 80}}}}])
    assert status == 200 and b"\xff\xc2" in out, "the mozjpeg preset writes progressive files"
    return out


def test_jobs_return_the_same_bytes_and_count_the_device_path():
    for name, data in (("pillow", X.pillow_files()["pillow_321x203_420_q30_rst0"]), ("pillow restarts", X.pillow_files()["pillow_100x75_422_q90_rst3"]),
                       ("mozjpeg preset", mozjpeg_preset_file()), ("corpus", G.entry("odd_24x24_420")[0])):
        s0, off, n0 = run_job(data, False)
        s1, on, n1 = run_job(data, True)
        assert s0 == s1 == 200, name
        assert on == off and len(on) > 100, name
        assert n0 == (0, 0) and n1 == (1, 0), (name, n0, n1)


def test_a_refused_script_and_a_damaged_file_fall_back_to_the_host_reader():
    damaged = X.damaged_files()
    emu = dict(zip(sorted(damaged), X.emulate_batch([damaged[n] for n in sorted(damaged)])))
    bad = [n for n in sorted(damaged) if emu[n][0] == 0 and emu[n][1] != 0]
    refused = G.refused()
    cases = [("refused script", refused["band_over_two_al"]), ("sequential multi-scan", refused["sequential_two_scans"])]
    cases += [(n, damaged[n]) for n in bad[:4]]
    answers = set()
    for name, data in cases:
        s0, off, n0 = run_job(data, False)
        s1, on, n1 = run_job(data, True)
        assert s0 == s1 and on == off, (name, s0, s1)
        assert n0 == (0, 0) and n1 == (0, 1), (name, n0, n1)
        answers.add(s0)
    assert 200 in answers                       # (the host reader decodes the refused scripts; what it makes of a damaged file is its own verdict)


def test_a_baseline_file_never_reaches_the_switch():
    data = X.save(X.image(64, 48, 3), quality=80)
    s0, off, n0 = run_job(data, False)
    s1, on, n1 = run_job(data, True)
    assert s0 == s1 == 200 and on == off and n0 == n1 == (0, 0)
