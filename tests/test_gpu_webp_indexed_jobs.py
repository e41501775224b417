"""The `webplossless` preset of `encode` with the context's stage flags (Context.set_webp_lossless_flags over
ifhip_shim_context_set_webp_lossless_flags, csrc/abi_shim.cpp) on an MI355X: with colour indexing on, a job's few-colour frame
comes out as the emulation's indexed file, in steps and in a graph, and a second job decodes it back; with it off the file is
the plain emulation's; the lossy coder's alpha planes do not see the switch; the querystring's format=webp stays refused."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from imageflow_amd.abi import Context, pack_raw_bgra, unpack_raw_bgra  # noqa: E402
from tests import webp_emulation as PLAIN  # noqa: E402
from tests import webp_frames as F  # noqa: E402
from tests import webp_indexed_emulation as E  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 90, 61
SOURCE = F.few_colours(W, H, n=7)
_EMU = {}


def rows_of(bgra):
    h, w, _ = bgra.shape
    return np.ascontiguousarray(bgra.reshape(h, 4 * w))


def emulated(flags):
    if flags not in _EMU:
        _EMU[flags] = E.encode(SOURCE, True, flags)
    return _EMU[flags]


def _job(form, preset):
    if form == "steps":
        return {"framewise": {"steps": [{"decode": {"io_id": 0}}, {"encode": {"io_id": 1, "preset": preset}}]}}
    return {"framewise": {"graph": {"nodes": {"0": {"decode": {"io_id": 0}}, "1": {"encode": {"io_id": 1, "preset": preset}}},
                                    "edges": [{"from": 0, "to": 1, "kind": "input"}]}}}


def _execute(data, form, preset, indexing=None, lossy=False):
    with Context() as c:
        if indexing is not None:
            assert c.set_webp_lossless_flags(color_indexing=indexing)
        if lossy:
            assert c.set_webp_lossy_encoder(True)
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        status, r = c.send_json("v1/execute", _job(form, preset))
        assert status == 200, (status, r, c.error_message())
        entry = [e for e in r["data"]["job_result"]["encodes"] if e["io_id"] == 1][0]
        return bytes(c.get_output_buffer(1)), entry


@pytest.mark.parametrize("form", ["steps", "graph"])
def test_the_switch_gives_the_indexed_file_and_a_second_job_reads_it_back(form):
    data = pack_raw_bgra(rows_of(SOURCE), W, H, alpha_meaningful=True)
    want, st = emulated(E.COLOR_INDEXING)
    assert st["indexed"] == 1 and st["colours"] == 7
    out, entry = _execute(data, form, "webplossless", indexing=True)
    assert (entry["preferred_mime_type"], entry["preferred_extension"], entry["w"], entry["h"]) == ("image/webp", "webp", W, H)
    assert out == want, "the job's file is the flagged coder's file of the job's pixels"
    got, mode = F.pillow_decode(out)
    assert mode == "RGBA" and np.array_equal(got, F.rgba_of(SOURCE))
    raw, _ = _execute(out, form, "gif")                                  # (the raw BGRA container) the device decoder reads the indexed file
    rows, w, h, alpha = unpack_raw_bgra(raw)
    assert (w, h, alpha) == (W, H, True)
    assert np.array_equal(np.ascontiguousarray(rows[:, :4 * w]).reshape(h, w, 4), SOURCE)


@pytest.mark.parametrize("indexing", [None, False])
def test_without_the_switch_the_file_is_the_plain_one(indexing):
    data = pack_raw_bgra(rows_of(SOURCE), W, H, alpha_meaningful=True)
    out, entry = _execute(data, "steps", "webplossless", indexing=indexing)
    assert out == PLAIN.encode(SOURCE, True)[0] == emulated(0)[0]
    assert len(out) > 2 * len(emulated(E.COLOR_INDEXING)[0]) and entry["preferred_mime_type"] == "image/webp"


def test_the_lossy_coders_alpha_plane_does_not_see_the_switch():
    """a frame whose alpha plane has four levels: indexing would code it smaller, and the lossy coder's files are pinned"""
    frame = F.photo(W, H, seed=95)
    frame[..., 3] = np.array([0, 85, 170, 255], np.uint8)[(np.arange(H)[:, None] // 9 + np.arange(W)[None, :] // 11) % 4]
    data = pack_raw_bgra(rows_of(frame), W, H, alpha_meaningful=True)
    preset = {"webplossy": {"quality": 80.0}}
    off, entry = _execute(data, "steps", preset, indexing=False, lossy=True)
    on, _ = _execute(data, "steps", preset, indexing=True, lossy=True)
    assert off[12:16] == b"VP8X" and b"ALPH" in off and entry["preferred_mime_type"] == "image/webp"
    assert on == off


def test_the_querystrings_format_webp_stays_refused():
    data = pack_raw_bgra(rows_of(SOURCE), W, H, alpha_meaningful=True)
    with Context() as c:
        assert c.set_webp_lossless_flags(color_indexing=True)
        c.add_input_buffer(0, data)
        c.add_output_buffer(1)
        status, _ = c.send_json("v1/execute", {"framewise": {"steps": [{"command_string": {"kind": "ir4", "value": "width=50&format=webp", "decode": 0, "encode": 1}}]}})
        assert status != 200
