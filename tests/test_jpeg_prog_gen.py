"""tests/jpeg_prog_gen.py, the seeded writer of progressive JPEG files no encoder writes: what the corpus covers (asserted from
the writer's `stats`), the host reader (csrc/jpeg_read.cpp) returns the writer's planes for every file, and a pin to
libjpeg-turbo: Pillow decodes each file to the pixels of the baseline file this library's writer codes from the same planes."""
import ctypes as C
import io

import numpy as np
import pytest

from imageflow_amd import _native
from tests import jpeg_prog_fixtures as X
from tests import jpeg_prog_gen as G

NAMES = G.names()


def union(key):
    out = set()
    for name in NAMES:
        out |= G.entry(name)[3][key]
    return out


def total(key):
    return sum(G.entry(name)[3][key] for name in NAMES)


def most(key):
    return max(G.entry(name)[3][key] for name in NAMES)


def test_the_corpus_holds_the_sizes():
    a = {name: CORPUS_ARGS(name) for name in G.names(big=False)}
    sizes = {(v[0], v[1], v[2]) for v in a.values()}
    assert (8, 8, "gray") in sizes and (16, 16, "420") in sizes
    for samp in ("420", "422", "440", "444"):
        assert (24, 24, samp) in sizes and (17, 9, samp) in sizes
    assert all(v[0] <= 64 and v[1] <= 48 for v in a.values())
    assert total("padded_blocks_coded") > 0 and total("padded_blocks_skipped") > 0


def CORPUS_ARGS(name):
    return G.CORPUS[name][0]


def test_the_corpus_holds_the_scan_scripts():
    assert union("kinds") == {"dc_first", "dc_refine", "ac_first", "ac_refine"}
    assert total("one_component_dc_in_color") >= 3
    assert most("max_dc_al") == 3 and most("refinement_depth") == 3
    assert total("single_index_bands") >= 2
    assert most("dc_only_components") == 1
    assert most("first_scans_at_level0") >= 2 and most("levels") >= 4
    st = G.entry("odd_17x9_420")[3]
    assert st["max_dc_al"] == 3 and st["refinement_depth"] == 3 and st["dc_only_components"] == 1 and st["first_scans_at_level0"] >= 2


def test_the_corpus_holds_the_end_of_band_runs():
    assert total("eobrun_spans_rows") > 0 and total("eobrun_cut_by_restart") > 0 and total("eob0") > 0
    assert G.entry("eob_run_1024x1024_gray")[3]["max_eobrun"] >= 1 << 14
    assert len(G.entry("eob_run_1024x1024_gray")[0]) < 20000
    assert total("eobrun_with_corrections") > 0 and total("corrections_inside_eobrun") > 0


def test_the_corpus_holds_the_refinement_cases():
    assert most("max_corrections_in_block") == 63
    assert total("zrl_over_history") > 0 and total("new_coefficient_at_63") > 0 and total("all_correction_blocks") > 0


def test_the_corpus_holds_the_restarts_and_the_stream_shapes():
    assert union("restart_kinds") == {"dc_first", "dc_refine", "ac_first", "ac_refine"}
    assert 1 in union("intervals") and len(union("intervals")) >= 4
    assert total("dri_changes") > 0 and total("fill_bytes") > 0
    assert union("pads") == {"ones", "zeros", "noise"}
    st = G.entry("all16_24x24_420")[3]
    assert st["min_code_len"] == st["max_code_len"] == 16 and st["table_redefinitions"] > 0
    # a stream longer than the kernel's stage (csrc/jpeg_progressive_core.hpp kProgStageWords, read back from the emulation)
    rc, facts = X.emu_prepare(G.entry("long_stream_64x48_444")[0])
    assert rc == 0 and facts["stage_words"] * 32 == G.STAGE_BITS
    assert G.entry("long_stream_64x48_444")[3]["max_stream_bits"] > G.STAGE_BITS and facts["max_stream_bits"] > G.STAGE_BITS


def test_the_quantisation_tables_are_the_writers():
    L = _native.lib()
    L.ifhip_jpeg_quality_tables.argtypes = [C.c_int, C.c_void_p]
    qt = np.zeros((2, 64), np.uint16)
    _native.check(L.ifhip_jpeg_quality_tables(G.QUALITY, qt.ctypes.data))
    assert np.array_equal(qt, np.stack(G.quality_tables(G.QUALITY)))


@pytest.mark.parametrize("name", NAMES)
def test_the_host_reader_returns_the_writers_planes(name):
    data, planes, qt, _ = G.entry(name)
    rc, got, got_qt = X.host_read(data)
    assert rc == 0
    assert len(got) == len(planes)
    for c in range(len(planes)):
        assert got[c].shape == planes[c].shape and np.array_equal(got[c], planes[c]), (name, c)
        assert np.array_equal(got_qt[c], qt[c])


def baseline_twin(name):
    data, planes, qt, _ = G.entry(name)
    w, h, samp = G.CORPUS[name][0][:3] if name in G.CORPUS else (1024, 1024, "gray")
    geo = G.geometry(w, h, samp)
    n = geo["ncomp"]
    L = _native.lib()
    L.ifhip_jpeg_write.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                                       C.c_size_t, C.POINTER(C.c_size_t)]
    bw, bh = np.array(geo["bw"] + [0] * (3 - n), np.uint32), np.array(geo["bh"] + [0] * (3 - n), np.uint32)
    hs, vs = np.array(list(geo["hs"]) + [0] * (3 - n), np.uint8), np.array(list(geo["vs"]) + [0] * (3 - n), np.uint8)
    coef = [np.ascontiguousarray(p) for p in planes]
    ptr = [coef[c].ctypes.data if c < n else None for c in range(3)]
    buf, size = np.zeros(4 << 20, np.uint8), C.c_size_t()
    _native.check(L.ifhip_jpeg_write(ptr[0], ptr[1], ptr[2], bw.ctypes.data, bh.ctypes.data, n, hs.ctypes.data, vs.ctypes.data, w, h,
                                     G.QUALITY, 0, buf.ctypes.data, buf.size, C.byref(size)))
    return buf[:size.value].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_pillow_decodes_every_file_to_the_pixels_of_its_baseline_twin(name):
    Image = pytest.importorskip("PIL.Image")
    prog = np.asarray(Image.open(io.BytesIO(G.entry(name)[0])))
    base = np.asarray(Image.open(io.BytesIO(baseline_twin(name))))
    assert prog.shape == base.shape and np.array_equal(prog, base), name


def test_the_refused_files_are_what_they_say():
    r = G.refused()
    assert set(r) >= {"refinement_before_first_scan", "two_first_scans_of_one_band", "band_over_two_al", "sequential_two_scans"}
    assert b"\xff\xc0" in r["sequential_two_scans"] and r["sequential_two_scans"].count(b"\xff\xda") == 2
    assert X.host_read(r["sequential_two_scans"])[0] == 0             # the host reader takes sequential multi-scan files
