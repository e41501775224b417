"""The device Huffman decoder (csrc/jpeg_entropy.hip) on legal baseline scans that no encoder writes: the crafted corpus of
tests/jpeg_gen.py -- every code 16 bits long, blocks of 1 665 bits across three sub-sequences, sub-sequences without a block
start, a second-level pool that overflows with no hook set, blocks and restart segments around sub-sequence 512 (the write
pass's chunk) and 1 008 (a synchronisation workgroup's own range), a stream on which a decoder off the symbol grid stays off
it -- decoded alone, in batches, in batches of mixed tables, into guarded planes, under the test hooks and in the prepared
form.  The expected coefficients are the WRITER's planes (and the oracle's serial decode, which tests/test_jpeg_gen.py holds to
them): exact equality everywhere; the one numeric bound is rounds <= n_subsequences + 2.

Only entries that the CPU checks accepted (tests/jpeg_gen.device_cases()) reach the device; there are no corrupt streams here."""
from collections import defaultdict

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from imageflow_amd.codecs import mozjpeg_decoder as D  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import jpeg_gen as G  # noqa: E402

DEV = "cuda:0"
LONG_AND_BOUNDARY = ("long_gray", "mixed_gray", "mixed_420", "pool_six_tables_long_444", "ri1_long_420", "bound_512_gray",
                     "bound_1008_gray", "bound_restart_gray", "bound_restart_mixed_gray")
HOOKS = [{"ent_test_inner": "1"}, {"ent_test_inner": "2"}, {"ent_test_pool": "0"}, {"ent_test_pool": "40"}, {"ent_test_pool": "8"},
         {"ent_test_inner": "2", "ent_test_pool": "8"}]


def case(name):
    """an entry the CPU checks let through -> (file, planes, qt, stats)"""
    assert name in G.device_cases(), f"{name} was refused by the CPU checks of tests/test_jpeg_gen.py: it is not sent to a device"
    return G.entry(name)


def as_oracle_input(name):
    """the writer's planes in the form oracle.jpeg_idct_color takes (what oracle.jpeg_read_coefficients returns)"""
    data, planes, qt, st = case(name)
    hs, vs = G.SAMPLING[st["sampling"]]
    n = len(planes)
    coef = [np.ascontiguousarray(planes[c]) if c < n else np.zeros((1, 1, 64), np.int16) for c in range(3)]
    q = np.zeros((3, 64), np.uint16)
    q[:n] = qt
    return dict(width=st["width"], height=st["height"], ncomp=n, hs=list(hs) + [0] * (3 - n), vs=list(vs) + [0] * (3 - n),
                bw=[p.shape[1] for p in planes], bh=[p.shape[0] for p in planes], coef=coef, qt=q)


def assert_coefficients(got, k, name, where=""):
    planes = G.entry(name)[1]
    for c, want in enumerate(planes):
        g = got[c][k].cpu().numpy()
        assert g.shape == want.shape, (name, c, where)
        if not np.array_equal(g, want):
            bad = np.argwhere(g != want)
            raise AssertionError(f"{name} {where} comp {c}: {len(bad)} coefficients differ, first at {bad[0]}: "
                                 f"{g[tuple(bad[0])]} for {want[tuple(bad[0])]}")


def decode(names, **kw):
    ent = D.JpegEntropyBatch([case(n)[0] for n in names], DEV, **kw)
    coef = ent.read_coefficients()
    assert ent.rounds <= ent.n_subsequences + 2, (names[:3], ent.rounds, ent.n_subsequences)
    return ent, coef


@pytest.mark.parametrize("name", G.names())
def test_every_entry_alone(name):
    data, planes, qt, st = case(name)
    ent, coef = decode([name])
    assert (ent.n_subsequences, ent.n_segments, ent.ncomp) == (st["n_sub"], st["segments"], len(planes)), name
    assert np.array_equal(ent.qt[0][:len(planes)], qt), name
    assert_coefficients(coef, 0, name)
    j = O.jpeg_read_coefficients(data)                                    # and the serial decoder, as the older tests hold it
    for c in range(j["ncomp"]):
        assert np.array_equal(coef[c][0].cpu().numpy(), j["coef"][c]), (name, c)


def geometry_groups():
    g = defaultdict(list)
    for name in G.names():
        p = G.CORPUS[name]
        g[(p["w"], p["h"], p["sampling"])].append(name)
    return {k: v for k, v in g.items() if len(v) > 1}


def test_batches_of_equal_geometry():
    groups = geometry_groups()
    assert len(groups) >= 6 and any(len(v) >= 4 for v in groups.values())
    for key, names in groups.items():
        for order in (names, names[::-1]):
            ent, coef = decode(order)
            for k, name in enumerate(order):
                assert np.array_equal(ent.qt[k][:ent.ncomp], G.entry(name)[2]), (key, name)
                assert_coefficients(coef, k, name, f"in the batch of {key}")


@pytest.mark.parametrize("n_files", [40, 300])
@pytest.mark.parametrize("reverse", [False, True])
def test_mixed_tables_in_one_batch(n_files, reverse):
    """Files of one geometry whose tables differ -- the standard ones, all codes 16 bits, a pool that overflows for the last
    component's tables / for its AC table only -- repeated until workgroups span many images: uniform_tables == 0, foreign
    lanes on the global tables, the serial search beside the LDS copy."""
    base = ["mix_std_444", "mix_all16_444", "pool_six_tables_444", "pool_last_ac_444"]
    base = base[::-1] if reverse else base
    names = [base[k % 4] for k in range(n_files)]
    ent, coef = decode(names)
    assert ent.n_subsequences > (1008 if n_files == 300 else 256)
    for c in range(3):
        want = torch.from_numpy(np.stack([G.entry(n)[1][c] for n in base])).to(DEV)
        got = coef[c].view(n_files // 4, 4, *coef[c].shape[1:])
        same = (got == want[None]).flatten(2).all(2)
        assert bool(same.all()), (c, torch.nonzero(~same)[:4].tolist())
    for k in (0, 1, 2, 3, n_files - 1):
        assert np.array_equal(ent.qt[k], G.entry(names[k])[2])


@pytest.mark.parametrize("name", LONG_AND_BOUNDARY)
def test_no_store_lands_behind_a_plane(name):
    """Guard regions of 0x5A5A behind every plane keep their pattern -- also with two files in the batch, so that the first
    file's planes end where the second's begin -- and the coefficients are the writer's."""
    data, planes, qt, st = case(name)
    for n in (1, 2):
        ent = D.JpegEntropyBatch([data] * n, DEV)
        guard = 1 << 16
        coef, bufs = [], []
        for c in range(3):
            shape = (n, max(ent.blocks_h[c], 1), max(ent.blocks_w[c], 1), 64)
            count = int(np.prod(shape))
            buf = torch.full((count + guard,), 0x5A5A, dtype=torch.int16, device=DEV)
            bufs.append((buf, count))
            coef.append(buf[:count].view(shape))
        ent.read_coefficients(coef)
        for c, (buf, count) in enumerate(bufs):
            assert bool((buf[count:] == 0x5A5A).all()), f"{name}: a store landed behind plane {c}"
            if c >= len(planes):
                assert bool((buf == 0x5A5A).all()), f"{name}: a store into the plane of a component the file does not have"
        for k in range(n):
            assert_coefficients(coef, k, name, f"file {k} of {n}")


@pytest.mark.parametrize("hook", HOOKS, ids=lambda h: "-".join(f"{k}={v}" for k, v in h.items()))
def test_rarely_taken_paths_on_crafted_scans(debug_switch, hook):
    """The host-iterated rounds (one or two fixpoint iterations per launch) and the serial code search (a pool of 0 / 40 / 8
    entries) on every crafted entry: the same coefficients."""
    for k, v in hook.items():
        debug_switch(k, v)
    most_rounds = 0
    for name in G.names():
        ent, coef = decode([name])
        most_rounds = max(most_rounds, ent.rounds)
        if name == "slow_sync_gray":
            print(hook, "slow_sync_gray rounds", ent.rounds, "of", ent.n_subsequences)
        assert_coefficients(coef, 0, name, str(hook))
    if "ent_test_inner" in hook:
        assert most_rounds > 100, most_rounds            # slow_sync_gray: the host did iterate, a sub-sequence per round


def test_prepared_form_with_and_without_the_early_upload():
    side = torch.cuda.Stream(DEV)
    for name in ("pool_six_tables_long_444", "bound_restart_mixed_gray", "ri1_long_420"):
        for stream in (None, side, torch.cuda.current_stream(DEV)):
            ent, coef = decode([name, name], prepared=True, upload_stream=stream)
            assert_coefficients(coef, 0, name, f"prepared, stream {stream}")
            assert_coefficients(coef, 1, name, f"prepared, stream {stream}")
    torch.cuda.synchronize()


IN_RANGE = [n for n in G.names() if G.CORPUS[n].get("in_range")]


@pytest.mark.parametrize("name", IN_RANGE)
def test_files_to_bgra(name):
    data = case(name)[0]
    j = as_oracle_input(name)
    assert np.array_equal(D.decode_frames([data], DEV).to_numpy()[0], O.jpeg_idct_color(j)), name
    if G.CORPUS[name]["sampling"] in ("420", "444"):
        got = D.decode_frames([data], DEV, scale_num=4).to_numpy()[0]
        assert np.array_equal(got, O.jpeg_idct_color_scaled(j, 4, 0)), name


def test_slow_synchronisation():
    """`slow_sync_gray`: one segment of 397 sub-sequences in which no speculative decode ever meets the true one, so the true
    state crosses the segment one sub-sequence per fixpoint iteration.  All of it fits one workgroup, whose iteration runs in
    LDS: measured rounds = 1 (MI355X); with one iteration per launch (ent_test_inner 1) 398, with two 200.  Only the
    existing bound is asserted."""
    data, planes, qt, st = case("slow_sync_gray")
    assert st["segments"] == 1 and st["n_sub"] >= 300
    ent, coef = decode(["slow_sync_gray"])
    print("slow_sync_gray rounds", ent.rounds, "of", ent.n_subsequences)
    assert ent.rounds <= ent.n_subsequences + 2, ent.rounds
    assert_coefficients(coef, 0, "slow_sync_gray")
