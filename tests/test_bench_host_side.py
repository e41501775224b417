"""Host-side pieces of bench.py and of the round-6 tools that need no GPU: the CPU count the baselines run on, the entropy
stage's issue yardstick (symbols from the host scan walk x the committed instruction model), and the enumeration behind DESIGN
section 4.1's "a fifth wave per SIMD adds no working lanes"."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_usable_cpus_is_a_count_this_process_may_use():
    import bench
    n = bench.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)


def test_entropy_issue_yardstick_from_a_file_and_the_committed_model():
    import bench
    f = bench._cfg4_one_file(0)                                    # a 3840x2160 4:2:0 q85 gradient file, as the cfg4 workload writes it
    r = bench.cfg4_entropy_roofline([f], 4, 0.5)                   # "4 such files decoded in 0.5 ms"
    assert r["bound"] == "issue" and r["walks"] == 4 and r["sampled_files"] == 1
    assert 1_200_000 * 4 < r["symbols"] < 1_500_000 * 4 and 0.6 < r["table_reads_per_symbol_with_pair_entries"] < 0.9
    assert r["lane_steps"]["round"] == 2 * r["lane_steps"]["count"] and r["lane_steps"]["write"] == r["symbols"]
    # frac = VALU issue cycles of the walks on 1 024 SIMD-32s at 2.4 GHz / the time given
    per = json.load(open(os.path.join(ROOT, "profiles", "entropy_issue_model.json")))["per_64_lane_steps"]
    cycles = sum(per[k]["valu"] * r["lane_steps"][k] / 64.0 for k in ("round", "count", "write")) * 2.0
    assert abs(r["frac"] - cycles / (1024 * 2.4e9) / 0.5e-3) < 2e-4
    assert abs(r["achieved"] / r["peak"] - r["frac"]) < 2e-3
    # the stage's compulsory HBM traffic: the coefficient planes of 4 files + the scans read by three kernels, in the time given
    h = r["hbm"]
    assert 4 * 24_883_200 < h["bytes"] < 4 * 24_883_200 + 3 * 4 * len(f) * 1.1
    assert abs(h["frac"] - h["bytes"] / 8e12 / 0.5e-3) < 2e-4 and abs(h["achieved"] / h["peak"] - h["frac"]) < 2e-3


def test_no_cut_with_the_encode_table_adds_busy_lanes_at_twenty_waves_per_cu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "five_waves_feasibility.py")], capture_output=True, text=True, check=True).stdout
    rows = [json.loads(ln) for ln in out.splitlines()]
    today = {r["shape"]: r["product_today_busy_lanes_per_cu"] for r in rows if "summary" in r}
    assert len(today) == 4
    for r in rows:
        if "summary" in r or r["tables"] != "with the encode table" or r["waves_per_cu"] < 20:
            continue
        assert r["busy_lanes_per_cu"] <= today[r["shape"]] * 1.01, r
    committed = open(os.path.join(ROOT, "profiles", "r6_five_waves_feasibility.jsonl")).read()
    assert committed == out                                        # the file under profiles/ is what the tool prints today


def test_options_of_a_plain_run_and_of_a_full_one():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--steps", "2", "--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        try:
            bench.parse_args(bad)
        except SystemExit as e:
            assert e.code == 2
        else:
            raise AssertionError(bad)


def test_bgra_frames_cuts_the_stride_padding():
    import torch
    import bench
    from imageflow_amd.graphics.bitmaps import Bitmap, get_stride
    n, w, h = 3, 5, 4
    st = get_stride(w)
    data = torch.arange(n * h * st, dtype=torch.int64).remainder(251).to(torch.uint8).view(n, h * st)
    got = bench.bgra_frames(Bitmap(data, w, h, st))
    assert got.shape == (n, h, w, 4)
    assert torch.equal(got.reshape(n, h, 4 * w), data.view(n, h, st)[:, :, :4 * w])


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import numpy as np
    import torch
    import bench
    a = torch.arange(10 * 6, dtype=torch.int32).view(10, 6).to(torch.uint8)
    b = torch.arange(10, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "all"), {"a": a, "b": b})
    assert np.array_equal(np.load(tmp_path / "all" / "a.npy"), a.numpy().astype(np.float32))
    assert np.load(tmp_path / "all" / "b.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "all" / "frame_index.npy"), np.arange(10.0))
    # over the budget: the same seeded sample of frames from every array, every time
    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 20) + 4 * 7 * 3)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    idx = np.load(tmp_path / "s1" / "frame_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 3 and list(idx) == sorted(set(idx))
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "frame_index.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "a.npy"), a.numpy()[idx.astype(int)].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "s1" / "b.npy"), idx.astype(np.float32))
