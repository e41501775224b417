"""bench.py as it is run for every change: a plain run prints the headline line and none of what --full adds, and
--dump-outputs writes what the last timed step computed -- bytes equal to the CPU oracle's on the same inputs, and the same
whether or not the run was --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import util as U  # noqa: E402


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_and_its_dumped_outputs(tmp_path):
    import bench
    from imageflow_amd.graphics.bitmaps import BitmapCompositing
    from imageflow_amd.graphics.weights import Filter
    common = ["--gpus", "1", "--frames", "2", "--total-frames", "8", "--warmup", "1"]
    plain = _bench(common + ["--steps", "3", "--dump-outputs", str(tmp_path / "plain")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["unit"] == "MP/s"
    for k in ("roofline", "parity_checked", "strong_1024", "cpu_baseline", "host_dropin", "other_configs"):
        assert k not in plain, k
    got = np.load(tmp_path / "plain" / "canvas.npy")
    assert got.dtype == np.float32 and got.shape == (2, 200, 200, 4)
    assert np.array_equal(np.load(tmp_path / "plain" / "frame_index.npy"), [0.0, 1.0])

    # the same inputs in a --full run (its strong_1024 job makes all 8 frames): the same outputs, and its parity stamp
    full = _bench(common + ["--steps", "2", "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    assert full["parity_checked"]["equal"] is True and full["roofline"]["frac"] > 0 and full["strong_1024"]["frames_per_gpu"] == 8
    assert np.array_equal(np.load(tmp_path / "full" / "canvas.npy"), got)

    # and the bytes are the CPU oracle's on frames made the way bench.py makes them
    fr = bench.make_frames(torch, 2, 0, 0, "cpu", "mixed", 3840, 2160, random_from=4)
    for i in range(2):
        src = fr.data[i].numpy().reshape(1, 2160, fr.stride)
        exp = np.zeros((1, 200, U.stride_for(200)), np.uint8)
        U.oracle_render(src, 3840, 2160, exp, 200, 200, 0, 0, 200, 200, filter_id=int(Filter["Robidoux"]),
                        compositing=int(BitmapCompositing.ReplaceSelf), matte_bgra=0, alpha_meaningful=False)
        assert np.array_equal(got[i].astype(np.uint8), exp[0][:, :800].reshape(200, 200, 4)), i
