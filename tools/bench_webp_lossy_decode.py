#!/usr/bin/env python3
"""The device lossy WebP decoder on batches of files (tools/bench_webp_lossy_decode.py [--case NAME] [--reps N]).  Cases: one
800x450 quality-75 file, 32 of them in one batch, the RGBA variant of that file (an ALPH chunk), and one lone 3840x2160 file,
all written by libwebp through Pillow.  Per case one JSON line, wall clock after a warm-up: the whole call with its wait; the
host stage (container walk, bool-decoding, staging and the upload the call waits for) together with the residual kernel, and the
other device stages by difference (the development switch vp8_decode_stop_after ends the call behind a
kernel); and the yardstick: one host core's libwebp through Pillow on the same files in the same run.

Without --case every case runs as a child process of its own under `timeout -k 10`, one after the other, and the first
that fails ends the run: nothing more is started on a device that has just faulted or hung."""
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# files, w, h, alpha, reps, time limit s
CASES = {"800x450x1": (1, 800, 450, False, 5, 200), "800x450x32": (32, 800, 450, False, 5, 300), "800x450_rgba_x1": (1, 800, 450, True, 5, 200),
         "2160p_x1": (1, 3840, 2160, False, 3, 600)}


def photo(w, h, seed, alpha):
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [128 + 90 * np.sin(x / (37.0 + 9 * k) + k + seed) * np.cos(y / (41.0 - 6 * k)) + 25 * ((x // 64 + y // 48) % 2) + rng.normal(0, 4, (h, w)) for k in range(3)]
    if alpha:
        planes.append(255 - 60 * (1 + np.sin(x / 90.0 + y / 70.0)))
    return np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)


def run_case(name, reps=None):
    import numpy as np
    import torch
    from PIL import Image
    from imageflow_amd import _native
    from imageflow_amd.codecs import webp_lossy_decoder as D
    from imageflow_amd.graphics.bitmaps import Bitmap
    n, w, h, alpha, default_reps, _ = CASES[name]
    reps = reps or default_reps
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    files, want = [], []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(photo(w, h, i, alpha), "RGBA" if alpha else "RGB").save(buf, "WEBP", quality=75, method=4)
        files.append(buf.getvalue())
    for f in files[:2]:
        want.append(np.asarray(Image.open(io.BytesIO(f)).convert("RGBA"))[..., [2, 1, 0, 3]])
    frames = [Bitmap(torch.zeros((1, h * stride), dtype=torch.uint8, device=dev), w, h, stride, alpha) for _ in range(n)]

    def batch():
        t0 = time.perf_counter()
        _, st = D.decode_webp_lossy_batch(files, dev, frames=frames)          # (reads the status words back: the device part is over)
        assert not any(st), st
        return (time.perf_counter() - t0) * 1e3

    def timed(stop=None):
        _native.debug_set("vp8_decode_stop_after", stop)
        batch()                                                           # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            batch()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        _native.debug_set("vp8_decode_stop_after", None)
        print(f"  {name} stop_after={stop}: {np.median(ts):.3f} ms", file=sys.stderr, flush=True)
        return float(np.median(ts))

    whole = timed()
    for i, wnt in enumerate(want):
        got = frames[i].data.view(h, stride)[:, :4 * w].cpu().numpy().reshape(h, w, 4)
        assert np.array_equal(got, wnt), "decoded frame differs from libwebp's"
    stages = {s: timed(s) for s in ("residual", "predict", "filter")}
    # (the call that stops behind its first kernel is the host stage -- walk, bool-decoding, staging, the upload it waits for -- plus the residual kernel)
    ts = []
    for _ in range(max(3, reps)):
        t0 = time.perf_counter()
        for f in files:
            im = Image.open(io.BytesIO(f))
            im.load()
        ts.append((time.perf_counter() - t0) * 1e3)
    host = float(np.median(ts))
    res = {"case": name, "files": n, "w": w, "h": h, "alpha": alpha, "reps": reps, "device": torch.cuda.get_device_name(0), "file_bytes": sum(len(f) for f in files),
           "whole_call_ms": round(whole, 3), "host_stage_upload_and_residuals_ms": round(stages["residual"], 3),
           "predict_ms": round(stages["predict"] - stages["residual"], 3), "loop_filter_ms": round(stages["filter"] - stages["predict"], 3),
           "alpha_and_bgra_ms": round(whole - stages["filter"], 3), "host_libwebp_one_core_ms": round(host, 3), "call_over_host": round(whole / host, 2),
           "MPps": round(n * w * h / 1e6 / (whole * 1e-3), 2)}
    print(json.dumps(res), flush=True)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else None
    if "--case" in sys.argv:
        run_case(sys.argv[sys.argv.index("--case") + 1], reps)
        return 0
    for name, case in CASES.items():
        cmd = ["timeout", "-k", "10", str(case[-1]), sys.executable, os.path.abspath(__file__), "--case", name] + (["--reps", str(reps)] if reps else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:                                                   # a fault, an abort or the time limit: nothing more runs on this device
            print(json.dumps({"case": name, "exit_status": rc, "stopped": True}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
