#!/usr/bin/env python3
"""The device WebP decoder on batches of files (tools/bench_webp_decode.py [--case NAME] [--reps N]).  Cases: 1, 8 and 32
files of the 800x450 photo-like test frames and one 3840x2160 file -- every file once as the device coder of
csrc/webp_encode.hip wrote it and once as libwebp wrote it (Pillow, lossless, quality 70, method 4: cross-colour, other tile
sizes).  Per case one JSON line: the whole call (host container walk and prepare, upload, the token loop and the transform
steps, wait) for the batch, the stages by difference (the development switch webp_decode_stop_after ends the call behind the
token loop), the host prepare alone, and the yardstick: one host core's libwebp through Pillow on the same files in the same run.

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
sys.path.insert(0, os.path.join(ROOT, "tools"))

# n, w, h, reps, time limit s
CASES = {"800x450x1": (1, 800, 450, 3, 200), "800x450x8": (8, 800, 450, 3, 200), "800x450x32": (32, 800, 450, 3, 300), "2160p_x1": (1, 3840, 2160, 1, 600)}


def run_case(name, reps=None):
    import numpy as np
    import torch
    from PIL import Image
    from imageflow_amd import _native
    from imageflow_amd.codecs import webp_decoder as D
    from imageflow_amd.codecs import webp_encoder as E
    from imageflow_amd.graphics.bitmaps import Bitmap
    from bench_png_encode import photo_frames
    n, w, h, default_reps, _ = CASES[name]
    reps = reps or default_reps
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    bm = Bitmap(photo_frames(n, w, h, stride, dev, True), w, h, stride, alpha_meaningful=True)
    want = bm.data.view(n, h, stride)[:, :, :4 * w].cpu().numpy()
    device_files = E.encode_webp_lossless(bm)
    libwebp_files = []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(want[i].reshape(h, w, 4)[..., [2, 1, 0, 3]]), "RGBA").save(buf, "WEBP", lossless=True, quality=70, method=4, exact=True)
        libwebp_files.append(buf.getvalue())
    res = {"case": name, "files": n, "w": w, "h": h, "reps": reps, "device": torch.cuda.get_device_name(0)}
    for label, files in (("device_coder", device_files), ("libwebp", libwebp_files)):
        frames = [Bitmap(torch.zeros((1, h * stride), dtype=torch.uint8, device=dev), w, h, stride, True) for _ in range(n)]

        def timed(call, stop=None, reps=reps):
            _native.debug_set("webp_decode_stop_after", stop)
            if reps > 1:
                call()                                               # warm-up
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            _native.debug_set("webp_decode_stop_after", None)
            print(f"  {name} {label} {call.__name__} stop_after={stop}: {np.median(ts):.3f} ms", file=sys.stderr, flush=True)
            return float(np.median(ts))

        def batch():
            _, st = D.decode_webp_batch(files, dev, frames=frames)
            assert not any(st), st
        whole = timed(batch)
        got = torch.stack([f.data.view(h, stride)[:, :4 * w] for f in frames]).cpu().numpy()
        assert np.array_equal(got, want), "decoded frames differ from the source"
        t_pixels = timed(batch, "pixels")
        ts = []
        for _ in range(max(3, reps)):
            t0 = time.perf_counter()
            for f in files:
                im = Image.open(io.BytesIO(f))
                im.load()
            ts.append((time.perf_counter() - t0) * 1e3)
        host = float(np.median(ts))
        res[label] = {"file_bytes": sum(len(f) for f in files), "batch_ms": round(whole, 3), "token_loop_with_host_part_ms": round(t_pixels, 3),
                      "transforms_ms": round(whole - t_pixels, 3), "host_libwebp_one_core_ms": round(host, 3), "batch_over_host": round(whole / host, 2),
                      "MPps": round(n * w * h / 1e6 / (whole * 1e-3), 2)}
    print(json.dumps(res), flush=True)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else None
    if "--case" in sys.argv:
        run_case(sys.argv[sys.argv.index("--case") + 1], reps)
        return 0
    for name, (_, _, _, _, limit) in CASES.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name] + (["--reps", str(reps)] if reps else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:                                                   # a fault, an abort or the time limit: nothing more runs on this device
            print(json.dumps({"case": name, "exit_status": rc, "stopped": True}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
