#!/usr/bin/env python3
"""Time ifhip_detect_content_batch_device (csrc/whitespace.hip): codes pass + replay pass, per call, on

  border   a batch of 3840x2160 product shots (content inside a white border)
  corners  one 3840x2160 frame whose content lies only in the corners
  single   single-frame latency, host-timed, including the 16-byte download of the rectangle

Prints one JSON line per case: device ms per call (hipEvents around `--iters` back-to-back calls), and what the codes pass
reads and writes by algorithmic bytes (4 B read + 1 B written per pixel) as a fraction of 8 TB/s if the whole call took
that long -- a lower bound on the codes pass's own fraction.  The per-pass split comes from a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_whitespace.py).

    python tools/bench_whitespace.py [--batch 8] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from imageflow_amd.graphics.whitespace import detect_content_into  # noqa: E402

W, H = 3840, 2160
HBM = 8e12


def frames(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    stride = 4 * W
    out = np.full((n, H, W, 4), 255, np.uint8)
    for i in range(n):
        if kind == "border":
            out[i, H // 8:H - H // 6, W // 7:W - W // 9] = rng.integers(0, 256, (H - H // 6 - H // 8, W - W // 9 - W // 7, 4), dtype=np.uint8)
        else:
            c = 270
            for ys in (slice(0, c), slice(H - c, H)):
                for xs in (slice(0, c), slice(W - c, W)):
                    out[i, ys, xs] = rng.integers(0, 256, (c, c, 4), dtype=np.uint8)
    return Bitmap.from_numpy(out.reshape(n, H * stride), W, H, stride, "cuda:0", alpha_meaningful=False)


def device_ms(b, iters):
    rects = torch.empty((b.n, 4), dtype=torch.int32, device="cuda:0")
    detect_content_into(b, 80, rects)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        detect_content_into(b, 80, rects)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, rects.cpu().tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    for kind, n in (("border", a.batch), ("corners", 1)):
        b = frames(kind, n)
        ms, rects = device_ms(b, a.iters)
        codes_bytes = 5.0 * W * H * n
        print(json.dumps({"case": kind, "frames": n, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 4),
                          "codes_pass_bytes": int(codes_bytes), "fraction_of_8TBps_if_all_codes": round(codes_bytes / (ms * 1e-3) / HBM, 4),
                          "rect0": rects[0]}), flush=True)
    b = frames("border", 1, seed=3)
    rects = torch.empty((1, 4), dtype=torch.int32, device="cuda:0")
    lat = []
    for i in range(a.iters + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        detect_content_into(b, 80, rects)
        rects.cpu()
        if i >= 3:
            lat.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"case": "single", "frames": 1, "latency_ms_median": round(float(np.median(lat)), 4),
                      "latency_ms_min": round(float(np.min(lat)), 4)}), flush=True)


if __name__ == "__main__":
    main()
