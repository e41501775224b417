#!/usr/bin/env python3
"""Times the finishing nodes on the device (csrc/white_balance.hip, csrc/round_corners.hip), one JSON line per case:

  white balance   1 and 64 frames of 3840x2160, random content and one constant colour: ms per call (memset + histogram
                  + apply), and the fraction of 8 TB/s with the traffic counted as 3 x frame bytes (read, read, write).
                  A constant frame far slower than a random one would mean the LDS histogram serialises.
  round corners   one 3840x2160 frame at 10 % and in circle mode: ms per call.

    python tools/bench_finishing.py [--iters K] [--out profiles/finishing_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from imageflow_amd.graphics.bitmaps import Bitmap, get_stride  # noqa: E402
from imageflow_amd.graphics.rounded_corners import clear_around_rounded_corners  # noqa: E402
from imageflow_amd.graphics.white_balance import white_balance_srgb  # noqa: E402

W, H = 3840, 2160
PEAK = 8e12


def frames(n, kind, dev):
    stride = get_stride(W)
    g = torch.Generator(device=dev).manual_seed(n)
    if kind == "constant":
        data = torch.tensor([40, 120, 200, 255], dtype=torch.uint8, device=dev).repeat(n, H * stride // 4)
    else:
        data = torch.randint(0, 256, (n, H * stride), dtype=torch.uint8, device=dev, generator=g)
    return Bitmap(data, W, H, stride)


def time_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = []
    for n in (1, 64):
        for kind in ("random", "constant"):
            b = frames(n, kind, dev)
            ms = time_ms(lambda: white_balance_srgb(b), a.iters)     # (frames keep changing: the maps are re-derived each call)
            traffic = 3.0 * n * W * H * 4
            lines.append({"op": "white_balance", "frames": n, "w": W, "h": H, "content": kind, "ms_per_call": round(ms, 4),
                          "traffic_bytes": traffic, "frac_of_8TBs": round(traffic / (ms * 1e-3) / PEAK, 3)})
            del b
            torch.cuda.empty_cache()
    b = frames(1, "random", dev)
    for mode, radii in (("percentage", [10.0]), ("circle", [0.0])):
        ms = time_ms(lambda: clear_around_rounded_corners(b, mode, radii, 0x80FFFFFF), a.iters)
        lines.append({"op": "round_corners", "frames": 1, "w": W, "h": H, "mode": mode, "radii": radii, "ms_per_call": round(ms, 4)})
    out = open(a.out, "w") if a.out else None
    for ln in lines:
        s = json.dumps(ln)
        print(s)
        if out:
            out.write(s + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
