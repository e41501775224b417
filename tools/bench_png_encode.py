#!/usr/bin/env python3
"""The device PNG coder on a batch in HBM: n BGRA frames -> n PNG files (tools/bench_png_encode.py [n] [w h] [rgb|rgba]
[--once]).  Prints one JSON line: ms per batch by hipEvents after warm-up, the files' sizes against zlib level 6 with
Z_FILTERED on the same filtered streams (one host thread, timed for scale), and whether every file inflates to a
stream of the full length.  --once: a single batch and no host comparison, for a kernel trace of its own."""
import json
import os
import struct
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imageflow_amd.codecs import libpng_encoder as PNG
from imageflow_amd.graphics.bitmaps import Bitmap


def photo_frames(n, w, h, stride, dev, alpha):
    """photo-like content: low-frequency sinusoids + Gaussian noise sigma 2.5 + flat rectangles (the size conditions' frame)"""
    g = torch.Generator(device=dev).manual_seed(7)
    y = torch.arange(h, device=dev).view(1, h, 1).float()
    x = torch.arange(w, device=dev).view(1, 1, w).float()
    k = torch.arange(n, device=dev).view(n, 1, 1).float()
    frames = torch.zeros((n, h, stride), dtype=torch.uint8, device=dev)
    px = frames[:, :, :4 * w].view(n, h, w, 4)
    noise = lambda: torch.randn((n, h, w), device=dev, generator=g) * 2.5
    px[..., 0] = (128 + 60 * torch.sin((x + 13 * k) / 97) + 30 * torch.cos(y / 45) + noise()).round().clamp(0, 255).to(torch.uint8)
    px[..., 1] = (128 + 60 * torch.cos((y + 7 * k) / 61) + 25 * torch.sin(x / 150) + noise()).round().clamp(0, 255).to(torch.uint8)
    px[..., 2] = (128 + 50 * torch.sin((x + y + 31 * k) / 120) + noise()).round().clamp(0, 255).to(torch.uint8)
    px[..., 3] = 255
    px[:, h // 8:h // 3, w // 10:w // 2, :3] = 255                    # a flat area, transparent when alpha is coded
    if alpha:
        px[:, h // 8:h // 3, w // 10:w // 2, 3] = 0
    return frames.view(n, -1)


def idat(data):
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        if data[at + 4:at + 8] == b"IDAT":
            out.append(data[at + 8:at + 8 + n])
        at += 12 + n
    return b"".join(out)


def main():
    args = [v for v in sys.argv[1:] if not v.startswith("--")]
    once = "--once" in sys.argv
    nums = [int(v) for v in args if v.isdigit()]
    n = nums[0] if nums else 32
    w, h = (nums[1], nums[2]) if len(nums) >= 3 else (800, 450)
    ct = PNG.PNG_RGBA if "rgba" in args else PNG.PNG_RGB
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    bm = Bitmap(photo_frames(n, w, h, stride, dev, ct == PNG.PNG_RGBA), w, h, stride, alpha_meaningful=ct == PNG.PNG_RGBA)
    stage = PNG.PngEncodeStage(w, h, ct, n, dev)
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    files = torch.empty((n, pitch), dtype=torch.uint8, device=dev)
    lengths = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    run = lambda: stage.encode_device(bm, 6, pitch, files, lengths, status)
    run()
    torch.cuda.synchronize()
    res = {"frames": n, "w": w, "h": h, "color_type": "rgba" if ct == PNG.PNG_RGBA else "rgb", "device": torch.cuda.get_device_name(0)}
    if once:
        print(json.dumps(res))
        return
    for _ in range(5):                                               # warm-up: clocks ramp over the first batches
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):                                               # five groups of ten batches: median and spread
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 10)
    assert int(status.abs().sum()) == 0
    ln = lengths.cpu().numpy()
    host = files.cpu().numpy()
    bpp = 3 if ct == PNG.PNG_RGB else 4
    filtered = n * h * (1 + w * bpp)
    streams = [zlib.decompress(idat(host[i, :int(ln[i])].tobytes())) for i in range(n)]
    t0 = time.perf_counter()
    ref = 0
    for s in streams:
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FILTERED)
        ref += len(co.compress(s) + co.flush())
    t1 = time.perf_counter()
    s_dev = sum(len(idat(host[i, :int(ln[i])].tobytes())) for i in range(n))
    res.update({
        "batch_ms_median": round(float(np.median(times)), 4), "batch_ms_min": round(min(times), 4), "batch_ms_max": round(max(times), 4),
        "MPps": round(n * w * h / 1e6 / (float(np.median(times)) * 1e-3), 1),
        "filtered_GBps": round(filtered / (float(np.median(times)) * 1e-3) / 1e9, 2),
        "idat_bytes": s_dev, "zlib6_filtered_bytes": ref, "S_over_R6": round(s_dev / ref, 4),
        "streams_inflate_to_full_length": all(len(s) == h * (1 + w * bpp) for s in streams),
        "host_zlib6_one_thread_ms": round((t1 - t0) * 1e3, 1),
    })
    print(json.dumps(res))


if __name__ == "__main__":
    main()
