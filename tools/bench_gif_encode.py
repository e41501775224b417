#!/usr/bin/env python3
"""The device GIF coder on a batch in HBM: n BGRA frames -> n GIF files (tools/bench_gif_encode.py [n] [w h] [opaque|alpha]
[--once] [--stages] [--all]).  Prints one JSON line per shape: ms per batch by hipEvents after warm-up, the files' sizes
beside Pillow's GIF files of the same palettes and indices, Pillow's save(.., "GIF") of those indexed frames on one host
thread as the outside yardstick, and this project's `pngquant` preset coder on the same frames.  --all: the three shapes of
DESIGN section 6 (1 and 32 frames of 800 x 450, one 3840 x 2160).  --stages: the shape again in a child process under
rocprofv3's kernel trace, and the median time of every kernel of the batch (histogram levels, palette, remap, lzw, scan,
gather, finish).  --once: a single batch and nothing else, what the trace runs."""
import csv
import glob
import io
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1, 800, 450), (32, 800, 450), (1, 3840, 2160)]


def stages(n, w, h, alpha):
    """median microseconds per kernel of one batch, from a kernel trace of a child process that runs the shape with --once"""
    with tempfile.TemporaryDirectory(prefix="bench_gif_encode_") as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), str(n), str(w), str(h),
               "alpha" if alpha else "opaque", "--once"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    per = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("ifhip::", "").replace("void ", "")
        if name.startswith(("pngq_histogram", "pngq_palette", "gif_")):
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    out = {}
    for name, v in per.items():
        k = 6 if name.startswith("pngq_histogram") else 1              # launches per batch
        batches = len(v) // k
        sums = [sum(v[i * k:(i + 1) * k]) for i in range(batches)]
        out[name] = {"us_median": round(float(np.median(sums[1:] or sums)), 1), "launches_per_batch": k}
    return out


def one_shape(n, w, h, alpha, once, with_stages):
    import torch
    from imageflow_amd.codecs import gif_encoder as GIF
    from imageflow_amd.codecs import pngquant as Q
    from imageflow_amd.graphics.bitmaps import Bitmap
    from tools.bench_png_encode import photo_frames
    from tools.bench_png_quantize import timed
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    bm = Bitmap(photo_frames(n, w, h, stride, dev, alpha), w, h, stride, alpha_meaningful=alpha)
    stage = GIF.GifEncodeStage(w, h, n, dev)
    res = {"frames": n, "w": w, "h": h, "alpha": alpha, "device": torch.cuda.get_device_name(0)}
    if once:
        for _ in range(4):
            stage.encode_device(bm)
        torch.cuda.synchronize()
        return res
    files, lengths, status, palettes, indices = stage.encode_device(bm, taps=True)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    res["gif"] = timed(lambda: stage.encode_device(bm))
    res["device_ms_per_frame"] = round(res["gif"]["ms_median"] / n, 3)
    ln = lengths.cpu().numpy()
    res["gif_bytes_per_frame"] = int(ln.sum()) // n
    pal, idx = palettes.cpu().numpy(), indices.cpu().numpy()
    res["palette_entries"] = [int(pal[i, 1024:].view(np.uint32)[0]) for i in range(n)][:4]
    # the outside yardstick: Pillow's writer on one host thread, on the indexed frames the device chose
    from PIL import Image
    k = min(n, 4)
    t, size = 0.0, 0
    for i in range(k):
        im = Image.fromarray(idx[i], "P")
        im.putpalette(pal[i, :1024].reshape(256, 4)[:, :3].tobytes())
        b = io.BytesIO()
        t0 = time.perf_counter()
        im.save(b, "GIF")
        t += time.perf_counter() - t0
        size += b.tell()
    res["pillow_one_thread_ms_per_frame"] = round(t * 1e3 / k, 2)
    res["pillow_bytes_per_frame"] = size // k
    res["gif_over_pillow_bytes"] = round(res["gif_bytes_per_frame"] / res["pillow_bytes_per_frame"], 4)
    try:                                                             # this project's pngquant preset coder on the same frames
        qs = Q.PngQuantStage(w, h, n, dev)
        qs.quantize_device(bm)
        torch.cuda.synchronize()
        res["pngquant"] = timed(lambda: qs.quantize_device(bm))
    except Exception as e:                                           # (a geometry that coder refuses)
        res["pngquant"] = str(e)[:80]
    if with_stages:
        del stage
        res["stages_us"] = stages(n, w, h, alpha)
    return res


def main():
    args = [v for v in sys.argv[1:] if not v.startswith("--")]
    nums = [int(v) for v in args if v.isdigit()]
    shapes = SHAPES if "--all" in sys.argv else [(nums[0] if nums else 32,) + ((nums[1], nums[2]) if len(nums) >= 3 else (800, 450))]
    for n, w, h in shapes:
        print(json.dumps(one_shape(n, w, h, "alpha" in args, "--once" in sys.argv, "--stages" in sys.argv)), flush=True)


if __name__ == "__main__":
    main()
