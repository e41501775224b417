#!/usr/bin/env python3
"""The device GIF decoder on batches of files (tools/bench_gif_decode.py [--case NAME] [--reps N]).  Cases: 1, 8 and 32
photo-like 800x450 files (the test frames quantised to 256 colours with dithering, written by Pillow), one flat 800x450 file
and one 3840x2160 file.  Per case one JSON line: the whole call (host container walk, upload, the five launches, wait) for the
batch; the stages by difference (the development switch gif_decode_stop_after ends the call behind the scan, or behind
lengths + place + resolve); and two yardsticks measured in the same run: one host core's Pillow on the same files, and this
project's own PNG reader (one wave per file) on palette PNG files of the same frames.

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

# n, w, h, flat, reps, time limit s
CASES = {"800x450x1": (1, 800, 450, False, 5, 200), "800x450x8": (8, 800, 450, False, 5, 200), "800x450x32": (32, 800, 450, False, 3, 300),
         "flat_800x450x1": (1, 800, 450, True, 5, 200), "2160p_x1": (1, 3840, 2160, False, 3, 400)}


def run_case(name, reps=None):
    import numpy as np
    import torch
    from PIL import Image
    from imageflow_amd import _native
    from imageflow_amd.codecs import gif_decoder as D
    from imageflow_amd.codecs import libpng_decoder as P
    from imageflow_amd.graphics.bitmaps import Bitmap
    from bench_png_encode import photo_frames
    n, w, h, flat, default_reps, _ = CASES[name]
    reps = reps or default_reps
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    src = photo_frames(n, w, h, stride, dev, False).view(n, h, stride)[:, :, :4 * w].cpu().numpy().reshape(n, h, w, 4)
    gifs, pngs, want = [], [], []
    for i in range(n):
        rgb = np.ascontiguousarray(src[i][..., [2, 1, 0]])
        if flat:
            rgb[:] = (40, 90, 200)
        pal = Image.fromarray(rgb, "RGB").quantize(256, dither=Image.Dither.FLOYDSTEINBERG)
        for fmt, out in (("GIF", gifs), ("PNG", pngs)):
            buf = io.BytesIO()
            pal.save(buf, fmt)
            out.append(buf.getvalue())
        rgba = np.asarray(pal.convert("RGBA"))
        want.append(np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]).reshape(h, 4 * w))
    want = np.stack(want)
    res = {"case": name, "files": n, "w": w, "h": h, "reps": reps, "device": torch.cuda.get_device_name(0), "gif_bytes": sum(map(len, gifs)), "png_bytes": sum(map(len, pngs))}
    frames = [Bitmap(torch.zeros((1, h * stride), dtype=torch.uint8, device=dev), w, h, stride, True) for _ in range(n)]

    def timed(call, stop=None):
        _native.debug_set("gif_decode_stop_after", stop)
        call()                                                   # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        _native.debug_set("gif_decode_stop_after", None)
        print(f"  {name} {call.__name__} stop_after={stop}: {np.median(ts):.3f} ms", file=sys.stderr, flush=True)
        return float(np.median(ts))

    def gif_batch():
        D.decode_gif_batch(gifs, None, dev, frames=frames)

    def png_batch():
        P.decode_png_batch(pngs, dev)
    whole = timed(gif_batch)
    _, st = D.decode_gif_batch(gifs, None, dev, frames=frames)
    assert not any(st), st
    got = torch.stack([f.data.view(h, stride)[:, :4 * w] for f in frames]).cpu().numpy()
    assert np.array_equal(got, want), "decoded frames differ from Pillow's"
    t_scan, t_resolve = timed(gif_batch, "scan"), timed(gif_batch, "resolve")
    png = timed(png_batch)
    ts = []
    for _ in range(max(3, reps)):
        t0 = time.perf_counter()
        for f in gifs:
            im = Image.open(io.BytesIO(f))
            im.load()
        ts.append((time.perf_counter() - t0) * 1e3)
    host = float(np.median(ts))
    res.update(batch_ms=round(whole, 3), scan_with_host_part_ms=round(t_scan, 3), lengths_place_resolve_ms=round(t_resolve - t_scan, 3), compose_ms=round(whole - t_resolve, 3),
               host_pillow_one_core_ms=round(host, 3), batch_over_host=round(whole / host, 2), own_png_reader_ms=round(png, 3), batch_over_png_reader=round(whole / png, 2),
               MPps=round(n * w * h / 1e6 / (whole * 1e-3), 2))
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
