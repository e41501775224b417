#!/usr/bin/env python3
"""The device palette coder on a batch in HBM: n BGRA frames -> n palette PNG files (tools/bench_png_quantize.py [n] [w h]
[opaque|alpha] [--once]).  Prints one JSON line: ms per batch by hipEvents after warm-up, the files' sizes beside the device
`libpng` files of the same frames and that coder's time, the palette sizes and errors, and Pillow's quantize(MEDIANCUT) +
save of the same frames on one host thread as the outside yardstick.  --once: a single batch and no comparison, for a
kernel trace of its own (the time per stage is the trace's: histogram, palette, remap, the four deflate kernels, finish)."""
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imageflow_amd.codecs import libpng_encoder as PNG
from imageflow_amd.codecs import pngquant as Q
from imageflow_amd.graphics.bitmaps import Bitmap
from tools.bench_png_encode import photo_frames


def timed(run, budget_ms=3000.0):
    """Median, min and max ms per batch over up to five groups; the group size follows the first batch's time."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); run(); e1.record()
    torch.cuda.synchronize()
    first = e0.elapsed_time(e1)
    reps = int(max(1, min(10, budget_ms / 5 / max(first, 1e-3))))
    for _ in range(min(5, reps)):                                    # warm-up: clocks ramp over the first batches
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps)
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "batches_per_group": reps}


def main():
    args = [v for v in sys.argv[1:] if not v.startswith("--")]
    once = "--once" in sys.argv
    nums = [int(v) for v in args if v.isdigit()]
    n = nums[0] if nums else 32
    w, h = (nums[1], nums[2]) if len(nums) >= 3 else (800, 450)
    alpha = "alpha" in args
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    bm = Bitmap(photo_frames(n, w, h, stride, dev, alpha), w, h, stride, alpha_meaningful=alpha)
    stage = Q.PngQuantStage(w, h, n, dev)
    out = stage.quantize_device(bm, taps=True)
    torch.cuda.synchronize()
    res = {"frames": n, "w": w, "h": h, "alpha": alpha, "device": torch.cuda.get_device_name(0)}
    if once:
        print(json.dumps(res))
        return
    assert int(out["status"].abs().sum()) == 0
    res["quantize"] = timed(lambda: stage.quantize_device(bm))
    ln = out["lengths"].cpu().numpy()
    pal = out["palettes"].cpu().numpy()
    res["palette_png_bytes"] = int(ln.sum())
    res["palette_entries"] = [int(pal[i, 1024:].view(np.uint32)[0]) for i in range(n)][:8]
    res["mse_before_dithering"] = [round(float(v), 8) for v in out["mse"].cpu().numpy()[:8]]
    ct = PNG.PNG_RGBA if alpha else PNG.PNG_RGB
    plain = PNG.PngEncodeStage(w, h, ct, n, dev)
    pitch = (plain.max_file_bytes + 15) // 16 * 16
    files = torch.empty((n, pitch), dtype=torch.uint8, device=dev)
    lengths = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    res["libpng"] = timed(lambda: plain.encode_device(bm, 6, pitch, files, lengths, status))
    res["libpng_png_bytes"] = int(lengths.cpu().numpy().sum())
    res["palette_over_libpng_bytes"] = round(res["palette_png_bytes"] / res["libpng_png_bytes"], 4)
    # the outside yardstick: Pillow on one host thread, the first frames only when the batch is large
    from PIL import Image
    host = bm.data.view(n, h, stride)[:, :, :4 * w].reshape(n, h, w, 4).cpu().numpy()
    k = min(n, 4)
    t0 = time.perf_counter()
    size = 0
    for i in range(k):
        rgba = np.ascontiguousarray(host[i][..., [2, 1, 0, 3]])
        im = Image.fromarray(rgba, "RGBA") if alpha else Image.fromarray(np.ascontiguousarray(rgba[..., :3]))
        q = im.quantize(256, method=Image.Quantize.FASTOCTREE if alpha else Image.Quantize.MEDIANCUT)   # (Pillow's median cut takes no alpha)
        b = io.BytesIO()
        q.save(b, "PNG")
        size += len(b.getvalue())
    res["pillow_one_thread_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / k, 2)
    res["pillow_bytes_per_frame"] = size // k
    res["device_ms_per_frame"] = round(res["quantize"]["ms_median"] / n, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
