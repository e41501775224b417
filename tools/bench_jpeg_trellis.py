#!/usr/bin/env python3
"""Times and sizes of the mozjpeg preset's device chain, on one GPU:

    python tools/bench_jpeg_trellis.py [--out FILE.json] [--quality Q]

Trellis chain: raw forward stage + trellis stage + the flagged device entropy coder (optimised tables, progressive).
Plain chain: the quantising forward stage + the same flagged coder -- what the libjpeg_turbo preset already does -- on the
same frames: 32 frames of 800x450 and 8 frames of 3840x2160 (tests/webp_frames.py photo).  hipEvents around one batch call
of each chain after warm-up (median, minimum and maximum of the repetitions); the trellis stage alone is timed too.  Reports
both times, their ratio and the mean file sizes.  No time is fixed in advance."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imageflow_amd.codecs import mozjpeg as M  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import util as U  # noqa: E402
from tests import webp_frames as F  # noqa: E402

DEV = "cuda:0"
HS, VS = [2, 1, 1], [2, 1, 1]


def bitmap(frames):
    n, h, w, _ = frames.shape
    rows = np.zeros((n, h, U.stride_for(w)), np.uint8)
    rows[:, :, :4 * w] = frames.reshape(n, h, 4 * w)
    return Bitmap.from_numpy(rows, w, h, rows.shape[-1], DEV, alpha_meaningful=False)


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def timed(frames, quality, reps):
    n, h, w, _ = frames.shape
    bm = bitmap(frames)
    fwd = M.JpegForwardStage(w, h, HS, VS, n, DEV)
    trellis = M.JpegTrellisStage(w, h, HS, VS, n, DEV)
    coder = M.JpegEntropyStage(w, h, HS, VS, fwd.blocks_w, fwd.blocks_h, n, DEV)
    qt = torch.from_numpy(np.stack([M.quant_tables_for_quality(quality)] * n).view(np.int16)).to(DEV)
    shapes = [(n, fwd.blocks_h[c], fwd.blocks_w[c], 64) for c in range(3)]
    raw = [torch.empty(s, dtype=torch.int16, device=DEV) for s in shapes]
    coef = [torch.empty(s, dtype=torch.int16, device=DEV) for s in shapes]
    pitch = (coder.max_file_bytes_for(True, True) + 15) // 16 * 16
    files = torch.empty((n, pitch), dtype=torch.uint8, device=DEV)
    out = {}

    def plain_chain():
        fwd.write_frames(bm, qt, coef=coef)
        out["plain"] = coder.encode_device(coef, quality, pitch, files, progressive=True, optimize_coding=True)

    def trellis_chain():
        fwd.write_frames(bm, None, coef=raw, raw=True)
        trellis.quantize(raw, qt, coef=coef)
        out["trellis"] = coder.encode_device(coef, quality, pitch, files, progressive=True, optimize_coding=True)

    res = {"frames": n, "quality": quality, "reps": reps}
    res["plain_ms"] = event_ms(plain_chain, reps)
    res["plain_file_bytes_mean"] = float(out["plain"][1].float().mean())
    assert out["plain"][2].cpu().tolist() == [0] * n
    res["trellis_ms"] = event_ms(trellis_chain, reps)
    res["trellis_file_bytes_mean"] = float(out["trellis"][1].float().mean())
    assert out["trellis"][2].cpu().tolist() == [0] * n
    res["trellis_stage_alone_ms"] = event_ms(lambda: trellis.quantize(raw, qt, coef=coef), reps)
    res["time_ratio"] = res["trellis_ms"]["median"] / res["plain_ms"]["median"]
    res["size_ratio"] = res["trellis_file_bytes_mean"] / res["plain_file_bytes_mean"]
    print(f"{n} x {w}x{h}", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quality", type=int, default=75)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures on the device and has no fall-back")
    out = {"times": {}}
    out["times"]["32x800x450"] = timed(np.stack([F.photo(800, 450, seed=70 + i) for i in range(32)]), args.quality, 30)
    big = F.photo(3840, 2160, seed=80)
    out["times"]["8x3840x2160"] = timed(np.stack([np.roll(big, 97 * i, 1) for i in range(8)]), args.quality, 10)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
