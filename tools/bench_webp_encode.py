#!/usr/bin/env python3
"""Sizes and times of the device lossless-WebP coder, on one GPU:

    python tools/bench_webp_encode.py [--out FILE.json] [--only-indexing] [--skip-indexing]

Sizes: the photo-like and flat test frames at 800x450 as this coder writes them, as libwebp writes them through Pillow
(lossless=True, quality=70, method=4: the simple API's defaults) and as this project's `libpng` coder writes them (RGBA,
and RGB for the opaque frames).  The frames are tests/webp_frames.py photo(800, 450, seed=61), photo(..., alpha=True,
seed=62) and flat(800, 450).
Times: 32 frames of 800x450 and 8 frames of 3840x2160, hipEvents around one batch call after warm-up (median, minimum and
maximum of the repetitions), beside ONE host core's libwebp on the same frames.  Every device file is decoded through
Pillow and compared with its source before its size counts.
Colour indexing (the stage flag IFHIP_WEBP_ENC_COLOR_INDEXING): few_colours(800, 450), few_colours(800, 450, n=200) and
flat(800, 450) with the flag off and on -- sizes beside libwebp's, and the times of a lone frame and of 32 -- and the
photographs again with the flag on, where the coder counts colours, gives up and writes the plain file.  --skip-indexing
leaves these rows out (the tool then runs on a library without the flag as well), --only-indexing everything else."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imageflow_amd.codecs import libpng_encoder as PNG  # noqa: E402
from imageflow_amd.codecs import webp_encoder as WEBP  # noqa: E402
from imageflow_amd.graphics.bitmaps import Bitmap  # noqa: E402
from tests import util as U  # noqa: E402
from tests import webp_frames as F  # noqa: E402

DEV = "cuda:0"


def bitmap(frames, alpha=True):
    n, h, w, _ = frames.shape
    rows = np.zeros((n, h, U.stride_for(w)), np.uint8)
    rows[:, :, :4 * w] = frames.reshape(n, h, 4 * w)
    return Bitmap.from_numpy(rows, w, h, rows.shape[-1], DEV, alpha_meaningful=alpha)


def libwebp(bgra):
    """(bytes, seconds) of libwebp's file; only the save is timed, not the channel swap or Pillow's wrapping of the array"""
    im, b = Image.fromarray(F.rgba_of(bgra), "RGBA"), io.BytesIO()
    t0 = time.perf_counter()
    im.save(b, "WEBP", lossless=True, quality=70, method=4)
    return len(b.getvalue()), time.perf_counter() - t0


def sizes():
    out = {}
    for name, frame in (("photo", F.photo(800, 450, seed=61)), ("photo_alpha", F.photo(800, 450, alpha=True, seed=62)), ("flat", F.flat(800, 450))):
        h, w = frame.shape[:2]
        bm = bitmap(frame[None])
        webp = WEBP.WebpEncodeStage(w, h, True, 1, DEV).encode(bm)[0][0]
        png = PNG.PngEncodeStage(w, h, PNG.PNG_RGBA, 1, DEV).encode(bm)[0][0]
        png_rgb = PNG.PngEncodeStage(w, h, PNG.PNG_RGB, 1, DEV).encode(bm)[0][0] if name != "photo_alpha" else None   # what the preset writes for an opaque frame
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(webp)).convert("RGBA")), F.rgba_of(frame))
        out[name] = {"device_webp": len(webp), "libwebp_q70_m4": libwebp(frame)[0], "device_libpng_rgba": len(png),
                     "device_libpng_rgb": len(png_rgb) if png_rgb else None, "raw": w * h * 4}
        print(name, out[name], flush=True)
    return out


def timed(frames, reps, host=True, **flags):
    n, h, w, _ = frames.shape
    bm = bitmap(frames)
    stage = WEBP.WebpEncodeStage(w, h, True, n, DEV, **flags)
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    files = torch.empty((n, pitch), dtype=torch.uint8, device=DEV)
    ln, st = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    for _ in range(3):
        stage.encode_device(bm, pitch, files, ln, st)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        stage.encode_device(bm, pitch, files, ln, st)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    assert st.cpu().tolist() == [0] * n
    res = {"frames": n, "device_ms_median": float(np.median(ms)), "device_ms_min": float(min(ms)), "device_ms_max": float(max(ms)), "reps": reps,
           "file_bytes_mean": float(ln.float().mean())}
    if host:
        host = [libwebp(f)[1] for f in frames[:min(n, 4)]]
        res.update({"libwebp_one_core_ms_per_frame": 1000 * float(np.mean(host)), "libwebp_one_core_ms_batch": 1000 * float(np.mean(host)) * n})
    print(f"{n} x {w}x{h}", flags, res, flush=True)
    return res


def indexing():
    """the frames of few colours, flag off and on: sizes against libwebp, times of a lone frame and of 32 (the same frame rolled)"""
    out = {}
    kinds = (("few_colours", F.few_colours(800, 450)), ("few_colours_200", F.few_colours(800, 450, n=200)), ("flat", F.flat(800, 450)),
             ("photo", F.photo(800, 450, seed=61)))
    for name, frame in kinds:
        h, w = frame.shape[:2]
        row = {"libwebp_q70_m4": libwebp(frame)[0]}
        for key, on in (("flag_off", False), ("flag_on", True)):
            data = WEBP.WebpEncodeStage(w, h, True, 1, DEV, color_indexing=on).encode(bitmap(frame[None]))[0][0]
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGBA")), F.rgba_of(frame))
            batch = np.stack([np.roll(frame, 13 * i, 1) for i in range(32)]) if name != "photo" else np.stack([F.photo(800, 450, seed=70 + i) for i in range(32)])
            row[key] = {"bytes": len(data), "ratio_to_libwebp": len(data) / row["libwebp_q70_m4"],
                        "lone": timed(frame[None], 30, host=False, color_indexing=on), "batch_32": timed(batch, 30, host=False, color_indexing=on)}
        out[name] = row
        print(name, {k: (v if k == "libwebp_q70_m4" else (v["bytes"], round(v["ratio_to_libwebp"], 3))) for k, v in row.items()}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-indexing", action="store_true")
    ap.add_argument("--skip-indexing", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures on the device and has no fall-back")
    out = {}
    if not args.only_indexing:
        out = {"sizes": sizes(), "times": {}}
        out["times"]["32x800x450"] = timed(np.stack([F.photo(800, 450, seed=70 + i) for i in range(32)]), 30)
        out["times"]["1x800x450"] = timed(F.photo(800, 450, seed=61)[None], 30)
        big = F.photo(3840, 2160, seed=80)
        out["times"]["8x3840x2160"] = timed(np.stack([np.roll(big, 97 * i, 1) for i in range(8)]), 10)
    if not args.skip_indexing:
        out["color_indexing"] = indexing()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
