#!/usr/bin/env python3
"""The device lossy WebP coder on batches of frames (tools/bench_webp_lossy_encode.py [--case NAME] [--reps N] [--quality Q] [--intra4]).
--intra4: stages with IFHIP_VP8_ENC_INTRA4, whose code kernel also tries the sixteen 4x4 luma modes of every macroblock.
Cases: one and 32 frames of 800x450 and one of 3840x2160, each with and without alpha.  Per case one JSON line, device time by
events around the call after a warm-up (the frames are in HBM already and the files stay there): the whole call, and the
kernels by difference -- the development switch vp8_encode_stop_after ends the call behind a launch: convert, the inner
lossless coder of the alpha planes, the macroblock wavefront, counts + probabilities, the bool-coded streams, the layout.  The
yardstick is ONE host core's libwebp through Pillow at method=4 on the same frames in the same run; its file sizes and PSNR
stand beside this coder's (decoded by Pillow).

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

# frames, w, h, alpha, reps, time limit s
CASES = {"800x450x1": (1, 800, 450, False, 5, 200), "800x450x32": (32, 800, 450, False, 5, 300), "800x450_rgba_x1": (1, 800, 450, True, 5, 200),
         "800x450_rgba_x32": (32, 800, 450, True, 3, 300), "2160p_x1": (1, 3840, 2160, False, 3, 400), "2160p_rgba_x1": (1, 3840, 2160, True, 3, 400)}
STOPS = ("convert", "alpha", "code", "decide", "streams")


def photo(w, h, seed, alpha):
    """BGRA, photo-like: smooth waves, a few edges, a little noise"""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [128 + 90 * np.sin(x / (37.0 + 9 * k) + k + seed) * np.cos(y / (41.0 - 6 * k)) + 25 * ((x // 64 + y // 48) % 2) + rng.normal(0, 4, (h, w)) for k in range(3)]
    planes.append(255 - 60 * (1 + np.sin(x / 90.0 + y / 70.0)) if alpha else 255 + 0 * x)
    return np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)


def psnr(a, b):
    import numpy as np
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(10.0 * np.log10(255.0 ** 2 / max(float(np.mean(d * d)), 1e-12)))


def run_case(name, reps=None, quality=75.0, intra4=False):
    import numpy as np
    import torch
    from PIL import Image
    from imageflow_amd import _native
    from imageflow_amd.codecs import webp_lossy_encoder as ENC
    from imageflow_amd.graphics.bitmaps import Bitmap
    n, w, h, alpha, default_reps, _ = CASES[name]
    reps = reps or default_reps
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    frames = [photo(w, h, i, alpha) for i in range(n)]
    rows = np.zeros((n, h, stride), np.uint8)
    for i, f in enumerate(frames):
        rows[i, :, :4 * w] = f.reshape(h, 4 * w)
    bitmap = Bitmap.from_numpy(rows, w, h, stride, dev, alpha_meaningful=alpha)
    stage = ENC.WebpLossyEncodeStage(w, h, alpha, n, dev, intra4=intra4)
    pitch = (stage.max_file_bytes + 15) // 16 * 16
    files = torch.empty((n, pitch), dtype=torch.uint8, device=dev)
    lengths, status = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)

    def timed(stop=None):
        _native.debug_set("vp8_encode_stop_after", stop)
        stage.encode_device(bitmap, quality, pitch, files, lengths, status)   # warm-up (the first one allocates the stage's scratch)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            stage.encode_device(bitmap, quality, pitch, files, lengths, status)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        _native.debug_set("vp8_encode_stop_after", None)
        print(f"  {name} stop_after={stop}: {np.median(ts):.3f} ms", file=sys.stderr, flush=True)
        return float(np.median(ts))

    at = {s: timed(s) for s in STOPS}
    whole = timed()
    assert not status.cpu().numpy().any(), status
    sizes = lengths.cpu().numpy()
    mine = files[0, :int(sizes[0])].cpu().numpy().tobytes()
    im = Image.open(io.BytesIO(mine))
    assert im.mode == ("RGBA" if alpha else "RGB") and im.size == (w, h)
    decoded = np.asarray(im.convert("RGBA"))[..., [2, 1, 0, 3]]
    if alpha:
        assert np.array_equal(decoded[..., 3], frames[0][..., 3])
    host_ts, host_sizes, host_psnr = [], [], 0.0
    for _ in range(max(3, reps)):
        t0 = time.perf_counter()
        host_sizes = []
        for f in frames:
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(f[..., [2, 1, 0, 3]] if alpha else f[..., [2, 1, 0]]), "RGBA" if alpha else "RGB").save(buf, "WEBP", quality=quality, method=4)
            host_sizes.append(len(buf.getvalue()))
        host_ts.append((time.perf_counter() - t0) * 1e3)
        host_psnr = psnr(np.asarray(Image.open(buf).convert("RGBA"))[..., [2, 1, 0, 3]], frames[-1])
    host = float(np.median(host_ts))
    res = {"case": name, "frames": n, "w": w, "h": h, "alpha": alpha, "quality": quality, "intra4": intra4, "reps": reps, "device": torch.cuda.get_device_name(0),
           "whole_call_ms": round(whole, 3), "convert_ms": round(at["convert"], 3), "inner_lossless_alpha_ms": round(at["alpha"] - at["convert"], 3),
           "code_wavefront_ms": round(at["code"] - at["alpha"], 3), "count_and_decide_ms": round(at["decide"] - at["code"], 3),
           "bool_streams_ms": round(at["streams"] - at["decide"], 3), "layout_ms": round(whole - at["streams"], 3),
           "file_bytes": int(sizes.sum()), "psnr_first_frame_db": round(psnr(decoded, frames[0]), 2),
           "host_libwebp_method4_one_core_ms": round(host, 3), "host_file_bytes": int(sum(host_sizes)), "host_psnr_last_frame_db": round(host_psnr, 2),
           "call_over_host": round(whole / host, 2), "MPps": round(n * w * h / 1e6 / (whole * 1e-3), 2)}
    print(json.dumps(res), flush=True)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else None
    quality = float(sys.argv[sys.argv.index("--quality") + 1]) if "--quality" in sys.argv else 75.0
    intra4 = "--intra4" in sys.argv
    if "--case" in sys.argv:
        run_case(sys.argv[sys.argv.index("--case") + 1], reps, quality, intra4)
        return 0
    for name, case in CASES.items():
        cmd = ["timeout", "-k", "10", str(case[-1]), sys.executable, os.path.abspath(__file__), "--case", name, "--quality", str(quality)] + (["--reps", str(reps)] if reps else []) + (["--intra4"] if intra4 else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:                                                   # a fault, an abort or the time limit: nothing more runs on this device
            print(json.dumps({"case": name, "exit_status": rc, "stopped": True}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
