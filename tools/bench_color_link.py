#!/usr/bin/env python3
"""The colour link kernels on batches of frames, next to the matrix kernel on the same frames (tools/bench_color_link.py
[--case NAME] [--reps N]).  Cases: 1 and 8 frames of 3840x2160 and 32 frames of 800x450, on photo-like content (neighbouring
pixels fall into neighbouring cells of the link) and on random bytes (every pixel its own cell: the worst case for the node
loads).  Per case one JSON line; per content and kernel -- the RGB link of a lut16 profile, the grey table, the matrix kernel
with a Display P3 plan -- the launch's time between two device events on its stream (median over the repetitions; the frames
are restored from a pristine copy before each one, outside the events, because the conversion is in place) and the pixel bytes
it moves, every pixel read once and written once, per second.  The link's own node loads are not counted.

Before anything is timed the device's bytes are compared with the CPU emulation's on one frame of the case.  The tool reports;
it gates nothing.

Without --case every case runs as a child process of its own under `timeout -k 10`, one after the other, and the first that
fails ends the run: nothing more is started on a device that has just faulted or hung."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# n, w, h, reps, time limit s
CASES = {"2160p_x1": (1, 3840, 2160, 50, 200), "2160p_x8": (8, 3840, 2160, 20, 300), "800x450x32": (32, 800, 450, 50, 200)}


def run_case(name, reps=None):
    import numpy as np
    import torch
    from imageflow_amd.codecs import color_profile as CP
    from imageflow_amd.graphics.bitmaps import Bitmap
    from bench_png_encode import photo_frames
    from tests import color_link_emulation as LE
    from tests import color_link_profiles as W
    from tests import color_profile_emulation as E
    from tests.test_jpeg_headers import P3_XYZ, make_icc
    n, w, h, default_reps, _ = CASES[name]
    reps = reps or default_reps
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    lut_icc, gray_icc, p3_icc = W.mft_profile(5, grid=17).icc, W.gray_profile(W.GRAY_TRCS["dotgain"]), make_icc(xyz=P3_XYZ)
    rgb_link, gray_link, plan = CP.link_from_icc(lut_icc), CP.link_from_icc(gray_icc, True), CP.plan_from_icc(p3_icc)
    kernels = {
        "rgb_link": (lambda bm: CP.link_to_srgb(bm, rgb_link), lambda rows: LE.transform(rows, w, LE.link_from_icc(lut_icc)[1])),
        "gray_table": (lambda bm: CP.link_to_srgb(bm, gray_link), lambda rows: LE.transform(rows, w, LE.link_from_icc(gray_icc, True)[1])),
        "matrix": (lambda bm: CP.transform_to_srgb(bm, plan), lambda rows: E.transform(rows, w, E.plan_from_icc(p3_icc)[1])),
    }
    moved = 2 * n * h * w * 4
    res = {"case": name, "frames": n, "w": w, "h": h, "reps": reps, "bytes_moved": moved, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator(device=dev).manual_seed(11)
    contents = {"photo": photo_frames(n, w, h, stride, dev, True),
                "random": torch.randint(0, 256, (n, h * stride), dtype=torch.uint8, device=dev, generator=g)}
    for label, pristine in contents.items():
        res[label] = {}
        for kernel, (launch, emulate) in kernels.items():
            bm = Bitmap(pristine.clone(), w, h, stride, alpha_meaningful=True)
            launch(bm)                                                    # warm-up (the link's upload), and the check
            torch.cuda.synchronize()
            last = n - 1
            want = emulate(pristine[last].view(h, stride).cpu().numpy())
            got = bm.data[last].view(h, stride).cpu().numpy()
            assert np.array_equal(got[:, :4 * w], want[:, :4 * w]), "the device's bytes differ from the emulation's"
            ms = []
            for _ in range(reps):
                bm.data.copy_(pristine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(bm)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            res[label][kernel] = {"launch_ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4), "p90_ms": round(float(np.percentile(ms, 90)), 4),
                                  "TBps": round(moved / (med * 1e-3) / 1e12, 3), "MPps": round(n * w * h / 1e6 / (med * 1e-3), 1)}
            print(f"  {name} {label} {kernel}: {med:.4f} ms", file=sys.stderr, flush=True)
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
