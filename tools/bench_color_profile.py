#!/usr/bin/env python3
"""The colour conversion kernel on batches of frames (tools/bench_color_profile.py [--case NAME] [--reps N]).  Cases: 1 and 32
frames of 800x450 and 8 frames of 3840x2160, each on photo-like content and on random bytes (the worst case for the LDS
tables: no two neighbours share a table entry), with a Display P3 plan.  Per case one JSON line: the launch's time between two
device events on its stream (median over the repetitions; the frames are restored from a pristine copy before each one, outside
the events, because the conversion is in place), the bytes it moves -- every pixel read once and written once, 2 x the frame
bytes -- per second, and next to it the memory system's own figure for that mix from csrc/bandwidth_probes.cpp: one 16-byte
vector written per vector read, and the device-to-device copy.  The 800x450x1 case measures a launch, not a stream.

Before anything is timed the device's bytes are compared with the CPU emulation's on one frame of the case.

Without --case every case runs as a child process of its own under `timeout -k 10`, one after the other, and the first that
fails ends the run: nothing more is started on a device that has just faulted or hung."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# n, w, h, reps, time limit s
CASES = {"800x450x1": (1, 800, 450, 200, 200), "800x450x32": (32, 800, 450, 100, 200), "2160p_x8": (8, 3840, 2160, 30, 300)}


def run_case(name, reps=None):
    import numpy as np
    import torch
    from imageflow_amd import _native
    from imageflow_amd.codecs import color_profile as CP
    from imageflow_amd.graphics.bitmaps import Bitmap
    from bench_png_encode import photo_frames
    from tests import color_profile_emulation as E
    from tests.test_jpeg_headers import P3_XYZ, make_icc
    n, w, h, default_reps, _ = CASES[name]
    reps = reps or default_reps
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    icc = make_icc(xyz=P3_XYZ)
    plan, emulated = CP.plan_from_icc(icc), E.plan_from_icc(icc)[1]
    moved = 2 * n * h * w * 4
    res = {"case": name, "frames": n, "w": w, "h": h, "reps": reps, "bytes_moved": moved, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator(device=dev).manual_seed(11)
    contents = {"photo": photo_frames(n, w, h, stride, dev, True),
                "random": torch.randint(0, 256, (n, h * stride), dtype=torch.uint8, device=dev, generator=g)}
    for label, pristine in contents.items():
        bm = Bitmap(pristine.clone(), w, h, stride, alpha_meaningful=True)
        CP.transform_to_srgb(bm, plan)                                   # warm-up, and the check
        torch.cuda.synchronize()
        last = n - 1
        want = E.transform(pristine[last].view(h, stride).cpu().numpy(), w, emulated)
        got = bm.data[last].view(h, stride).cpu().numpy()
        assert np.array_equal(got[:, :4 * w], want[:, :4 * w]), "the device's bytes differ from the emulation's"
        ms = []
        for _ in range(reps):
            bm.data.copy_(pristine)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            CP.transform_to_srgb(bm, plan)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        res[label] = {"launch_ms": round(med, 4), "min_ms": round(float(np.min(ms)), 4), "p90_ms": round(float(np.percentile(ms, 90)), 4),
                      "TBps": round(moved / (med * 1e-3) / 1e12, 3), "MPps": round(n * w * h / 1e6 / (med * 1e-3), 1)}
        print(f"  {name} {label}: {med:.4f} ms", file=sys.stderr, flush=True)
    L = _native.lib()
    L.ifhip_measure_mixed_bandwidth.argtypes = [C.c_size_t, C.c_uint32, C.c_int, C.POINTER(C.c_double)]
    bps = C.c_double(0)
    probe_bytes = 1 << 30
    _native.check(L.ifhip_measure_mixed_bandwidth(probe_bytes, 1, 5, C.byref(bps)))          # one vector written per vector read
    res["probe_one_write_per_read_TBps"] = round(bps.value / 1e12, 3)
    _native.check(L.ifhip_measure_copy_bandwidth(probe_bytes, 5, C.byref(bps)))
    res["probe_copy_TBps"] = round(bps.value / 1e12, 3)
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
