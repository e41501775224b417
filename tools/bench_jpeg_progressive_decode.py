#!/usr/bin/env python3
"""The device progressive JPEG decoder against the route it replaces (tools/bench_jpeg_progressive_decode.py [--case NAME]
[--reps N]).  Inputs: Pillow progressive files of the photo-like frame at quality 85, 4:2:0.  Cases: one file of 800x450, 32
of them in one batch, one of 3840x2160.  Per case one JSON line, after a warm-up:

  prepare_ms            the host front end (marker walk, un-stuffing, stream records), all files, one core
  device_call_ms        ifhip_jpeg_progressive_decode_batch_device with its upload, to the end of the last kernel (wall clock
                        around a synchronise; median)
  clear_ms, level_ms[]  the clear and each level's launch, from hipEvents around calls that the development switch
                        jpeg_progressive_stop_after ends behind a launch, by difference (the first figure holds the upload)
  host_route_ms         ifhip_jpeg_read_coefficients_host on one core plus the upload of its planes: the route of a job with
                        the switch off

The planes are compared with the host reader's before anything is timed.  Without --case every case runs as a child process
of its own under `timeout -k 10`, one after the other, and the first that fails ends the run: nothing more is started on a
device that has just faulted or hung."""
import ctypes as C
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# files, w, h, reps, time limit s
CASES = {"800x450x1": (1, 800, 450, 9, 200), "800x450x32": (32, 800, 450, 7, 300), "2160p_x1": (1, 3840, 2160, 5, 400)}


def photo(w, h, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [128 + 90 * np.sin(x / (37.0 + 9 * k) + k + seed) * np.cos(y / (41.0 - 6 * k)) + 25 * ((x // 64 + y // 48) % 2) + rng.normal(0, 4, (h, w)) for k in range(3)]
    return np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)


def run_case(name, reps=None):
    import numpy as np
    import torch
    from PIL import Image
    from imageflow_amd import _native
    from imageflow_amd.codecs import jpeg_progressive_decoder as D
    n, w, h, default_reps, _ = CASES[name]
    reps = reps or default_reps
    dev = "cuda:0"
    files = []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(photo(w, h, i)).save(buf, "JPEG", quality=85, subsampling="4:2:0", progressive=True)
        files.append(buf.getvalue())
    L = _native.lib()
    L.ifhip_jpeg_read_coefficients_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def med(ts):
        return float(np.median(ts))

    ts = []
    for _ in range(max(3, reps)):
        t0 = time.perf_counter()
        prepared = [D.PreparedProgressive(f) for f in files]
        ts.append((time.perf_counter() - t0) * 1e3)
    prepare_ms = med(ts)
    coef, status = D.decode_batch_device(prepared, device=dev)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    host = [[np.zeros(p.plane_shape(c), np.int16) for c in range(3)] for p in prepared]
    qt = np.zeros((3, 64), np.uint16)

    def host_route():
        t0 = time.perf_counter()
        up = []
        for f, planes in zip(files, host):
            _native.check(L.ifhip_jpeg_read_coefficients_host(f, len(f), planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, qt.ctypes.data))
            up += [torch.from_numpy(p).to(dev, non_blocking=False) for p in planes]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, up

    _, up = host_route()
    for i in (0, n - 1):
        for c in range(3):
            assert torch.equal(coef[i][c], up[3 * i + c]), "device planes differ from the host reader's"
    host_ms = med([host_route()[0] for _ in range(max(3, reps))])

    def call(stop=None, events=False):
        _native.debug_set("jpeg_progressive_stop_after", stop)
        out = []
        for k in range(reps + 1):                                     # the first is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            D.decode_batch_device(prepared, coef, status, dev)
            e1.record()
            torch.cuda.synchronize()
            if k:
                out.append(e0.elapsed_time(e1) if events else (time.perf_counter() - t0) * 1e3)
        _native.debug_set("jpeg_progressive_stop_after", None)
        return med(out)

    whole = call()
    levels = max(p.n_levels for p in prepared)
    steps = [call(str(k), events=True) for k in range(levels + 1)]
    res = {"case": name, "files": n, "w": w, "h": h, "reps": reps, "device": torch.cuda.get_device_name(0), "file_bytes": sum(len(f) for f in files),
           "scans": prepared[0].n_scans, "streams": sum(p.n_streams for p in prepared), "levels": levels,
           "prepare_ms": round(prepare_ms, 3), "device_call_ms": round(whole, 3), "upload_and_clear_ms": round(steps[0], 3),
           "level_ms": [round(steps[k + 1] - steps[k], 3) for k in range(levels)], "host_route_ms": round(host_ms, 3),
           "prepare_plus_call_over_host_route": round((prepare_ms + whole) / host_ms, 2), "MPps_device_call": round(n * w * h / 1e6 / (whole * 1e-3), 2)}
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
