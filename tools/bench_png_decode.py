#!/usr/bin/env python3
"""The device PNG decoder on batches of files (tools/bench_png_decode.py [--case NAME] [--reps N]).  Cases: 32 files of
800x450 RGBA, 8 files of 3840x2160 RGBA, one 256x256 RGBA logo -- the first two are the encoder's own shapes, every file
once as the device coder wrote it and once with the same filtered stream deflated by zlib level 6.  Per case one JSON line:
the whole call (host chunk walk, upload, three launches, wait) for the batch and for the same files one call at a time,
the stages' times by difference (the development switch png_decode_stop_after ends the call behind inflate / un-filter),
and the yardstick: one host thread's zlib.decompress of the same streams, timed in the same run, as a ratio.

Without --case every case runs as a child process of its own under `timeout -k 10`, one after the other, and the first
that fails ends the run: nothing more is started on a device that has just faulted or hung."""
import json
import os
import struct
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# n, w, h, reps, time limit s.  Inflate runs one wave per stream at a few MB/s, so a repetition of the 2160p batch takes seconds
# and one of its files one by one a minute: that case is timed once, without a warm-up call.
CASES = {"800x450x32": (32, 800, 450, 3, 300), "logo_256": (1, 256, 256, 20, 120), "2160p_x8": (8, 3840, 2160, 1, 900)}


def chunk(tag, data=b""):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def idat(data):
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        if data[at + 4:at + 8] == b"IDAT":
            out.append(data[at + 8:at + 8 + n])
        at += 12 + n
    return b"".join(out)


def with_stream(data, z):
    """the file with its IDAT replaced by one chunk holding z"""
    at = data.index(b"IDAT") - 4
    return data[:at] + chunk(b"IDAT", z) + chunk(b"IEND")


def run_case(name, reps=None):
    import numpy as np
    import torch
    from imageflow_amd import _native
    from imageflow_amd.codecs import libpng_decoder as D
    from imageflow_amd.codecs import libpng_encoder as E
    from imageflow_amd.graphics.bitmaps import Bitmap
    from bench_png_encode import photo_frames
    n, w, h, default_reps, _ = CASES[name]
    reps = reps or default_reps
    dev = "cuda:0"
    stride = (w * 4 + 63) // 64 * 64
    bm = Bitmap(photo_frames(n, w, h, stride, dev, True), w, h, stride, alpha_meaningful=True)
    device_files = E.encode_png(bm)
    raw = [zlib.decompress(idat(f)) for f in device_files]
    zlib_files = [with_stream(f, zlib.compress(r, 6)) for f, r in zip(device_files, raw)]
    want = bm.data.view(n, h, stride)[:, :, :4 * w].cpu().numpy()
    res = {"case": name, "files": n, "w": w, "h": h, "reps": reps, "device": torch.cuda.get_device_name(0)}
    for label, files in (("device_coder", device_files), ("zlib6", zlib_files)):
        frames = [Bitmap(torch.zeros((1, h * stride), dtype=torch.uint8, device=dev), w, h, stride, True) for _ in range(n)]

        def timed(call, stop=None, reps=reps):
            _native.debug_set("png_decode_stop_after", stop)
            if reps > 1:
                call()                                               # warm-up
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            _native.debug_set("png_decode_stop_after", None)
            print(f"  {name} {label} {call.__name__} stop_after={stop}: {np.median(ts):.3f} ms", file=sys.stderr, flush=True)
            return float(np.median(ts))

        def batch():
            _, st = D.decode_png_batch(files, dev, frames=frames)
            assert not any(st), st

        def one_by_one():
            for f, fr in zip(files, frames):
                _, st = D.decode_png_batch([f], dev, frames=[fr])
                assert not any(st), st
        whole = timed(batch)
        got = torch.stack([f.data.view(h, stride)[:, :4 * w] for f in frames]).cpu().numpy()
        assert np.array_equal(got, want), "decoded frames differ from the source"
        t_inf, t_unf = timed(batch, "inflate"), timed(batch, "unfilter")
        serial = timed(one_by_one, reps=1) if n > 1 else whole
        streams = [idat(f) for f in files]
        ts = []
        for _ in range(max(3, reps // 2)):
            t0 = time.perf_counter()
            for s in streams:
                zlib.decompress(s)
            ts.append((time.perf_counter() - t0) * 1e3)
        host = float(np.median(ts))
        res[label] = {"stream_bytes": sum(len(s) for s in streams), "batch_ms": round(whole, 3), "one_by_one_ms": round(serial, 3),
                      "inflate_ms": round(t_inf, 3), "unfilter_ms": round(t_unf - t_inf, 3), "expand_ms": round(whole - t_unf, 3),
                      "host_zlib_decompress_one_thread_ms": round(host, 3), "inflate_over_host": round(t_inf / host, 2),
                      "batch_over_host": round(whole / host, 2), "MPps": round(n * w * h / 1e6 / (whole * 1e-3), 1)}
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
