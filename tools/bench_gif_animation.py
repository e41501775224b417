#!/usr/bin/env python3
"""An animated GIF through a job: decode -> resample_2d -> encode gif (tools/bench_gif_animation.py [frames] [w h] [--all]).
Prints one JSON line per shape with two wall-clock times, each the median (and the least and the most) of five runs after a
warm-up run; a run ends with the output buffer in host memory:

  animation_job   ONE job on a context with Context.set_gif_animation and Context.set_gif_encoder on: the source's screens
                  decoded once, the node chain run per frame, the frames coded in one call into one animated file;
  n_jobs_route    the same pictures on the route there was before: N jobs with {"select_frame": k}, each decoding and
                  composing frames 0 .. k again and each writing a one-frame file (which nobody has yet joined into one).

--all: the two shapes of DESIGN section 6, a synthetic 32-frame and a 3-frame 800 x 450 animation.  The source is written by
the device coder itself from photo-like frames that drift from frame to frame."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(32, 800, 450), (3, 800, 450)]


def source(n, w, h, dev):
    """an n-frame animation of w x h: one photo-like frame rolled a few columns further in every frame, full frames, local tables"""
    import torch
    from imageflow_amd.codecs import gif_encoder as GIF
    from imageflow_amd.graphics.bitmaps import Bitmap
    from tools.bench_png_encode import photo_frames
    stride = (w * 4 + 63) // 64 * 64
    base = photo_frames(1, w, h, stride, dev, False).view(h, stride)[:, :4 * w].reshape(h, w, 4)
    frames = torch.zeros((n, h, stride), dtype=torch.uint8, device=dev)
    for k in range(n):
        frames[k, :, :4 * w] = torch.roll(base, shifts=7 * k, dims=1).reshape(h, 4 * w)
    bm = Bitmap(frames.view(n, h * stride), w, h, stride, alpha_meaningful=False)
    return GIF.GifEncodeStage(w, h, min(n, 32), dev).encode_animation(bm, [4] * n, [False] * n, repeat=0)


def job(c, msg, src):
    c.add_input_buffer(0, src)
    c.add_output_buffer(1)
    status, r = c.send_json("v1/execute", msg)
    assert status == 200, r
    return bytes(c.get_output_buffer(1))


def one_shape(n, w, h):
    import torch
    from imageflow_amd.abi import Context
    from imageflow_amd.codecs import gif_decoder as D
    dev = "cuda:0"
    src = source(n, w, h, dev)
    ow, oh = w // 2, h // 2
    chain = [{"resample_2d": {"w": ow, "h": oh}}, {"encode": {"io_id": 1, "preset": "gif"}}]

    def animation_job():
        with Context() as c:
            assert c.set_gif_encoder(True) and c.set_gif_animation(True)
            return job(c, {"framewise": {"steps": [{"decode": {"io_id": 0}}] + chain}}, src)

    def n_jobs_route():
        out = []
        for k in range(n):
            with Context() as c:
                assert c.set_gif_encoder(True)
                out.append(job(c, {"framewise": {"steps": [{"decode": {"io_id": 0, "commands": [{"select_frame": k}]}}] + chain}}, src))
        return out

    def timed(f):
        f()
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(t)), 2), [round(min(t), 2), round(max(t), 2)]

    res = {"frames": n, "w": w, "h": h, "out_w": ow, "out_h": oh, "source_bytes": len(src), "device": torch.cuda.get_device_name(0)}
    animated, singles = animation_job(), n_jobs_route()
    assert D.gif_frame_count(animated)[0] == n and len(singles) == n
    screens, _ = D.decode_gif_frames(animated, dev)                  # the two routes hold the same pictures
    for k in (0, n - 1):
        one = D.decode_gif(singles[k], 0, dev)
        assert torch.equal(screens.data[k], one.data[0]), k
    res["animation_bytes"], res["n_jobs_bytes"] = len(animated), sum(len(f) for f in singles)
    res["animation_job_ms"], res["animation_job_ms_min_max"] = timed(animation_job)
    res["n_jobs_route_ms"], res["n_jobs_route_ms_min_max"] = timed(n_jobs_route)
    res["animation_job_ms_per_frame"] = round(res["animation_job_ms"] / n, 3)
    res["n_jobs_route_ms_per_frame"] = round(res["n_jobs_route_ms"] / n, 3)
    res["n_jobs_over_animation"] = round(res["n_jobs_route_ms"] / res["animation_job_ms"], 2)
    return res


def main():
    nums = [int(v) for v in sys.argv[1:] if v.isdigit()]
    shapes = SHAPES if "--all" in sys.argv or not nums else [(nums[0],) + ((nums[1], nums[2]) if len(nums) >= 3 else (800, 450))]
    for n, w, h in shapes:
        print(json.dumps(one_shape(n, w, h)), flush=True)


if __name__ == "__main__":
    main()
