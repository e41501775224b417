#!/usr/bin/env python3
"""Research tool (GPU): record what the resample launcher decides -- kernel and geometry -- for a fixed list of cases, one JSON
object per case, as tests/golden/launch_geometry.jsonl.  Every case is launched for real through
ifhip_scale_and_render_batch_device (the planar-YCbCr case through ifhip_jpeg_decode_resample_batch_device) with the
`trace_launch` switch set, and the line the library prints is stored next to the inputs; `generic` stands for the generic
two-pass kernels, a bare status for a call that failed.  tests/test_launch_plan.py asks ifhip_describe_launch (host only) for
the same cases and expects the same lines, so an intended change of launch geometry is made by running this tool again:
    python tools/record_launch_geometry.py [OUT.jsonl]
One process, every case once."""
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.scan_shapes import FILTERS, SHAPES  # noqa: E402

F = {"Robidoux": 2, "Ginseng": 4, "Lanczos": 6}
# every resample shape of the five BASELINE configs with bench.py's frame counts: (in_w, in_h, w, h, filter, sharpen, alpha, frames)
BASELINE_SHAPES = [
    (480, 270, 200, 113, F["Robidoux"], 0.0, 0, 4096),          # cfg1's resize
    (3840, 2160, 200, 200, F["Robidoux"], 0.0, 0, 256),         # cfg2
    (3840, 2160, 1600, 900, F["Robidoux"], 0.0, 0, 128),        # cfg3: the four levels of the pyramid
    (1600, 900, 1200, 675, F["Robidoux"], 0.0, 0, 128),
    (1600, 900, 800, 450, F["Robidoux"], 0.0, 0, 128),
    (1200, 675, 400, 225, F["Robidoux"], 0.0, 0, 128),
    (1920, 1080, 800, 450, F["Robidoux"], 0.0, 0, 64),          # cfg4's resize from a BGRA bitmap
    (7680, 4320, 400, 225, F["Lanczos"], 15.0, 1, 64),          # cfg5
]
CFG2 = (3840, 2160, 200, 200, F["Robidoux"], 0.0, 0, 256)
HD_UP = (960, 540, 1920, 1080, F["Ginseng"], 0.0, 0, 8)
# source rows of 4*w bytes, a multiple of 4 but not of 16: the fused kernel's 16-byte row reads do not apply
ODD_STRIDES = [(1001, 667, 500, 333, F["Robidoux"], 0), (1001, 667, 500, 333, F["Robidoux"], 1), (799, 599, 200, 150, F["Lanczos"], 0),
               (333, 500, 999, 1500, F["Ginseng"], 1), (1921, 1081, 641, 361, F["Robidoux"], 0), (150, 150, 48, 48, F["Robidoux"], 0)]


def stride64(w):
    return (w * 4 + 63) // 64 * 64


def case(in_w, in_h, w, h, filt, sharpen, alpha, n, stride=None, force_kernel=-1, cu_budget=0, ycc=0):
    st = stride or stride64(in_w)
    return {"in_w": in_w, "in_h": in_h, "w": w, "h": h, "filter": int(filt), "sharpen": sharpen, "alpha": alpha, "ycc": ycc,
            "n_images": n, "in_stride": st, "in_image_bytes": in_h * st, "align": 256, "working_space": 1,
            "force_kernel": force_kernel, "cu_budget": cu_budget}


def cases():
    out = []
    for alpha in (0, 1):
        for (iw, ih, ow, oh) in SHAPES:
            for filt in FILTERS:
                out.append(case(iw, ih, ow, oh, filt, 0.0, alpha, max(1, min(256, int(1.5e9 // (iw * ih * 4 + ow * oh * 4))))))
    for s in BASELINE_SHAPES:
        out.append(case(*s))
        out.append(case(*s[:7], 1))
    for s in (CFG2, HD_UP):
        for fk in (0, 1, 2):
            out.append(case(*s, force_kernel=fk))
        out.append(case(*s, cu_budget=224))
    for (iw, ih, ow, oh, filt, alpha) in ODD_STRIDES:
        out.append(case(iw, ih, ow, oh, filt, 0.0, alpha, 16, stride=4 * iw))
    # cfg4 from the planar-YCbCr path: 3840x2160 4:2:0 decoded at 4/8; the three planes are 1920x1080 samples, pitch 1920
    c = case(1920, 1080, 800, 450, F["Robidoux"], 0.0, 0, 64, stride=1920, ycc=1)
    c["in_image_bytes"] = 1920 * 1080
    out.append(c)
    return out


class Stderr:
    """What the library writes to file descriptor 2 during one call."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()


def main():
    import numpy as np
    import torch

    from imageflow_amd import _native
    from imageflow_amd.codecs import mozjpeg_decoder as D
    from imageflow_amd.graphics.bitmaps import Bitmap
    from imageflow_amd.graphics.scaling import ResamplePlan, ScaleAndRenderParams

    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "launch_geometry.jsonl")
    dev = torch.device("cuda:0")
    L = _native.lib()
    _native.debug_set("trace_launch", "1")
    plans = {}
    lines = []
    for c in cases():
        key = (c["in_w"], c["in_h"], c["w"], c["h"], c["filter"], c["sharpen"])
        if key not in plans:
            plans[key] = ResamplePlan(*key)
        plan = plans[key]
        can = Bitmap.create_u8(c["n_images"], c["w"], c["h"], dev)
        _native.set_cu_budget(c["cu_budget"])
        with Stderr() as err:
            if c["ycc"]:
                stage = D.JpegPixelStage(2 * c["in_w"], 2 * c["in_h"], 3, [2, 1, 1], [2, 1, 1], c["n_images"], device=str(dev), scale_num=4,
                                         luma_spatial=True, luma_srgb=True)
                coef = [torch.zeros((c["n_images"], stage.blocks_h[k], stage.blocks_w[k], 64), dtype=torch.int16, device=dev) for k in range(3)]
                qt = torch.ones((c["n_images"], 3, 64), dtype=torch.int16, device=dev)
                fused = stage.read_frames_into(coef, qt, can, ScaleAndRenderParams(0, 0, c["w"], c["h"]), plan=plan)
                rc = 0 if fused else -1
            else:
                src = torch.empty((c["n_images"], c["in_image_bytes"]), dtype=torch.uint8, device=dev)
                assert src.data_ptr() % c["align"] == 0
                rc = L.ifhip_scale_and_render_batch_device(
                    plan.handle, src.data_ptr(), c["in_image_bytes"], c["in_stride"], c["alpha"], c["n_images"], can.data.data_ptr(),
                    can.image_bytes, can.w, can.h, can.stride, 0, 0, c["working_space"], int(can.compose), int(can.matte), None,
                    c["force_kernel"], C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            torch.cuda.synchronize()
        traced = [ln for ln in err.text.splitlines() if ln.startswith("ifhip ") and " launch" in ln]
        rec = dict(c)
        if rc:
            rec["status"] = rc
        elif not traced or traced[-1].startswith("ifhip generic launch"):
            rec["line"] = "generic"
        else:
            rec["line"] = traced[-1]
        lines.append(json.dumps(rec))
        del can
    _native.set_cu_budget(0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} cases -> {out_path}")


if __name__ == "__main__":
    main()
