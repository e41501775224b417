"""The launch planner (csrc/resample_plan.cpp) against tests/golden/launch_geometry.jsonl: for every case recorded from real
launches on the MI355X (tools/record_launch_geometry.py), ifhip_describe_launch -- host only, no GPU -- gives the recorded line
byte for byte.  A change of launch geometry is made on purpose, by recording the file again."""
import json
import os

import pytest

from imageflow_amd import _native
from imageflow_amd.errors import FlowError
from imageflow_amd.graphics.scaling import describe_launch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_geometry.jsonl")
CASES = [json.loads(line) for line in open(GOLDEN) if line.strip()]


def _describe(c):
    _native.set_cu_budget(c["cu_budget"])
    try:
        return describe_launch(c["in_w"], c["in_h"], c["w"], c["h"], c["filter"], c["sharpen"], c["alpha"], c["ycc"], c["n_images"],
                               c["in_stride"], c["in_image_bytes"], c["align"], c["working_space"], c["force_kernel"])
    finally:
        _native.set_cu_budget(0)


def _id(c):
    return "{in_w}x{in_h}-{w}x{h}-f{filter}-a{alpha}-n{n_images}-s{in_stride}-k{force_kernel}-cu{cu_budget}-y{ycc}".format(**c)


def test_golden_file_covers_the_kernels():
    lines = [c.get("line", "") for c in CASES]
    assert len(CASES) >= 281
    assert any(ln.startswith("ifhip fused launch:") for ln in lines)
    assert any(ln.startswith("ifhip banded launch:") for ln in lines)
    assert any(ln.startswith("ifhip banded launch (instead of") for ln in lines)
    assert any(ln == "generic" for ln in lines)
    assert any("status" in c for c in CASES) and any(c["ycc"] for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_launch_decision_matches_the_recorded_launch(c):
    if "status" in c:
        with pytest.raises(FlowError) as e:
            _describe(c)
        assert int(e.value.kind) == c["status"]
    elif c["line"] == "generic":
        assert _describe(c).startswith("ifhip generic launch: %dx%d -> %dx%d " % (c["in_w"], c["in_h"], c["w"], c["h"]))
    else:
        assert _describe(c) == c["line"]
