"""Static guard on the colour conversion kernel (no GPU: hipcc cross-compiles and reports resource usage, as
tests/test_kernel_resources.py does for the kernels that set the headline numbers; imageflow_amd/kernel_report.py prints the
same report).  The kernel is memory-bound: scratch traffic would share its load counter, and its LDS is what fixes how many
workgroups share a CU."""
import os

from imageflow_amd import build as B
from tests.test_kernel_resources import _int, resource_usage


def test_color_transform_kernel_uses_no_scratch_and_the_lds_the_design_states():
    rows = resource_usage(os.path.join(B.CSRC, "color_profile.hip"))
    kernels = [r for n, r in rows.items() if "color_transform_kernel" in n]
    assert len(kernels) == 1, sorted(rows)
    r = kernels[0]
    assert _int(r, "ScratchSize [bytes/lane]") == 0, r
    assert _int(r, "LDS Size [bytes/block]") == 3 * 256 * 8 * 4 + 16384 == 40960, r      # eight copies of three f32 tables + the linear->sRGB bytes
    assert _int(r, "VGPRs") <= 64, r                                                    # 1 024 lanes: 128 at the most; two workgroups a CU need 64
    design = open(os.path.join(os.path.dirname(B.CSRC), "..", "DESIGN.md")).read()
    assert "4.14" in design and "40 960" in design
