"""Static guard (no GPU: hipcc cross-compiles and reports resource usage) on the trellis stage's kernels and on the forward
stage they were added beside: the raw form of jpeg_forward_fused_kernel is a sibling instantiation, and the quantising
instantiations the encode path's timings depend on must come out as they did before it existed."""
import os
import re

import pytest

from imageflow_amd import build as B
from tests.test_kernel_resources import _int, resource_usage

# VGPRs, LDS bytes per workgroup, scratch bytes per lane of the quantising instantiations, measured with this function on a
# build of the revision before the raw form was added (jpeg_forward_fused_kernel<HS, VS>)
FORWARD_BEFORE = {(1, 1): (41, 19200, 0), (2, 1): (41, 17152, 0), (2, 2): (42, 19456, 0)}


@pytest.fixture(scope="module")
def forward_rows():
    return resource_usage(os.path.join(B.CSRC, "jpeg_forward.hip"))


def test_trellis_kernels_keep_four_waves_per_simd_without_scratch():
    rows = resource_usage(os.path.join(B.CSRC, "jpeg_trellis.hip"))
    for name in ("trellis_search_kernel", "trellis_plain_kernel", "trellis_table_kernel"):
        r = rows[name]
        assert _int(r, "ScratchSize [bytes/lane]") == 0, (name, r)
        assert _int(r, "LDS Size [bytes/block]") <= 64 * 1024, (name, r)
        assert _int(r, "VGPRs") <= 512 // 4, (name, r)                  # 512 registers per SIMD lane: 4 waves of 128
        assert _int(r, "Occupancy [waves/SIMD]") >= 4, (name, r)


@pytest.mark.parametrize("hs,vs", sorted(FORWARD_BEFORE))
def test_forward_instantiations_are_what_they_were(forward_rows, hs, vs):
    found = [r for n, r in forward_rows.items() if re.match(rf"void jpeg_forward_fused_kernel<{hs}, {vs}(, false)?>$", n)]
    assert len(found) == 1, list(forward_rows)
    r = found[0]
    assert (_int(r, "VGPRs"), _int(r, "LDS Size [bytes/block]"), _int(r, "ScratchSize [bytes/lane]")) == FORWARD_BEFORE[(hs, vs)], r


def test_raw_instantiations_exist_without_scratch(forward_rows):
    raw = [r for n, r in forward_rows.items() if re.match(r"void jpeg_forward_fused_kernel<\d, \d, true>$", n)]
    assert len(raw) == 3 and all(_int(r, "ScratchSize [bytes/lane]") == 0 for r in raw), list(forward_rows)
