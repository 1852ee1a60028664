"""Not gpu: the gfx950 code object of `pretrain_gather_kernel` inside libhamt_hip.so, read the way tests/test_kernel_resources.py reads the
hot kernels.  A row gather that spills runs out of scratch memory at a fraction of the HBM rate and still passes every comparison:
refuse any spill and any scratch."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import OBJCOPY, READELF, _code_objects  # noqa: E402


@pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJCOPY)), reason="ROCm LLVM tools not installed")
def test_pretrain_gather_kernel_has_no_spills_and_no_scratch(tmp_path):
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    found = []
    for co in _code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and "pretrain_gather_kernel" in name.group(1):
                found.append((int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)), int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                              int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)), int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                              int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))))
    assert len(found) == 1, found
    vgpr_spill, sgpr_spill, scratch, vgpr, lds = found[0]
    assert (vgpr_spill, sgpr_spill, scratch, lds) == (0, 0, 0, 0), found[0]
    assert vgpr <= 128, vgpr                    # four waves per SIMD at the least: the kernel hides its latency by occupancy alone
