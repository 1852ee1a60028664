"""Not gpu: the gfx950 code objects of the PACKED form of `attn_wide_bwd_kernel` (the backward of the packed attention calls with 129 .. 256
tokens on a side) inside libhamt_hip.so, read the way tests/test_kernel_resources.py reads the hot kernels.  Sixteen waves per workgroup
leave 128 registers per lane: a spill still passes every comparison and runs out of scratch memory."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import OBJCOPY, READELF, _code_objects  # noqa: E402


@pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJCOPY)), reason="ROCm LLVM tools not installed")
def test_packed_wide_backward_has_no_spills_and_no_scratch(tmp_path):
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    found = {}
    for co in _code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            m = name and re.search(r"attn_wide_bwd_kernelI(..)Lb1EEE", name.group(1))     # <TI, TO, PACKED = true>
            if m:
                found[m.group(1)] = tuple(int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
                                          for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "vgpr_count"))
    assert set(found) == {"ff", "tt", "tf", "ft"}, found            # fp32 / bf16 in x fp32 / bf16 out
    for io, (vgpr_spill, sgpr_spill, scratch, vgpr) in found.items():
        assert (vgpr_spill, sgpr_spill, scratch) == (0, 0, 0), (io, found[io])
        assert vgpr <= 128, (io, vgpr)                               # 1024 threads per workgroup: four waves per SIMD
