"""CPU half of the op-level test of `hamt_attn_cls_fwd` (one query per (image, head): the cls row of the ViT's last block).  Before
test_gpu_extract.py relies on the cases and the bound of tests/_attn_cls_ref.py, this file shows that
  1. the cases hold what they claim (every Sk around the 64-lane and 8-key steps, both dtypes, a +90 / -90 row, equal keys);
  2. the kernel's arithmetic restated in numpy float32 stays under the cap `MEASURED` (the GPU bound is 8 x the cap);
  3. each mistake the GPU half is meant to catch exceeds that bound tenfold on the cases;
  4. the entry point is declared, bound and built, and its gfx950 code uses no scratch and spills nothing."""
import os
import re
import subprocess

import numpy as np
import pytest

import _attn_cls_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_have_what_the_gpu_half_needs():
    cs = R.cases()
    assert sorted({c["Sk"] for c in cs}) == [1, 5, 63, 64, 65, 197, 256]
    for Sk in R.SKS:
        assert {c["dtype"] for c in cs if c["Sk"] == Sk} == {"fp32", "bf16"}
    assert any(c["pad_q"] for c in cs) and any(c["pad_kv"] for c in cs) and any(not c["pad_q"] and not c["pad_kv"] for c in cs)
    for c in cs:
        assert c["q"].shape == (R.N_IMG, R.H) and c["k"].shape == c["v"].shape == (R.N_IMG * c["Sk"], R.H)
        if c["dtype"] == "bf16":                                    # already rounded: the kernel and float64 see identical inputs
            assert all(np.array_equal(R.to_bf16(c[t]), c[t]) for t in "qkv")
    for c in (c for c in cs if "+-90" in c["name"]):
        s = (c["q"][0, :R.DH].astype(np.float64) * c["k"][:c["Sk"], :R.DH].astype(np.float64)).sum(1) * R.SCALE
        assert s[3] == 90.0 and s[64] == -90.0 and np.abs(np.delete(s, [3, 64])).max() < 30
    eq = [c for c in cs if "equal" in c["name"]][0]
    assert all((eq["k"][b * eq["Sk"]:(b + 1) * eq["Sk"]] == eq["k"][b * eq["Sk"]]).all() for b in range(R.N_IMG))
    want = R.attn_cls_f64(eq["q"], eq["k"], eq["v"], eq["Sk"])
    assert np.allclose(want, eq["v"].astype(np.float64).reshape(R.N_IMG, eq["Sk"], R.H).mean(1), atol=1e-12)


def test_fp32_restatement_is_under_the_cap():
    worst = 0.0
    for c in R.cases():
        e = R.errors(c, R.attn_cls32(c["q"], c["k"], c["v"], c["Sk"])).max()
        print(f"[attn_cls fp32 restatement] {c['name']}: {e:.3f} units")
        worst = max(worst, e)
    print(f"[attn_cls fp32 restatement] worst {worst:.3f} units (cap {R.MEASURED}, GPU bound {R.BOUND})")
    assert R.MEASURED / 2 <= worst <= R.MEASURED and R.BOUND == 8 * R.MEASURED


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_cases_catch(mistake):
    worst = max(R.errors(c, R.attn_cls32(c["q"], c["k"], c["v"], c["Sk"], mistake)).max() for c in R.cases())
    print(f"[attn_cls {mistake}] worst case error {worst:.3g} units = {worst / R.BOUND:.3g} x the GPU bound")
    assert worst >= 10 * R.BOUND
    if mistake == "no_max":                     # only the row with a score above 88 can tell
        rest = max(R.errors(c, R.attn_cls32(c["q"], c["k"], c["v"], c["Sk"], mistake)).max() for c in R.cases() if "+-90" not in c["name"])
        assert rest <= R.BOUND


def test_symbol_in_header_binding_and_build():
    from vln_hamt_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "hamt.h")).read()
    m = re.search(r"\bint\s+hamt_attn_cls_fwd\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES["hamt_attn_cls_fwd"]) == 6
    assert '"attn_cls.hip"' in open(os.path.join(ROOT, "vln_hamt_amd", "csrc", "build.py")).read()
    assert callable(ops.attn_cls)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert hasattr(lib, "hamt_attn_cls_fwd") and lib.hamt_version() == 2        # an added entry point leaves the ABI number alone


def test_attn_cls_fails_loudly_without_gpu():
    import torch
    from vln_hamt_amd import ops
    from vln_hamt_amd._lib import HamtError
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(HamtError):
        ops.attn_cls(torch.zeros(2, 128), torch.zeros(10, 128), torch.zeros(10, 128), 2)


def test_attn_cls_kernels_use_no_scratch(tmp_path):
    """The cross-compiled gfx950 code object of attn_cls.hip: no scratch memory, no spilled registers, 1 KB of LDS (read as
    tests/test_eval_ref.py does)."""
    from test_kernel_resources import OBJCOPY, READELF, _code_objects
    from vln_hamt_amd import _lib
    assert "hamt_attn_cls_fwd" in _lib.SIGNATURES
    if not (os.path.exists(READELF) and os.path.exists(OBJCOPY)):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = []
    for co in _code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or "attn_cls_fwd_kernel" not in name.group(1):
                continue
            num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
            seen.append(name.group(1))
            print(name.group(1), "vgprs", num("vgpr_count"), "sgprs", num("sgpr_count"), "lds", num("group_segment_fixed_size"))
            assert num("vgpr_spill_count") == 0 and num("sgpr_spill_count") == 0 and num("private_segment_fixed_size") == 0, (name.group(1), blk)
            assert num("group_segment_fixed_size") == 1024 and num("vgpr_count") <= 64, name.group(1)
    assert len(seen) == 2, seen                  # bf16 and fp32 inputs
