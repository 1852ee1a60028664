"""Not gpu: RangerLars (Ralamb + Lookahead, optim/rangerlars.py) -- the factory and its parameter groups, the host coefficients
against the reference's formulas, the static item table, the fixture against its generator, the new kernels' registers."""
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from _util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Tiny(torch.nn.Module):
    """parameter names of the reference's model kinds: decayed weights, biases, 'LayerNorm.weight', a lower-case layer_norm gain"""

    def __init__(self):
        super().__init__()
        self.dense = torch.nn.Linear(8, 8)
        self.LayerNorm = torch.nn.LayerNorm(8)
        self.layer_norm = torch.nn.LayerNorm(8)
        self.emb = torch.nn.Embedding(10, 8)


def test_build_optimizer_rangerlars_groups():
    from vln_hamt_amd.optim import RangerLars, build_optimizer
    model = _Tiny()
    opts = types.SimpleNamespace(optim="rangerlars", learning_rate=5e-5, betas=(0.9, 0.98), weight_decay=0.01)
    opt = build_optimizer(model, opts)
    assert isinstance(opt, RangerLars)
    names = {id(p): n for n, p in model.named_parameters()}
    g0, g1 = opt.param_groups
    assert sorted(names[id(p)] for p in g0["params"]) == ["dense.weight", "emb.weight", "layer_norm.weight"]
    assert sorted(names[id(p)] for p in g1["params"]) == ["LayerNorm.bias", "LayerNorm.weight", "dense.bias", "layer_norm.bias"]
    assert g0["weight_decay"] == 0.01 and g1["weight_decay"] == 0.0
    for g in opt.param_groups:
        assert g["lr"] == 5e-5 and g["betas"] == (0.9, 0.98) and g["eps"] == 1e-8
        assert g["lookahead_alpha"] == 0.5 and g["lookahead_k"] == 6 and g["lookahead_step"] == 0
    with pytest.raises(ValueError):
        build_optimizer(model, types.SimpleNamespace(optim="adam", learning_rate=1e-4, betas=(0.9, 0.98), weight_decay=0.01))


def test_rangerlars_signature_and_ralamb():
    from vln_hamt_amd.optim import Ralamb, RangerLars
    ps = [torch.nn.Parameter(torch.zeros(4))]
    r = RangerLars(ps, 0.25, 3, 1e-3, (0.8, 0.99))          # RangerLars(params, alpha, k, *args) -> Ralamb(params, lr, betas)
    g = r.param_groups[0]
    assert (g["lookahead_alpha"], g["lookahead_k"], g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (0.25, 3, 1e-3, (0.8, 0.99), 1e-8, 0)
    assert "lookahead_step" not in Ralamb(ps).param_groups[0]
    with pytest.raises(ValueError):
        RangerLars(ps, alpha=1.5)
    with pytest.raises(ValueError):
        RangerLars(ps, k=0)


@pytest.mark.parametrize("betas", [(0.9, 0.98), (0.9, 0.999)])
def test_host_coefficients_match_the_reference_formulas(betas):
    """ralamb.py:57-68, restated: the branch flag (N_sma >= 5) and s*lr, t = 1 ... 50"""
    from vln_hamt_amd.optim.rangerlars import ralamb_coef
    b1, b2 = betas
    lr = 3e-4
    for t in range(1, 51):
        rho_inf = 2.0 / (1.0 - b2) - 1.0
        rho = rho_inf - 2.0 * t * b2 ** t / (1.0 - b2 ** t)
        rect, s = ralamb_coef(t, b1, b2)
        assert rect == (rho >= 5), t
        if rho >= 5:
            want = math.sqrt((1 - b2 ** t) * (rho - 4) / (rho_inf - 4) * (rho - 2) / rho * rho_inf / (rho_inf - 2)) / (1 - b1 ** t)
        else:
            want = 1.0 / (1 - b1 ** t)
        assert abs(s * lr - want * lr) <= 1e-15 * want * lr, (t, s, want)
    if betas == (0.9, 0.98):          # steps 1-5 take the un-rectified branch, step 6 onward the rectified one
        assert [ralamb_coef(t, b1, b2)[0] for t in range(1, 8)] == [False] * 5 + [True] * 2


def test_item_table_layout():
    """include/hamt.h hamt_ralamb_table: items inside one parameter each, at most 1024 float4, in arena order"""
    from vln_hamt_amd.optim.rangerlars import ITEM4, item_table
    ends = np.array([8, 8, 4096, 4104, 4104 + 3 * 4096 + 8, 20000 + 8 * 1024 * 4 + 512])
    n = int(ends[-1])
    tab, nitems = item_table(ends, n)
    assert tab.dtype == np.int32 and tab.size == 2 * nitems + len(ends) + 2
    starts, param, first = tab[:nitems + 1], tab[nitems + 1:2 * nitems + 1], tab[2 * nitems + 1:]
    assert starts[0] == 0 and starts[-1] == n // 4 and (np.diff(starts) > 0).all() and (np.diff(starts) <= ITEM4).all()
    assert first[0] == 0 and first[-1] == nitems and (np.diff(param) >= 0).all()
    b4 = np.concatenate([[0], ends[:-1]]) // 4
    for q in range(len(ends)):
        its = np.arange(first[q], first[q + 1])
        assert (param[its] == q).all()
        if its.size:
            assert starts[its[0]] == b4[q] and starts[its[-1] + 1] == ends[q] // 4
        else:
            assert ends[q] == b4[q] * 4            # (an empty parameter has no item)


@pytest.mark.skipif(not os.path.isdir(os.environ.get("HAMT_REFERENCE", "/root/reference")),
                    reason="needs the reference's source tree (HAMT_REFERENCE), which the repository does not hold")
def test_committed_rangerlars_golden_matches_its_generator():
    """tools/gen_rangerlars_golden.py re-run against the reference reproduces tests/golden/rangerlars_tiny.npz key for key, bit for bit"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_rangerlars_golden", os.path.join(ROOT, "tools", "gen_rangerlars_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = gen.generate()
    old = load_npz("rangerlars_tiny.npz")
    assert set(new) == set(old), sorted(set(new) ^ set(old))[:10]
    for k in new:
        a = np.asarray(new[k])
        assert a.dtype == old[k].dtype and np.array_equal(a, old[k], equal_nan=a.dtype.kind == "f"), k


def test_rangerlars_kernels_do_not_spill(tmp_path):
    import test_kernel_resources as tkr
    if not (os.path.exists(tkr.READELF) and os.path.exists(tkr.OBJCOPY)):
        pytest.skip("ROCm LLVM tools not installed")
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = {}
    for co in tkr._code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([tkr.READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or "ralamb_" not in name.group(1):
                continue
            seen[name.group(1)] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                                   int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert sum(k in n for n in seen for k in ("ralamb_moments_kernel", "ralamb_trust_kernel", "ralamb_apply_kernel")) == 3, seen
    assert all(sp == 0 and scratch == 0 for sp, scratch in seen.values()), seen
