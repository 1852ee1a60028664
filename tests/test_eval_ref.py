"""Not gpu: the validation pass (vln_hamt_amd/validate.py, ops.eval_ce / eval_kl / eval_mse_cols, csrc/eval.hip) -- the float64
restatement the GPU tests compare against reproduces the REFERENCE's own validate_* functions (tests/golden/validate.npz,
tools/gen_validate_golden.py), the cases can tell the likely mistakes from the right kernel, the host side (totals across ranks,
dispatch, key names, mode handling) is right, the entry points are declared and bound, and the cross-compiled kernels use no scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

from _eval_ref import (GOLDEN_TAGS, argmax_cases, argmax_rows, eval_ce_f64, eval_kl_f64, eval_mse_cols_f64, fold_cases, golden_batches,
                       golden_f64, kl_argmax_case, mse_cols_case, split_finite, top_two_gap_ok)
from _smallops_ref import ce_cases, kl_cases
from _util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hamt_eval_ce", "hamt_eval_kl", "hamt_eval_mse_cols")


def _entry_points():
    from vln_hamt_amd import _lib, ops, validate                   # (the feature under test: absent on the parent commit)
    assert callable(ops.eval_ce) and callable(ops.eval_kl) and callable(ops.eval_mse_cols) and callable(validate.validate)
    return [_lib.SIGNATURES[n] for n in NAMES]


# ---------------------------------------------------------------------------------------------- the golden
@pytest.mark.parametrize("tag", sorted(GOLDEN_TAGS))
def test_restatement_reproduces_the_reference(tag):
    """tests/_eval_ref.py against the reference's validate_* on the scripted outputs: accuracies (and so the counts) exact, losses
    within what the reference's own fp32 arithmetic can differ from float64 by (printed: the GPU golden test adds it to its bound)"""
    _entry_points()
    store = load_npz("validate.npz")
    got, exact, _, slack = golden_f64(store, tag)
    for k, v in got.items():
        key = f"{tag}/want/{k}"
        if key not in store:
            continue
        want = float(store[key])
        if k in exact:
            assert v == want, (tag, k, v, want)
        elif not np.isfinite(want):
            assert not np.isfinite(v), (tag, k, v, want)
        else:
            print(f"[{tag}] {k}: reference {want!r}  float64 {v!r}  distance {abs(v - want):.3e}  allowed {slack[k]:.3e}")
            assert abs(v - want) <= slack[k], (tag, k, v, want, slack[k])
    assert got["n"] > 0


def test_golden_covers_what_it_should():
    _entry_points()
    store = load_npz("validate.npz")
    for tag in GOLDEN_TAGS:
        bs = golden_batches(store, tag)
        rows = [len(b["scores"]) for b in bs]
        assert len(bs) == 3 or tag == "sapnan"
        assert tag == "sapnan" or (0 in rows and len(set(rows)) == 3), (tag, rows)
    mlm = golden_batches(store, "mlm")
    assert mlm[0]["scores"].shape[1] == 30522 and "mlm/0/scores" not in store             # regenerated from the seed, not stored
    lab = mlm[0]["txt_labels"][mlm[0]["txt_labels"] != -1]
    hit = argmax_rows(mlm[0]["scores"]) == lab
    assert hit.any() and not hit.all()
    sap = golden_batches(store, "sap")[0]
    x, lab = sap["scores"], sap["ob_action_viewindex"]
    assert x.shape[1] == 37 and np.isinf(x).any()
    ties = [r for r in range(len(x)) if (x[r] == x[r].max()).sum() == 2]
    assert ties and all(lab[r] == np.flatnonzero(x[r] == x[r].max())[0] for r in ties)     # the label is the LOWER column of the tie
    assert eval_ce_f64(x, 37, lab)[1] == eval_ce_f64(x, 37, lab, highest=True)[1] + len(ties)
    nan = golden_batches(store, "sapnan")[0]
    assert np.isinf(nan["scores"]).all(axis=1).any() and np.isinf(nan["scores"][np.arange(4), nan["ob_action_viewindex"]]).any()
    assert float(store["sapnan/want/acc"]) == 0.75 and not np.isfinite(float(store["sapnan/want/loss"]))
    assert golden_batches(store, "itm")[0]["scores"].shape[1] == 5
    mrc = golden_batches(store, "mrc")
    t = mrc[0]["targets"]
    assert t.shape[1] == 1000 and (t == 0).all(axis=1).any() and ((t == 1).sum(axis=1) == 1).any()
    for b in mrc:                                                                          # n_feat: the device's row count is the mask sum
        assert int(b["hist_mrc_masks"].sum()) == len(b["scores"])
    assert golden_f64(store, "mrc")[0]["n"] == sum(int(b["hist_mrc_masks"].sum()) for b in mrc)
    for tag in ("sar", "sprel"):
        col = np.abs(np.concatenate([b["scores"][:, 0] for b in golden_batches(store, tag)]))
        assert (col < 1e-2).any() and (col > 1e2).any()
    for tag in ("mlm", "sap", "itm", "mrc"):
        assert all(top_two_gap_ok(b["scores"]) for b in golden_batches(store, tag))


# ---------------------------------------------------------------------------------------------- the cases catch the mistakes
def _ce_inputs():
    out = [(c["name"], c["buf"], c["C"], c["label"]) for c in argmax_cases() + fold_cases()]
    for c in ce_cases():
        if c["layout"] == "colstride":
            continue
        fin, _ = split_finite(c)
        out.append((c["name"], c["buf"][fin], c["C"], c["label"][fin]))
    return out


@pytest.mark.parametrize("mistake", ["highest", "drop_tail", "count_ignored", "add_ignored", "stride_is_C"])
def test_ce_cases_catch(mistake):
    """every mistake changes a count, or moves a loss sum by more than the summed bound, on at least one case"""
    _entry_points()
    caught = []
    for name, buf, C, label in _ce_inputs():
        s, k, n, bound = eval_ce_f64(buf, C, label)
        s2, k2, n2, _ = eval_ce_f64(buf, C, label, **{mistake: True})
        if k2 != k or n2 != n or not abs(s2 - s) <= bound:
            caught.append(name)
    print(mistake, "caught by", caught)
    assert caught, mistake


def test_argmax_cases_are_what_they_say():
    _entry_points()
    for c in argmax_cases():
        x = c["buf"][:, :c["C"]]
        a = argmax_rows(x)
        for r, (cols, lab) in enumerate(c["peaks"]):
            if cols:
                assert a[r] == min(cols) and all(x[r, col] == x[r].max() for col in cols), (c["name"], r)
        if c["C"] > 261:
            assert any(len(cols) == 2 and cols[1] - cols[0] == 256 for cols, _ in c["peaks"])
    assert [c["R"] for c in fold_cases()] == [0, 1, 255, 256, 257, 4097]
    assert all((c["label"] < 0).any() for c in fold_cases() if c["R"] > 3)


def test_kl_and_mse_cases_catch():
    _entry_points()
    c = kl_argmax_case()
    s, k, n, bound = eval_kl_f64(c["x"], c["t"])
    assert (k, n) == (4, 8), (k, n)                                 # rows 0, 2, 4, 6 agree
    assert eval_kl_f64(c["x"], c["t"], target_from_pred=True)[1] == 8
    for kc in kl_cases():
        assert np.isfinite(eval_kl_f64(kc["x"], kc["t32"])[0])
    for C in (2, 3, 4):
        m = mse_cols_case(257, C)
        right, wrong = eval_mse_cols_f64(m["x"], m["t"]), eval_mse_cols_f64(m["x"], m["t"], swap=True)
        assert abs(wrong[0] - right[0]) > 1e-12 * right[0] and right[0] > 1e3 * right[1]


# ---------------------------------------------------------------------------------------------- the host side
def test_combine_totals_sums_in_rank_order():
    _entry_points()
    from vln_hamt_amd.validate import combine_totals
    ranks = [([1e16, 0.5, 0.0, 0.0], [3, 10, 0, 0, 7]), ([1.0, 0.25, 0.0, 0.0], [4, 11, 0, 0, 8]), ([-1e16, 0.125, 0.0, 0.0], [5, 12, 0, 0, 9])]
    sums, counts = combine_totals(ranks)
    assert sums == [((0.0 + 1e16) + 1.0) + -1e16, 0.875, 0.0, 0.0] and sums[0] == 0.0      # (rank order: 1.0 is absorbed by 1e16)
    assert counts == [12, 33, 0, 0, 24] and all(type(c) is int for c in counts)
    assert combine_totals([ranks[0], ranks[2], ranks[1]])[0][0] == 1.0                                         # another order gives another sum
    assert combine_totals(ranks[:1]) == (ranks[0][0], ranks[0][1])
    with pytest.raises(ValueError):
        combine_totals([])
    with pytest.raises(ValueError):
        combine_totals([([1.0], [1]), ([1.0, 2.0], [1])])


class _Model:
    def __init__(self):
        self.calls = []

    def eval(self):
        self.calls.append("eval")

    def train(self):
        self.calls.append("train")


def test_validate_dispatches_and_renames(monkeypatch):
    _entry_points()
    from vln_hamt_amd import validate as V
    seen = []

    def fake(prefix):
        def fn(model, loader):
            seen.append((prefix, loader, list(model.calls)))
            return {"loss": len(seen), "acc": 0.5}
        return fn
    monkeypatch.setattr(V, "_VALIDATORS", tuple((p, fake(p)) for p, _ in V._VALIDATORS))
    assert [p for p, _ in V._VALIDATORS] == ["mlm", "sap", "sar", "sprel", "mrc", "itm"]
    model, logged = _Model(), []
    loaders = {"mlm": "L0", "sap_r2r": "L1", "sar": "L2", "sprel": "L3", "mrc_x": "L4", "itm": "L5"}
    out = V.validate(model, loaders, setname="_unseen", log_fn=logged.append)
    assert [(p, l) for p, l, _ in seen] == [("mlm", "L0"), ("sap", "L1"), ("sar", "L2"), ("sprel", "L3"), ("mrc", "L4"), ("itm", "L5")]
    assert all(calls == ["eval"] for _, _, calls in seen) and model.calls == ["eval", "train"]
    assert out["val_unseen_sap_r2r_loss"] == 2 and out["val_unseen_mrc_x_acc"] == 0.5 and len(out) == 12
    assert logged[1] == {"valid_unseen_sap_r2r/val_unseen_sap_r2r_loss": 2, "valid_unseen_sap_r2r/val_unseen_sap_r2r_acc": 0.5} and len(logged) == 6
    assert set(V.validate(model, {"itm": "L"})) == {"val_itm_loss", "val_itm_acc"}
    with pytest.raises(ValueError, match="Undefined task nsp"):
        V.validate(model, {"nsp": "L"})
    import inspect
    for name in ("validate_mlm", "validate_sap", "validate_sar", "validate_sprel", "validate_mrc", "validate_itm"):
        assert list(inspect.signature(getattr(V, name)).parameters) == ["model", "val_loader"], name
    assert list(inspect.signature(V.validate).parameters) == ["model", "val_dataloaders", "setname", "log_fn"]
    assert callable(V.compute_accuracy_for_soft_targets)


def test_eval_ops_fail_loudly_without_gpu():
    import torch
    from vln_hamt_amd import ops
    from vln_hamt_amd._lib import HamtError
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(HamtError):
        ops.EvalAccumulator("cpu")
    with pytest.raises(HamtError):
        ops.eval_ce(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), None)


# ---------------------------------------------------------------------------------------------- ABI and code object
def test_symbols_in_header_and_binding():
    sigs = _entry_points()
    src = open(os.path.join(ROOT, "include", "hamt.h")).read()
    for name, sig in zip(NAMES, sigs):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(sig), name
    from vln_hamt_amd import _lib, ops
    assert '"eval.hip"' in open(os.path.join(ROOT, "vln_hamt_amd", "csrc", "build.py")).read()
    assert ops.EVAL_SLOTS == 4
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES) and lib.hamt_version() == 2


def test_eval_kernels_use_no_scratch(tmp_path):
    """The cross-compiled gfx950 code object of eval.hip: no scratch memory, no spilled registers, and no more LDS than the few
    words that pass partial results between the four waves (read as tests/test_nav_graph.py does)."""
    from test_kernel_resources import OBJCOPY, READELF, _code_objects
    from vln_hamt_amd import _lib
    _entry_points()
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
            if not name or not re.search(r"eval_(ce_rows|kl_rows|fold|mse_cols)_kernel", name.group(1)):
                continue
            num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
            seen.append(name.group(1))
            print(name.group(1), "vgprs", num("vgpr_count"), "sgprs", num("sgpr_count"), "lds", num("group_segment_fixed_size"))
            assert num("vgpr_spill_count") == 0 and num("sgpr_spill_count") == 0 and num("private_segment_fixed_size") == 0, (name.group(1), blk)
            assert num("group_segment_fixed_size") <= 256 and num("vgpr_count") <= 64, name.group(1)
    assert len(seen) == 7 and all(any(k in s for s in seen) for k in ("ce_rows", "kl_rows", "fold", "mse_cols")), seen
