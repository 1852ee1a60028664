"""GPU: the device-side validation pass -- ops.eval_ce / eval_kl / eval_mse_cols (csrc/eval.hip) against the float64 restatements of
tests/_eval_ref.py, and vln_hamt_amd.validate against the reference's statements on the model's own outputs and against the
reference's own numbers (tests/golden/validate.npz).  Counts are exact; a loss sum is within the SUM of the per-row bounds of
tests/_smallops_ref.py (CE_LOSS_BOUND / KL_LOSS_BOUND row units), no new number."""
import numpy as np
import pytest
import torch

from _eval_ref import (FOLD_R, GOLDEN_TAGS, MSE_COLS_C, MSE_COLS_R, argmax_cases, eval_ce_f64, eval_kl_f64, eval_mse_cols_f64, fold_cases,
                       golden_batches, golden_f64, kl_argmax_case, mse_cols_case, split_finite)
from _smallops_ref import ce_cases, kl_cases
from _util import load_npz, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_ce(buf, C, label, layout="view", acc=None):
    """one ops.eval_ce call on the [:, :C] view of `buf` in the case's layout -> (sums, counts)"""
    from vln_hamt_amd import ops
    acc = acc or ops.EvalAccumulator(DEV)
    if layout == "empty_rows":
        x = ops.empty_rows(buf.shape[0], C, DEV)
        x.copy_(dev(buf[:, :C]))
    elif layout == "colstride":
        x = dev(buf[:, :C].T).t()
        if x.shape[0] > 1:                                         # (a single row has no column stride to speak of)
            assert x.stride(1) != 1
            with pytest.raises(ops.L.HamtError):
                ops.eval_ce(x, dev(label), acc)
        x = x.contiguous()                                         # as CrossEntropyFn does
    else:
        x = dev(buf)[:, :C]
    ops.eval_ce(x, dev(label), acc)
    return acc.read()


def check_ce(name, buf, C, label, layout="view"):
    (sums, counts) = run_ce(buf, C, label, layout)
    want, k, n, bound = eval_ce_f64(buf, C, label)
    print(f"[{name}] loss sum {sums[0]!r} float64 {want!r} |d| {abs(sums[0] - want):.3e} bound {bound:.3e}  correct {counts[0]}/{counts[1]}")
    assert counts[:2] == [k, n] and counts[2:] == [0, 0] and sums[1:] == [0.0, 0.0, 0.0], (name, counts, k, n, sums)
    assert abs(sums[0] - want) <= bound, (name, sums[0], want, bound)


# ---------------------------------------------------------------------------------------------- eval_ce
@pytest.mark.parametrize("i", range(len(ce_cases())), ids=[c["name"] for c in ce_cases()])
def test_eval_ce_loss_cases(i):
    """every case of _smallops_ref.ce_cases(): the rows with a finite (or ignored) loss in one call, the rows that must give inf / NaN
    in a call of their own, whose total has to be non-finite with the counts still exact"""
    c = ce_cases()[i]
    fin, bad = split_finite(c)
    check_ce(c["name"], c["buf"][fin], c["C"], c["label"][fin], c["layout"])
    if len(bad):
        sums, counts = run_ce(c["buf"][bad], c["C"], c["label"][bad], c["layout"])
        _, k, n, _ = eval_ce_f64(c["buf"][bad], c["C"], c["label"][bad])
        assert not np.isfinite(sums[0]) and counts[:2] == [k, n], (c["name"], sums, counts, k, n)


@pytest.mark.parametrize("i", range(len(argmax_cases())), ids=[c["name"] for c in argmax_cases()])
def test_eval_ce_argmax_cases(i):
    c = argmax_cases()[i]
    check_ce(c["name"], c["buf"], c["C"], c["label"])


@pytest.mark.parametrize("i", range(len(FOLD_R)), ids=[f"R{r}" for r in FOLD_R])
def test_eval_ce_row_counts(i):
    c = fold_cases()[i]
    check_ce(c["name"], c["buf"], c["C"], c["label"])


def test_eval_ce_bad_rows():
    """a label >= C gives NaN (no out-of-bounds read) and still counts; a NaN logit puts NaN into the sum and is never correct -- not
    even where the NaN sits on the label, which is where torch's max would point"""
    from vln_hamt_amd import ops
    x = np.random.Generator(np.random.PCG64(9)).standard_normal((3, 300)).astype(np.float32)
    sums, counts = run_ce(x, 300, np.array([300, -1, int(np.argmax(x[2]))], dtype=np.int64))
    assert np.isnan(sums[0]) and counts[:2] == [1, 2]
    x[0, 7] = np.nan
    x[1, 299] = np.nan
    sums, counts = run_ce(x, 300, np.array([7, int(np.nanargmax(x[1])), int(np.argmax(x[2]))], dtype=np.int64))
    assert np.isnan(sums[0]) and counts[:2] == [1, 3]
    acc = ops.EvalAccumulator(DEV)
    with pytest.raises(ops.L.HamtError):
        ops.eval_ce(dev(x).double(), dev(np.zeros(3, dtype=np.int64)), acc)
    with pytest.raises(ops.L.HamtError):
        ops.eval_ce(dev(x), dev(np.zeros(3, dtype=np.int32)), acc)
    with pytest.raises(ops.L.HamtError):
        ops.eval_ce(dev(x), dev(np.zeros(4, dtype=np.int64)), acc)
    with pytest.raises(ops.L.HamtError):
        ops.eval_mse_cols(dev(x)[:, :5], dev(x)[:, :5], acc)
    assert acc.read() == ([0.0] * 4, [0] * 4)


# ---------------------------------------------------------------------------------------------- eval_kl, eval_mse_cols
@pytest.mark.parametrize("i", range(len(kl_cases()) + 1), ids=[c["name"] for c in kl_cases()] + ["argmax"])
def test_eval_kl_cases(i):
    from vln_hamt_amd import ops
    c = kl_cases()[i] if i < len(kl_cases()) else kl_argmax_case()
    R, C = c["R"], c["C"]
    xb, tb = np.full((R, C + 5), 7.0, dtype=np.float32), np.full((R, C + 2), 0.5, dtype=np.float32)     # two different row strides
    xb[:, :C], tb[:, :C] = c["x"], c["t32"]
    acc = ops.eval_kl(dev(xb)[:, :C], dev(tb)[:, :C], ops.EvalAccumulator(DEV))
    sums, counts = acc.read()
    want, k, n, bound = eval_kl_f64(c["x"], c["t32"])
    print(f"[{c['name']}] loss sum {sums[0]!r} float64 {want!r} |d| {abs(sums[0] - want):.3e} bound {bound:.3e}  agree {counts[0]}/{counts[1]}")
    assert counts == [k, n, 0, 0] and abs(sums[0] - want) <= bound, (c["name"], sums, counts, want, k, n, bound)


@pytest.mark.parametrize("C", MSE_COLS_C)
def test_eval_mse_cols(C):
    """equal to the float64 sum of the fp32 terms to 1e-12 relative: the terms are exact, only the order of the fp64 fold differs"""
    from vln_hamt_amd import ops
    for R in MSE_COLS_R:
        c = mse_cols_case(R, C)
        acc = ops.eval_mse_cols(dev(c["xb"])[:, :C], dev(c["tb"])[:, :C], ops.EvalAccumulator(DEV))
        sums, counts = acc.read()
        want = eval_mse_cols_f64(c["x"], c["t"])
        print(f"[{c['name']}] {sums[:C]} float64 {want.tolist()}")
        assert counts == [0] * 4 and sums[C:] == [0.0] * (4 - C)
        assert all(abs(sums[j] - want[j]) <= 1e-12 * want[j] for j in range(C)), (c["name"], sums, want)


# ---------------------------------------------------------------------------------------------- accumulation, determinism, capture
def _three_updates(acc, poison=False):
    from vln_hamt_amd import ops
    total = np.zeros(4)
    for i in (4, 1, 2):                                            # R = 257, 1, 255
        c = fold_cases()[i]
        if poison:
            acc.workspace(4097).fill_(float("nan"))
        ops.eval_ce(dev(c["buf"])[:, :c["C"]], dev(c["label"]), acc)
        total += np.array(eval_ce_f64(c["buf"], c["C"], c["label"]))
    return total


def test_accumulates_and_repeats_bit_identically():
    from vln_hamt_amd import ops
    acc = ops.EvalAccumulator(DEV)
    want, k, n, bound = _three_updates(acc)
    sums, counts = acc.read()
    print(f"three updates: {sums[0]!r} float64 {want!r} |d| {abs(sums[0] - want):.3e} bound {bound:.3e}")
    assert counts[:2] == [int(k), int(n)] and abs(sums[0] - want) <= bound
    first = acc.buf.clone()
    for poison in (False, True):
        acc.zero_()
        assert acc.read() == ([0.0] * 4, [0] * 4)
        _three_updates(acc, poison)
        assert torch.equal(acc.buf, first), (poison, acc.read(), sums, counts)       # int64 view of the fp64 sums: bit for bit


def test_eval_ce_in_a_captured_graph():
    """one eval_ce call captured as a linear graph with the project's helpers: two replays add exactly twice the eager amount"""
    from vln_hamt_amd import ops, streams
    from vln_hamt_amd.graph import _finish_graph, _new_graph
    c = fold_cases()[4]
    x, lab = dev(c["buf"])[:, :c["C"]], dev(c["label"])
    acc = ops.EvalAccumulator(DEV)
    ops.eval_ce(x, lab, acc)
    eager_s, eager_c = acc.read()
    side = streams.role_stream(torch.cuda.current_device(), "capture")
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        ops.eval_ce(x, lab, acc)                                   # warm-up on the capture stream
    cur.wait_stream(side)
    torch.cuda.synchronize()
    acc.zero_()
    torch.cuda.synchronize()
    g = _new_graph()
    with torch.cuda.graph(g, stream=side):
        ops.eval_ce(x, lab, acc)
    g = _finish_graph(g)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    sums, counts = acc.read()
    assert sums[0] == 2 * eager_s[0] and counts[:2] == [2 * eager_c[0], 2 * eager_c[1]], (sums, counts, eager_s, eager_c)


def test_no_sync_inside_the_loop():
    from vln_hamt_amd import ops
    c, k, m = fold_cases()[3], kl_cases()[2], mse_cols_case(255, 3)
    x, lab = dev(c["buf"])[:, :c["C"]], dev(c["label"])
    kx, kt, mx, mt = dev(k["x"]), dev(k["t32"]), dev(m["x"]), dev(m["t"])
    idx = dev(np.flatnonzero(c["label"] >= 0).astype(np.int64))
    acc = ops.EvalAccumulator(DEV)
    ops.eval_ce(x, lab, acc)                                       # (the workspace is sized outside the guarded region as well as inside)
    acc.zero_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            lab[0].item()
            raised = False
        except RuntimeError:
            raised = True
        if raised:
            ops.eval_ce(x.index_select(0, idx), lab.index_select(0, idx), acc)       # labels by index list, as validate_mlm takes them
            ops.eval_kl(kx, kt, acc)
            ops.eval_mse_cols(mx, mt, acc)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build")
    sums, counts = acc.read()
    assert counts[1] == len(idx) + k["R"]


# ---------------------------------------------------------------------------------------------- validate_* on the model and on the golden
class Recording:
    """the model, with every compute_loss=False output kept: the reference's statements are then restated on the SAME scores"""

    def __init__(self, model):
        self.model, self.outputs = model, []

    def __call__(self, batch, task, compute_loss=True):
        out = self.model(batch, task=task, compute_loss=compute_loss)
        self.outputs.append(out)
        return out

    def eval(self):
        self.model.eval()

    def train(self):
        self.model.train()


def _f64(t):
    return t.detach().cpu().double().numpy()


def reference_statements(task, outputs, batches):
    """main_r2r.py:344-511 on recorded outputs, in float64 -> (returned dict without the throughput key, summed bound per loss key)"""
    if task in ("mlm", "sap", "itm"):
        tot = k = n = bound = 0
        for out, b in zip(outputs, batches):
            if task == "mlm":
                scores, labels = out, b["txt_labels"][b["txt_labels"] != -1]
            elif task == "sap":
                scores, labels = out, b["ob_action_viewindex"]
            else:
                scores, labels = out
            x = scores.detach().float().cpu().numpy()
            s, kk, nn, bd = eval_ce_f64(x, x.shape[1], labels.cpu().numpy())
            tot, k, n, bound = tot + s, k + kk, n + nn, bound + bd
        return {"loss": tot / n, "acc": k / n}, {"loss": bound / n}
    if task == "mrc":
        tot = k = n = bound = 0
        for (pred, tgt), b in zip(outputs, batches):
            s, kk, _, bd = eval_kl_f64(pred.detach().float().cpu().numpy(), tgt.detach().float().cpu().numpy())
            tot, k, n, bound = tot + s, k + kk, n + int(b["hist_mrc_masks"].sum().item()), bound + bd
        return {"loss": tot / n, "acc": k / n}, {"loss": bound / n}
    keys = ("heading_loss", "elevation_loss", "progress_loss")[:3 if task == "sar" else 2]
    sums, n = np.zeros(len(keys)), 0
    for out, b in zip(outputs, batches):
        scores = out.detach().float().cpu()
        tg = [b["ob_action_angles"][:, 0], b["ob_action_angles"][:, 1], b["ob_progress"]] if task == "sar" else [b["sp_targets"][:, 0], b["sp_targets"][:, 1]]
        for j in range(len(keys)):                                 # F.mse_loss(scores[:, j], target_j, reduction='sum')
            d = (scores[:, j] - tg[j].float().cpu()).numpy()       # fp32 difference and square, as the kernel takes them
            sums[j] += float((d * d).astype(np.float64).sum())
        n += scores.size(0)
    return {k: sums[j] / n for j, k in enumerate(keys)}, {k: 1e-12 * sums[j] / n for j, k in enumerate(keys)}


@pytest.fixture(scope="module")
def tiny_sd():
    from oracle.hamt_oracle import make_state_dict, pretrain_param_shapes
    cfg = tiny_cfg()
    return cfg, make_state_dict(pretrain_param_shapes(cfg), seed=3)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_validate_end_to_end(tiny_sd, prec):
    """tiny config, the six tasks, two synth batches each: validate_* equals the reference's statements in float64 on the model's OWN
    compute_loss=False outputs of the same batches (so the precision mode does not enter the tolerance); `validate` leaves the model in
    training mode and returns the prefixed keys"""
    from test_gpu_model import build, to_dev
    from vln_hamt_amd import validate as V
    from vln_hamt_amd.synth import TASKS, make_batch, make_itm_rng
    cfg, sd = tiny_sd
    model = build(cfg, sd, prec, train=True)
    rec = Recording(model)
    loaders = {}
    for i, task in enumerate(TASKS):
        bs = []
        for j in range(2):
            b = make_batch(task, 4 + 2 * j, cfg, seed=50 + 10 * i + j, txt_len=20 + 4 * j, hist_len=4, ragged=bool(j))
            if task == "itm":
                r = make_itm_rng(b, seed=7 + j)
                b["itm_neg_idxs"], b["itm_shuffled_pos_ids"] = r["neg_idxs"], r["shuffled_pos_ids"]
            bs.append(to_dev(b))
        loaders[task] = bs
    logged = []
    out = V.validate(rec, loaders, setname="_seen", log_fn=logged.append)
    assert model.training and len(logged) == 6 and len(rec.outputs) == 12
    pos = 0
    for task in loaders:
        want, bound = reference_statements(task, rec.outputs[pos:pos + 2], loaders[task])
        pos += 2
        thr = "feat_per_s" if task == "mrc" else "tok_per_s"
        assert {k for k in out if k.startswith(f"val_seen_{task}_")} == {f"val_seen_{task}_{k}" for k in list(want) + [thr]}, task
        assert out[f"val_seen_{task}_{thr}"] > 0
        for k, v in want.items():
            got = out[f"val_seen_{task}_{k}"]
            print(f"[{prec} {task}] {k}: {got!r} float64 {v!r} |d| {abs(got - v):.3e} bound {bound.get(k, 0.0):.3e}")
            assert (got == v) if k == "acc" else (abs(got - v) <= bound[k]), (task, k, got, v, bound.get(k))


class Scripted:
    def __init__(self, tag, batches):
        self.tag, self.batches, self.i = tag, batches, 0

    def __call__(self, batch, task, compute_loss=True):
        assert compute_loss is False
        b = self.batches[batch["i"]]
        if self.tag == "itm":
            return dev(b["scores"]), dev(b["labels"])
        if self.tag == "mrc":
            return dev(b["scores"]), dev(b["targets"])
        return dev(b["scores"])


@pytest.mark.parametrize("tag", sorted(GOLDEN_TAGS))
def test_validate_on_the_reference_golden(tag):
    """validate.npz through validate_* with a stand-in model on the device, against the REFERENCE's returned numbers: accuracies exact,
    losses within the summed bound plus the reference's own distance from float64 (tests/test_eval_ref.py prints and bounds it)"""
    from vln_hamt_amd import validate as V
    store = load_npz("validate.npz")
    bs = golden_batches(store, tag)
    fn = {"mlm": V.validate_mlm, "sap": V.validate_sap, "sapnan": V.validate_sap, "itm": V.validate_itm, "mrc": V.validate_mrc,
          "sar": V.validate_sar, "sprel": V.validate_sprel, "sprel3d": V.validate_sprel}[tag]
    loader = [dict({k: dev(v) for k, v in b.items() if k not in ("scores", "labels", "targets")}, i=i) for i, b in enumerate(bs)]
    got = fn(Scripted(tag, bs), loader)
    f64, exact, bound, slack = golden_f64(store, tag)
    want = {k.split("/")[-1]: float(v) for k, v in store.items() if k.startswith(f"{tag}/want/")}
    assert set(got) == set(want) | {"feat_per_s" if tag == "mrc" else "tok_per_s"}
    for k, w in want.items():
        print(f"[{tag}] {k}: {got[k]!r} reference {w!r} float64 {f64[k]!r}")
        if k in exact:
            assert got[k] == w, (tag, k, got[k], w)
        elif not np.isfinite(w):
            assert not np.isfinite(got[k]), (tag, k, got[k], w)
        else:
            assert abs(got[k] - f64[k]) <= bound[k] and abs(got[k] - w) <= bound[k] + slack[k], (tag, k, got[k], w, f64[k], bound[k], slack[k])
    if tag == "mrc":                                               # compute_accuracy_for_soft_targets, the reference's helper
        assert V.compute_accuracy_for_soft_targets(dev(bs[0]["scores"]), dev(bs[0]["targets"])) == eval_kl_f64(bs[0]["scores"], bs[0]["targets"])[1]
