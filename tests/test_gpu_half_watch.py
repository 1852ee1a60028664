"""-m gpu: audit.HalfRangeWatch on the tiny bf16 model (tests/_util.tiny_cfg, built as tests/test_gpu_model.py builds its tiny models):
the watch changes nothing it watches, counts what it should, names a doctored layer, and promotion removes the clamp."""
import functools
import warnings

import pytest
import torch

from _util import batch_from, load_npz, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
HALF_MAX = 65504.0
TASK = "sap"
# the doctored layer: the attention output projection of the first text layer (its input is the oracle's, layer for layer)
SITE = "bert.encoder.layer.0.attention.output.dense"
DOCTORED = SITE + ".weight"
FRAC_LO, FRAC_HI = 0.01, 0.50        # the share of the doctored layer's output that must lie beyond half's range
FRAC_PICK = 0.05                    # the power is the smallest that puts at least this share there (well inside the bounds)


@functools.lru_cache(maxsize=1)
def _tiny():
    from oracle.hamt_oracle import make_state_dict, pretrain_param_shapes
    store = load_npz("tiny_pretrain.npz")
    cfg = tiny_cfg()
    sd = make_state_dict(pretrain_param_shapes(cfg), seed=int(store["meta/sd_seed"]))
    cpu_batch, _ = batch_from(store, TASK)
    return cfg, sd, cpu_batch


def _build(sd=None):
    from vln_hamt_amd.model.pretrain_cmt import MultiStepNavCMTPreTraining
    from vln_hamt_amd.modeling import HamtConfig
    cfg, sd0, _ = _tiny()
    kw = dict(vars(cfg))
    kw["pretrain_tasks"] = set(cfg.pretrain_tasks)
    m = MultiStepNavCMTPreTraining(HamtConfig(hamt_precision="bf16", **kw))
    m.load_state_dict(sd0 if sd is None else sd, strict=True)
    return m.to(DEV).eval()


def _batch():
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in _tiny()[2].items()}


def _fwd_bwd(model, batch):
    """(loss, {name: grad}) of one training-style pass"""
    for p in model.parameters():
        p.grad = None
    loss = model(batch, TASK, True)
    loss.mean().backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _same(a, b):
    la, ga = a
    lb, gb = b
    assert torch.equal(la, lb), (la, lb)
    assert set(ga) == set(gb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def _site_runs(model, batch):
    """{parameter name: forward executions of the dense layer with that weight} for one no-grad forward, counted WITHOUT the watch: each
    of the three block functions asks ops.weight_operand for its weights once per forward, the weight of its audited layer included"""
    from vln_hamt_amd import blocks
    names = {id(p): n for n, p in model.named_parameters()}
    seen = {}
    orig = blocks.weight_operand

    def spy(w, prec):
        seen[names.get(id(w), "?")] = seen.get(names.get(id(w), "?"), 0) + 1
        return orig(w, prec)

    blocks.weight_operand = spy
    try:
        with torch.no_grad():
            model(batch, TASK, True)
    finally:
        blocks.weight_operand = orig
    return seen


def _is_site(name):
    """the audited layers by name: an attention block's `output.dense` / a feed-forward block's second layer (`*output.dense`)"""
    return name.endswith("output.dense.weight")


def test_watch_on_equals_watch_off_and_counts():
    from vln_hamt_amd import HalfRangeWatch
    model, batch = _build(), _batch()
    off = _fwd_bwd(model, batch)
    runs = _site_runs(model, batch)
    watch = HalfRangeWatch(model)
    with watch:
        on = _fwd_bwd(model, batch)
    assert not watch.enabled
    _same(on, off)
    rows = watch.report()
    sites = {r.name for r in rows}
    assert rows and all(_is_site(n) for n in sites), sites
    assert sites == {n for n in runs if _is_site(n)}, sites ^ {n for n in runs if _is_site(n)}
    for r in rows:
        print(f"[half watch] {r.name}: at_limit {r.at_limit} nonfinite {r.nonfinite} max_abs {r.max_abs:.4g} calls {r.calls}")
        assert r.at_limit == 0 and r.nonfinite == 0 and 0.0 < r.max_abs < HALF_MAX, r
        assert r.calls == runs[r.name], (r, runs[r.name])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert watch.check() == []
    # a pass outside the `with` is not audited; reset() zeroes the records and keeps the rows
    _fwd_bwd(model, batch)
    assert watch.report() == rows
    assert all(r.calls == 0 and r.max_abs == 0.0 for r in watch.reset().report()) and len(watch.report()) == len(rows)


def _doctor_power():
    """(k, fraction): the smallest power of two 2^k by which DOCTORED is multiplied so that at least 5 % of that layer's fp32 output on
    the test batch, computed by the CPU oracle, lies beyond +-65504.  Scaling W by 2^k turns the output y = W c + b into 2^k (y - b) + b."""
    from oracle.hamt_oracle import HamtOracle
    cfg, sd, cpu_batch = _tiny()
    orc = HamtOracle(sd, cfg)
    outs, lin = [], orc._lin

    def spy(name, x):
        y = lin(name, x)
        if name == SITE:
            outs.append(y.detach())
        return y

    orc._lin = spy
    with torch.no_grad():
        orc.forward(cpu_batch, TASK, True)
    assert len(outs) == 1
    y, b = outs[0].double(), sd[SITE + ".bias"].double()
    for k in range(1, 60):
        frac = float((((y - b) * 2.0 ** k + b).abs() > HALF_MAX).double().mean())
        if frac >= FRAC_PICK:
            return k, frac
    raise AssertionError("no power found")


@functools.lru_cache(maxsize=1)
def _doctored_sd():
    k, frac = _doctor_power()
    sd = dict(_tiny()[1])
    sd[DOCTORED] = sd[DOCTORED] * 2.0 ** k          # a power of two: exact in fp32 and in the bf16 image of the weight
    return k, frac, sd


def test_doctored_site_is_named_then_promoted():
    """bert.encoder.layer.0.attention.output.dense.weight x 2^POWER: the oracle's fp32 output of that layer on the tiny SAP batch then has
    FRACTION of its elements beyond +-65504 (POWER and FRACTION are printed by the test and recorded here: see below), inside the
    issue's 1 % .. 50 %.  check() names exactly that parameter, once; promoted, the layer reports no element at the limit and a largest
    magnitude above 65504.

    Recorded: POWER = 21, FRACTION = 0.2423 (1.30 % at 2^20, 57.97 % at 2^22; the undoctored output peaks at 0.094)."""
    from vln_hamt_amd import HalfRangeWarning, HalfRangeWatch
    k, frac, sd = _doctored_sd()
    print(f"[half watch] doctored {DOCTORED} by 2^{k}: {100 * frac:.2f} % of its fp32 output beyond {HALF_MAX:.0f}")
    assert FRAC_LO <= frac <= FRAC_HI, (k, frac)
    model, batch = _build(sd), _batch()
    watch = HalfRangeWatch(model)
    with watch, torch.no_grad():
        model(batch, TASK, True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert watch.check() == [DOCTORED]
        assert watch.check() == [DOCTORED]                   # named again, warned about once
    mine = [w for w in caught if issubclass(w.category, HalfRangeWarning)]
    assert len(mine) == 1 and DOCTORED in str(mine[0].message), [str(w.message) for w in caught]
    row = {r.name: r for r in watch.report()}[DOCTORED]
    n_out = batch["txt_ids"].numel() * sd[DOCTORED].shape[0]
    print(f"[half watch] {row}: {row.at_limit / n_out:.4f} of {n_out} elements at the limit")
    assert row.max_abs == HALF_MAX and row.nonfinite == 0 and 0 < row.at_limit <= n_out * row.calls

    assert watch.promote([DOCTORED]) == [DOCTORED]
    watch.reset()
    with watch, torch.no_grad():
        model(batch, TASK, True)
    rows = watch.report()
    assert all(r.at_limit == 0 and r.nonfinite == 0 for r in rows), [r for r in rows if r.at_limit or r.nonfinite]
    assert {r.name: r for r in rows}[DOCTORED].max_abs > HALF_MAX
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert watch.check() == []
    with pytest.raises(Exception):
        watch.promote(["no.such.layer"])


def test_promote_every_site_equals_fp32_dense_outputs(monkeypatch):
    from vln_hamt_amd import HalfRangeWatch, blocks
    batch = _batch()
    model = _build()
    watch = HalfRangeWatch(model)
    with watch, torch.no_grad():
        model(batch, TASK, True)
    names = [r.name for r in watch.report()]
    watch.promote(names)
    promoted = _fwd_bwd(model, batch)                       # no watch enabled: promotion does not need one

    ref_model = _build()
    monkeypatch.setattr(blocks, "O_DTYPE", torch.float32)
    want = _fwd_bwd(ref_model, batch)
    monkeypatch.undo()
    _same(promoted, want)
    half = _fwd_bwd(ref_model, batch)                       # ... and the comparison can tell: half outputs give another loss
    assert not torch.equal(half[0], want[0])
    watch.promote(names, on=False)
    _same(_fwd_bwd(model, batch), half)


def _trunk_args(batch):
    g = batch.get
    return (g("txt_ids"), g("txt_masks"), g("hist_img_fts"), g("hist_ang_fts"), g("hist_pano_img_fts"), g("hist_pano_ang_fts"), g("hist_masks"),
            g("ob_img_fts"), g("ob_ang_fts"), g("ob_nav_types"), g("ob_masks"))


def test_captured_graph_audits_on_every_replay():
    """graph.GraphedInference runs its callable once eagerly (the warm-up in front of the capture: audited like any pass), captures it
    (launches recorded, not run) and replays the graph on every call, the capturing one included: k calls = (1 + k) x the per-pass calls."""
    from vln_hamt_amd import HalfRangeWatch
    from vln_hamt_amd.graph import GraphedInference
    model, batch = _build(), _batch()
    args = _trunk_args(batch)
    assert all(torch.is_tensor(a) for a in args)
    watch = HalfRangeWatch(model)
    with watch, torch.no_grad():
        eager = [t.clone() for t in model.bert(*args)]
    per_pass = {r.name: r.calls for r in watch.report()}
    assert per_pass and all(c > 0 for c in per_pass.values())
    watch.reset()

    k = 3
    gi = GraphedInference(lambda *a: model.bert(*a))
    with watch:
        for _ in range(k):
            out = gi("trunk", *args)
    for e, o in zip(eager, out):
        assert torch.equal(e, o)
    got = {r.name: r for r in watch.report()}
    assert {n: r.calls for n, r in got.items()} == {n: (1 + k) * c for n, c in per_pass.items()}
    assert all(r.at_limit == 0 and r.nonfinite == 0 and 0 < r.max_abs < HALF_MAX for r in got.values())
    # the graph audits whether the watch is still enabled or not: the launches are in it
    out = gi("trunk", *args)
    assert {r.name: r.calls for r in watch.report()} == {n: (2 + k) * c for n, c in per_pass.items()}

    # captured with the watch disabled: never audits, enabled later or not
    watch.reset()
    gi_off = GraphedInference(lambda *a: model.bert(*a))
    gi_off("trunk", *args)
    with watch:
        gi_off("trunk", *args)
    assert all(r.calls == 0 and r.max_abs == 0.0 and r.at_limit == 0 for r in watch.report())


def test_table_capacity():
    from vln_hamt_amd import HalfRangeWatch
    from vln_hamt_amd._lib import HamtError
    model, batch = _build(), _batch()
    watch = HalfRangeWatch(model, capacity=1)
    with pytest.raises(HamtError, match="capacity"):
        with watch, torch.no_grad():
            model(batch, TASK, True)
    assert not watch.enabled and len(watch.report()) == 1


def test_env_switch_watches_an_unmodified_script():
    """HAMT_HALF_WATCH=1 in a fresh interpreter (the switch is read at import): a script that knows nothing of the watch runs the doctored
    model once; at exit the warning names the doctored layer and the summary line counts the layers"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch\nsys.path.insert(0, 'tests')\nimport test_gpu_half_watch as T\n"
            "m = T._build(T._doctored_sd()[2])\n"
            "with torch.no_grad():\n    m(T._batch(), T.TASK, True)\ntorch.cuda.synchronize()\nprint('script done')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, HAMT_HALF_WATCH="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "script done" in r.stdout and "[HAMT_HALF_WATCH] 16 dense layer(s) watched, 1 at half's limit" in r.stdout, r.stdout
    assert "HalfRangeWarning" in r.stderr and DOCTORED + ": " in r.stderr and "at half's limit" in r.stderr, r.stderr[-3000:]


def test_one_watch_at_a_time():
    from vln_hamt_amd import HalfRangeWatch
    from vln_hamt_amd._lib import HamtError
    a, b = HalfRangeWatch(), HalfRangeWatch()
    with a:
        with pytest.raises(HamtError):
            b.enable()
    b.enable().disable()
