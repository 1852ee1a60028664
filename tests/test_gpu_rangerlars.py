"""-m gpu: RangerLars (Ralamb + Lookahead) on the arenas -- against the reference's own optimizer (tests/golden/rangerlars_tiny.npz,
tools/gen_rangerlars_golden.py), at op level against a float64 restatement, captured against eager, across a checkpoint, over a dropped
pass, and under the gradient exchange."""
import io
import os

import numpy as np
import pytest
import torch

from _util import load_npz, tiny_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_DECAY = ('bias', 'LayerNorm.bias', 'LayerNorm.weight')
ZERO_GRAD = ("next_action.net.4.bias",)       # d(CE)/d(shared logit bias) is exactly 0: its "gradient" is rounding noise (test_gpu_model)


def to_dev(b):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else (v.to(DEV) if torch.is_tensor(v) else v)) for k, v in b.items()}


def build(cfg, sd, prec, train=False):
    from vln_hamt_amd.model.pretrain_cmt import MultiStepNavCMTPreTraining
    from vln_hamt_amd.modeling import HamtConfig
    kw = dict(vars(cfg))
    kw["pretrain_tasks"] = set(cfg.pretrain_tasks)
    m = MultiStepNavCMTPreTraining(HamtConfig(hamt_precision=prec, **kw))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.train(train)
    if train:
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
    return m


def groups(model):
    named = list(model.named_parameters())
    return [{'params': [p for n, p in named if not any(nd in n for nd in NO_DECAY)], 'weight_decay': 0.01},
            {'params': [p for n, p in named if any(nd in n for nd in NO_DECAY)], 'weight_decay': 0.0}]


def tiny_sd(seed=7):
    from oracle.hamt_oracle import make_state_dict, pretrain_param_shapes
    return make_state_dict(pretrain_param_shapes(tiny_cfg()), seed=seed)


def fixture_batch(store, step, cfg):
    """the generator's batch of training step `step` (tools/gen_rangerlars_golden.py:batch_for)"""
    from vln_hamt_amd.synth import make_batch
    task = str(store["meta/tasks"][step - 1])
    return task, to_dev(make_batch(task, 3, cfg, seed=200 + step, txt_len=20, hist_len=4, ragged=True))


def train_steps(model, opt, store, cfg, steps, lr_total=20):
    from oracle.hamt_oracle import lr_at
    from vln_hamt_amd.optim import clip_grad_norm_
    out = []
    for step in steps:
        task, batch = fixture_batch(store, step, cfg)
        loss = model(batch, task, True).mean()
        loss.backward()
        for g in opt.param_groups:
            g['lr'] = lr_at(step, 5e-3, 2, lr_total)
        gn = clip_grad_norm_(model.parameters(), 5.0, optimizer=opt)
        opt.step()
        opt.zero_grad()
        out.append((float(loss), float(gn)))
    return out


def state_by_name(opt, model):
    """state_dict() of the optimizer, per parameter NAME (torch's index = position in the groups' parameter lists)"""
    name_of = {id(p): n for n, p in model.named_parameters()}
    order = [name_of[id(p)] for g in opt.param_groups for p in g["params"]]
    sd = opt.state_dict()
    st = {order[i]: v for i, v in sd["state"].items()}
    slow = {order[i] for i in sd.get("slow_state", {})}
    return st, slow, sd


def test_rangerlars_vs_reference_goldens():
    """The reference's RangerLars (tools/gen_rangerlars_golden.py): pre-loop step() + 17 steps over six tasks, syncs at 5 (create), 11, 17.
    Probe tolerance: 5e-4 absolute = a tenth of the peak learning rate.  An element's update is s*lr*trust*u, |u| ~ 1 after the
    rectification: a wrong trust ratio, decay order, branch or Lookahead action moves elements by ~lr * s per step (an interpolation
    that did not happen: by half of six steps of movement), well above it; the HIP forward / backward differ from the CPU reference by
    rounding only (loss <= 1e-3 as in test_train_steps_vs_optimizer_goldens)."""
    from vln_hamt_amd.optim import RangerLars
    store = load_npz("rangerlars_tiny.npz")
    cfg = tiny_cfg()
    model = build(cfg, tiny_sd(int(store["meta/sd_seed"])), "fp32")
    names = [str(n) for n in store["meta/names"]]
    assert sorted(names) == sorted(n for n, _ in model.named_parameters())
    opt = RangerLars(groups(model), lr=5e-3, betas=(0.9, 0.98))
    assert sorted(n for n, _ in model.named_parameters() if not any(nd in n for nd in NO_DECAY)) == sorted(store["meta/decay_names"].tolist())
    n_probe = int(store["meta/probe_n"])

    def check_state(step):
        pre = f"step{step}/"
        st, slow, sd = state_by_name(opt, model)
        assert [g["lookahead_step"] for g in sd["param_groups"]] == store[pre + "lookahead_step"].tolist(), step
        assert slow == {n for n, h in zip(names, store[pre + "has_slow"]) if h}, (step, sorted(slow ^ {n for n, h in zip(names, store[pre + "has_slow"]) if h}))
        worst = 0.0
        for i, n in enumerate(names):
            assert st.get(n, {}).get("step", 0) == int(store[pre + "step"][i]), (step, n)
            if n in st and n not in ZERO_GRAD:
                for key in ("weight_norm", "adam_norm", "trust_ratio"):
                    ref = float(store[pre + key][i])
                    e = abs(float(st[n][key]) - ref) / max(abs(ref), 1e-12)
                    worst = max(worst, e)
                    assert e <= 1e-4, (step, n, key, float(st[n][key]), ref)
        return worst

    opt.zero_grad()
    opt.step()                                    # main_r2r.py:230
    check_state(0)
    worst_p = worst_s = 0.0
    for step in range(1, 18):
        (loss, gn), = train_steps(model, opt, store, cfg, [step])
        assert abs(loss - float(store[f"step{step}/loss"])) < 1e-3, (step, loss)
        assert abs(gn - float(store[f"step{step}/grad_norm"])) < 2e-3 * float(store[f"step{step}/grad_norm"]), (step, gn)
        cur = dict(model.named_parameters())
        for k in store:
            if k.startswith(f"step{step}/param/"):
                n = k.split("/param/")[1]
                if n in ZERO_GRAD:
                    continue
                f = cur[n].detach().reshape(-1).cpu()
                got = f[:: max(1, f.numel() // n_probe)][:n_probe].numpy()
                d = float(np.abs(got - store[k]).max())
                worst_p = max(worst_p, d)
                assert d < 5e-4, (step, n, d)
        worst_s = max(worst_s, check_state(step))
    print(f"[rangerlars vs reference] worst probe difference {worst_p:.2e}, worst norm / trust relative difference {worst_s:.2e}")


# ------------------------------------------------------------------------------------------------ op level
SIZES = [1, 3, 4, 5, 7, 8, 9, 16, 31, 64, 100, 255, 768, 1000, 1023, 1024, 1025, 2048, 4095, 4096, 4097, 8192, 12289, 30000, 65536,
         100003, 262144, 500000, 1_000_000, 3_000_000]


def _op_case():
    """~30 tensors, 1 element to 3 M: active 0 (slots pre-filled with NaN) / 1 / 2, both N_sma branches, all three Lookahead actions,
    one tensor whose norm is > 10, one all-zero tensor"""
    from vln_hamt_amd.optim.rangerlars import item_table
    rng = np.random.Generator(np.random.PCG64(11))
    nt = len(SIZES)
    offs, n = [], 0
    for s in SIZES:
        offs.append(n)
        n += (s + 7) // 8 * 8
    n = (n + 511) // 512 * 512
    ends = np.array(offs[1:] + [n])
    active = np.array([[1, 2, 0][i % 3] for i in range(nt)], dtype=np.float32)
    rect = np.array([(i // 2) % 2 for i in range(nt)], dtype=np.float32)
    action = np.array([(i // 4) % 3 for i in range(nt)], dtype=np.float32)
    big, zero = SIZES.index(1_000_000), SIZES.index(4096)
    active[big], active[zero] = 1, 1
    lr = np.where(np.arange(nt) % 5 == 0, 3e-3, 1e-3)
    s = np.where(rect == 1, 0.37, 1.9)
    wd = np.where(np.arange(nt) % 4 == 1, 0.0, 0.01)
    alpha = np.where(np.arange(nt) % 2 == 0, 0.5, 0.25)
    hyp = np.stack([lr, s * lr, wd, active], 1).astype(np.float32)
    rl = np.stack([rect, action, alpha, -wd * lr], 1).astype(np.float32)
    p = np.zeros(n, np.float32)
    g, m, v, slow = (np.zeros(n, np.float32) for _ in range(4))
    begins = [0] + list(ends[:-1])
    for i, sz in enumerate(SIZES):
        lo, hi = begins[i], ends[i]
        if active[i] == 0:
            for a in (p, g, m, v, slow):
                a[lo:hi] = np.nan
            continue
        if i == zero:
            continue
        sc = 0.1 if i == big else 0.02
        p[lo:lo + sz] = rng.normal(0, sc, sz)
        g[lo:lo + sz] = rng.normal(0, 1e-2, sz)
        m[lo:lo + sz] = rng.normal(0, 1e-3, sz)
        v[lo:lo + sz] = rng.uniform(1e-7, 1e-4, sz)
        slow[lo:lo + sz] = p[lo:lo + sz] + rng.normal(0, 1e-3, sz)
    assert np.linalg.norm(p[begins[big]:ends[big]].astype(np.float64)) > 10
    tab, nitems = item_table(ends, n)
    return dict(n=n, ends=ends, begins=begins, active=active, rect=rect, action=action, hyp=hyp, rl=rl, p=p, g=g, m=m, v=v, slow=slow,
                tab=tab, nitems=nitems, zero=zero, big=big)


def _restate(c, max_norm, gsq, b1, b2, eps):
    """float64 restatement of ralamb.py:43-95 + lookahead.py:29-39 per tensor"""
    coef = min(1.0, max_norm / (float(np.sqrt(np.float32(gsq))) + 1e-6))
    out = {k: c[k].astype(np.float64).copy() for k in ("p", "g", "m", "v", "slow")}
    stats = {}
    for i in range(len(c["ends"])):
        if c["active"][i] == 0:
            continue
        sl = slice(c["begins"][i], c["ends"][i])
        lr, slr, wd = (float(x) for x in c["hyp"][i, :3])
        p, g, m, v = (c[k][sl].astype(np.float64) for k in ("p", "g", "m", "v"))
        gg = g * coef
        m = b1 * m + (1 - b1) * gg
        v = b2 * v + (1 - b2) * gg * gg
        pd = p - wd * lr * p
        u = m / (np.sqrt(v) + eps) if c["rect"][i] else m
        wn = min(np.sqrt((pd * pd).sum()), 10.0)
        an = np.sqrt(((pd - slr * u) ** 2).sum())
        tr = 1.0 if wn == 0 or an == 0 else wn / an
        pn = pd - slr * tr * u
        a = int(c["action"][i])
        if a == 1:
            out["slow"][sl] = pn
        elif a == 2:
            s = out["slow"][sl] + c["rl"][i, 2] * (pn - out["slow"][sl])
            out["slow"][sl], pn = s, s
        out["p"][sl], out["m"][sl], out["v"][sl] = pn, m, v
        if c["active"][i] == 1:
            out["g"][sl] = 0.0
        stats[i] = (wn, an, tr)
    return out, stats


def test_ralamb_table_op_vs_float64():
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd.ops import _p, _stream
    c = _op_case()
    b1, b2, eps, max_norm, gsq = 0.9, 0.98, 1e-8, 1.0, 25.0         # clip coefficient 1 / (5 + 1e-6) < 1
    d = {k: torch.from_numpy(c[k]).to(DEV) for k in ("p", "g", "m", "v", "slow")}
    d["p16"] = torch.full((c["n"],), float("nan"), device=DEV).to(torch.bfloat16)
    for i in range(len(c["ends"])):
        if c["active"][i] != 0:
            d["p16"][c["begins"][i]:c["ends"][i]] = 0
    d["stats"] = torch.full((len(c["ends"]), 4), 7.0, device=DEV)
    init = {k: t.clone() for k, t in d.items()}
    items = torch.from_numpy(c["tab"]).to(DEV)
    hyp, rl = torch.from_numpy(c["hyp"]).to(DEV), torch.from_numpy(c["rl"]).to(DEV)
    partials = torch.zeros(2 * c["nitems"], device=DEV)
    gn = torch.tensor([gsq], device=DEV)

    def launch():
        L.check(L.load().hamt_ralamb_table(_p(d["p"]), _p(d["g"]), _p(d["m"]), _p(d["v"]), _p(d["p16"]), _p(d["slow"]), _p(items), c["nitems"],
                                           _p(hyp), _p(rl), len(c["ends"]), _p(partials), _p(d["stats"]), _p(gn), max_norm, b1, b2, 1 - b1, 1 - b2,
                                           eps, 1, _stream()), "hamt_ralamb_table")
        torch.cuda.synchronize()
        return {k: t.clone() for k, t in d.items()}

    first = launch()
    want, stats = _restate(c, max_norm, gsq, b1, b2, eps)
    bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)
    st = first["stats"].cpu().double()
    for i in range(len(c["ends"])):
        sl = slice(c["begins"][i], c["ends"][i])
        if c["active"][i] == 0:                  # untouched, byte for byte, whatever the slots hold
            for k in ("p", "g", "m", "v", "slow", "p16"):
                assert torch.equal(bits(first[k][sl]), bits(init[k][sl])), (i, k)
            assert torch.equal(first["stats"][i], init["stats"][i])
            continue
        for k in ("p", "m", "v", "slow"):
            ref = torch.from_numpy(want[k][sl])
            got = first[k][sl].cpu().double()
            scale = max(float(ref.abs().max()), 1e-30)
            err = float((got - ref).abs().max()) / scale
            assert err <= 2e-6, (i, SIZES[i], k, err)
        assert torch.equal(bits(first["p16"][sl]), bits(first["p"][sl].to(torch.bfloat16))), i          # shadow of the final value
        g_want = init["g"][sl] if c["active"][i] == 2 else torch.zeros_like(init["g"][sl])
        assert torch.equal(bits(first["g"][sl]), bits(g_want)), i
        if c["action"][i] == 0:
            assert torch.equal(bits(first["slow"][sl]), bits(init["slow"][sl])), i
        for j, ref in enumerate(stats[i]):
            assert abs(float(st[i, j]) - ref) <= 1e-5 * max(abs(ref), 1e-30), (i, j, float(st[i, j]), ref)
    assert float(st[c["big"], 0]) == 10.0 and float(st[c["zero"], 2]) == 1.0 and float(st[c["zero"], 0]) == 0.0
    for k, t in init.items():                    # a second launch on the same inputs: bit-identical
        d[k].copy_(t)
    second = launch()
    for k in first:
        assert torch.equal(bits(first[k]), bits(second[k])), k


# ------------------------------------------------------------------------------------------------ step machinery
def test_graph_replay_matches_eager_rangerlars():
    """hipGraph-captured steps (graph.GraphedTrainStep) == eager steps, bf16, pre-loop step + 13 steps (syncs at 5 and 11); bound and
    eps = 1.0 as test_graph_replay_matches_eager_steps"""
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.optim import RangerLars, clip_grad_norm_
    from vln_hamt_amd.synth import make_batch, make_itm_rng
    cfg, sd = tiny_cfg(), tiny_sd(7)

    def make():
        m = build(cfg, sd, "bf16", train=True)
        o = RangerLars(groups(m), lr=1e-3, betas=(0.9, 0.98), eps=1.0)
        o.zero_grad()
        o.step()
        return m, o

    seq = ["sap", "mlm", "itm", "mrc"] * 3 + ["sap"]
    batches = {}
    for t in set(seq):
        b = make_batch(t, 4, cfg, seed=sum(map(ord, t)), txt_len=20, hist_len=4, ragged=True, device=DEV)
        if t == "itm":
            r = make_itm_rng(b, seed=3)
            b["itm_neg_idxs"], b["itm_shuffled_pos_ids"] = r["neg_idxs"], r["shuffled_pos_ids"]
        batches[t] = b
    m1, o1 = make()
    for t in seq:
        m1(batches[t], t, True).mean().backward()
        clip_grad_norm_(m1.parameters(), 5.0, optimizer=o1)
        o1.step()
        o1.zero_grad()
    m2, o2 = make()
    gs = GraphedTrainStep(m2, o2, 5.0)
    for t in seq:
        gs.step(t, batches[t], t)
    gs.finish()
    torch.cuda.synchronize()
    assert len(gs.graphs) == 4
    assert [g["lookahead_step"] for g in o1.param_groups] == [g["lookahead_step"] for g in o2.param_groups] == [14, 14]
    assert (o1._steps == o2._steps).all() and (o1._has_slow == o2._has_slow).all() and o1._has_slow.any()
    worst = max(float((a - b).abs().max()) for (_, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()))
    ws = float((o1._flat_slow - o2._flat_slow).abs().max())
    print(f"[rangerlars graph vs eager] worst parameter difference after {len(seq)} steps: {worst:.2e}, slow weights {ws:.2e}")
    assert worst < 2e-5 and ws < 2e-5, (worst, ws)


def test_rangerlars_checkpoint_resume_is_bit_identical():
    """7 steps, state_dict (through torch.save), a fresh model + optimizer, load, on to 17 == 17 uninterrupted steps, bit for bit (fp32)"""
    from vln_hamt_amd.optim import RangerLars
    store = load_npz("rangerlars_tiny.npz")
    cfg, sd = tiny_cfg(), tiny_sd(7)

    def fresh(msd=None):
        m = build(cfg, sd if msd is None else msd, "fp32")
        return m, RangerLars(groups(m), lr=5e-3, betas=(0.9, 0.98))

    m1, o1 = fresh()
    o1.zero_grad()
    o1.step()
    train_steps(m1, o1, store, cfg, range(1, 18))
    m2, o2 = fresh()
    o2.zero_grad()
    o2.step()
    train_steps(m2, o2, store, cfg, range(1, 8))
    buf = io.BytesIO()
    torch.save({"model": {k: v.cpu() for k, v in m2.state_dict().items()}, "optimizer": o2.state_dict()}, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    assert len(ck["optimizer"]["slow_state"]) > 0 and all(isinstance(k, int) for k in ck["optimizer"]["slow_state"])
    m3, o3 = fresh(ck["model"])
    o3.load_state_dict(ck["optimizer"])
    assert (o3._has_slow == o2._has_slow).all() and torch.equal(o3._flat_slow, o2._flat_slow)
    train_steps(m3, o3, store, cfg, range(8, 18))
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
        assert torch.equal(a, b), n
    assert torch.equal(o1._flat_slow, o3._flat_slow) and torch.equal(o1._flat_m, o3._flat_m) and torch.equal(o1._flat_v, o3._flat_v)
    assert (o1._steps == o3._steps).all() and [g["lookahead_step"] for g in o1.param_groups] == [g["lookahead_step"] for g in o3.param_groups]
    # a dict without 'slow_state' (a Ralamb / reference-style checkpoint without Lookahead): the slow weights start fresh
    m4, o4 = fresh(ck["model"])
    o4.load_state_dict({"state": ck["optimizer"]["state"], "param_groups": ck["optimizer"]["param_groups"]})
    assert not o4._has_slow.any() and o4.state_dict()["slow_state"] == {}


def test_rangerlars_dropped_pass_takes_its_counts_back():
    """clip_grad_norm_ (counts the step) then zero_grad() without step(), on the pass that would have been a Lookahead sync: step counts,
    the Lookahead counter and the slow buffers equal those of a run without that pass (the reference counts inside step() only)"""
    from vln_hamt_amd.optim import RangerLars, clip_grad_norm_
    store = load_npz("rangerlars_tiny.npz")
    cfg, sd = tiny_cfg(), tiny_sd(7)
    runs = []
    for drop in (False, True):
        m = build(cfg, sd, "fp32")
        o = RangerLars(groups(m), lr=5e-3, betas=(0.9, 0.98))
        o.zero_grad()
        o.step()
        train_steps(m, o, store, cfg, range(1, 5))
        if drop:
            task, batch = fixture_batch(store, 2, cfg)        # an MLM pass: another set of active parameters
            m(batch, task, True).mean().backward()
            clip_grad_norm_(m.parameters(), 5.0, optimizer=o)
            assert o._counted is not None and o.param_groups[0]["lookahead_step"] == 6
            o.zero_grad()
        assert [g["lookahead_step"] for g in o.param_groups] == [5, 5]
        train_steps(m, o, store, cfg, range(5, 9))
        torch.cuda.synchronize()
        runs.append((m, o))
    (m1, o1), (m2, o2) = runs
    assert (o1._steps == o2._steps).all() and (o1._has_slow == o2._has_slow).all() and o1._has_slow.any()
    assert [g["lookahead_step"] for g in o1.param_groups] == [g["lookahead_step"] for g in o2.param_groups] == [9, 9]
    worst = max(float((a - b).abs().max()) for (_, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()))
    assert worst < 1e-6, worst


# ------------------------------------------------------------------------------------------------ exchange
def test_rangerlars_exchange_choice_and_refusals():
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.optim import RangerLars
    from vln_hamt_amd.parallel import OverlappedGradSync, ShardedGradSync, make_grad_sync
    cfg, sd = tiny_cfg(), tiny_sd(7)
    m = build(cfg, sd, "bf16", train=True)
    o = RangerLars(groups(m), lr=1e-3, betas=(0.9, 0.98)).materialize()
    sync = make_grad_sync(o, "bf16")
    try:
        assert type(sync) is OverlappedGradSync
    finally:
        sync.close()
    with pytest.raises(ValueError, match="all-reduce"):
        ShardedGradSync(o)
    with pytest.raises(L.HamtError):
        o.attach(m)
    with pytest.raises(L.HamtError):
        GraphedTrainStep(m, o, 5.0, overlap_update=True)


def test_rangerlars_one_rank_exchange_matches_single_process():
    """OverlappedGradSync through a one-rank group == plain single-process steps, captured and eager (pattern of
    test_overlapped_grad_sync_matches_single_process_steps, fp32 wire)"""
    import torch.distributed as dist
    from vln_hamt_amd import wgrad
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.optim import RangerLars, clip_grad_norm_
    from vln_hamt_amd.parallel import OverlappedGradSync, broadcast_params
    from vln_hamt_amd.synth import make_batch
    if not wgrad.ENABLED:
        pytest.skip("HAMT_NO_DEFER_WGRAD: no queued weight gradients to overlap with")
    cfg, sd = tiny_cfg(), tiny_sd(7)

    def make():
        m = build(cfg, sd, "bf16", train=True)
        o = RangerLars(groups(m), lr=1e-3, betas=(0.9, 0.98), eps=1.0)
        o.zero_grad()
        o.step()
        return m, o

    seq = ["sap", "mlm", "sap", "mrc", "mlm", "sap", "mrc"]
    batches = {t: make_batch(t, 4, cfg, seed=sum(map(ord, t)), txt_len=20, hist_len=4, ragged=True, device=DEV) for t in set(seq)}
    m1, o1 = make()
    for t in seq:
        m1(batches[t], t, True).mean().backward()
        clip_grad_norm_(m1.parameters(), 5.0, optimizer=o1)
        o1.step()
        o1.zero_grad()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29577")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        for use_graph in (True, False):
            m2, o2 = make()
            broadcast_params(o2)
            sync = OverlappedGradSync(o2, n_groups=3, wire="fp32")
            try:
                if use_graph:
                    gs = GraphedTrainStep(m2, o2, 5.0, grad_sync=sync)
                    for t in seq:
                        gs.step(t, batches[t], t)
                else:
                    for t in seq:
                        m2(batches[t], t, True).mean().backward()
                        sync(o2)
                        clip_grad_norm_(m2.parameters(), 5.0, optimizer=o2)
                        o2.step()
                        o2.zero_grad()
            finally:
                sync.close()
            torch.cuda.synchronize()
            worst = max(float((a - b).abs().max()) for (_, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()))
            print(f"[rangerlars one-rank exchange, graph={use_graph}] worst parameter difference after {len(seq)} steps: {worst:.2e}")
            assert worst < 2e-5, (use_graph, worst)
            assert (o1._has_slow == o2._has_slow).all() and o1._has_slow.any()
    finally:
        if created:
            dist.destroy_process_group()


def _rl_rank_worker(rank, world, port, out_dir):
    """one data-parallel rank with its own batches, gloo carrying the CUDA tensors (two ranks share the one GPU)"""
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from vln_hamt_amd.optim import RangerLars, clip_grad_norm_
    from vln_hamt_amd.parallel import OverlappedGradSync, broadcast_params, make_grad_sync
    from vln_hamt_amd.synth import make_batch
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = tiny_cfg()
        m = build(cfg, tiny_sd(5), "bf16", train=True)
        o = RangerLars(groups(m), lr=1e-3, betas=(0.9, 0.98)).materialize()
        broadcast_params(o)
        sync = make_grad_sync(o, "bf16")
        assert type(sync) is OverlappedGradSync
        try:
            o.zero_grad()
            o.step()
            for i, t in enumerate(["sap", "mlm", "sap", "mrc", "sap", "mlm", "sap"]):
                b = make_batch(t, 4, cfg, seed=1000 * rank + i, txt_len=20, hist_len=4, ragged=True, device=DEV)
                m(b, t, True).mean().backward()
                sync(o)
                clip_grad_norm_(m.parameters(), 5.0, optimizer=o)
                o.step()
                o.zero_grad()
            torch.cuda.synchronize()
        finally:
            sync.close()
        assert o._has_slow.any()
        torch.save({"p": o._flat_p.cpu(), "slow": o._flat_slow.cpu(), "p16": o._flat_p16.cpu()}, os.path.join(out_dir, f"rl{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_rangerlars_two_ranks_on_one_gpu_stay_identical(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rl_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(os.path.join(str(tmp_path), f"rl{r}.pt")) for r in range(2))
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: the ranks diverged"
