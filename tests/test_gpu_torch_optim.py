"""-m gpu: torch.optim's AdamW / Adam / RMSprop / SGD on the arenas (hamt_optim_table, optim.torch_rules, agent.optim):
  6   the kernel at op level against the float64 restatement of tests/_torch_optim_ref.py (test_torch_optim_ref.py shows on the CPU that the
      restatement is torch's arithmetic and that the cases tell a wrong kernel from a right one), its bit rules and argument errors;
  7   the four optimisers on bare parameters over five steps against torch.optim on the CPU in float64;
  8   the agents' pair (vln_bert clipped at 40, critic not) against a float64 twin fed the device's own gradients;
  9   checkpoints: across a reload, to and from torch.optim, the agents' layout;
  10  a rollout training step captured in one graph against the eager loop;
  11  the gradient exchange."""
import copy
import os
import types

import numpy as np
import pytest
import torch

import _adamw_ref as A
import _torch_optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 1024                      # elements behind every array that no launch may touch
CANARY_VALUE = 1234.5
KEYS = ("p", "g", "m", "v", "p16")
GSQ, MAX_NORM = 25.0, 1.0          # clip coefficient 1 / (5 + 1e-6) < 1
ERR_ARG = -1                       # HAMT_ERR_ARG


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    A.make_case.cache_clear()
    A.small_case.cache_clear()
    R.medium_case.cache_clear()


def _lib():
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd.ops import _p, _stream
    return L, _p, _stream


def _classes():
    from vln_hamt_amd.optim import TorchAdam, TorchAdamW, TorchRMSprop, TorchSGD
    return {R.ADAMW: TorchAdamW, R.ADAM: TorchAdam, R.RMSPROP: TorchRMSprop, R.SGD: TorchSGD}


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def with_canary(a, dtype=torch.float32):
    t = torch.full((a.size + CANARY,), CANARY_VALUE, dtype=dtype, device=DEV)
    t[:a.size] = torch.from_numpy(a).to(DEV).to(dtype)
    return t


def arena_init(c, unowned="nan"):
    """the case on the device, a canary behind every array; the m / v arenas the rule does not own are NaN-filled buffers (`unowned` ==
    "nan") or absent ("null")"""
    rule = c["rule"]
    d = {k: with_canary(c[k]) for k in ("p", "g")}
    for k, has in (("m", R.HAS_M[rule]), ("v", R.HAS_V[rule])):
        if has:
            d[k] = with_canary(c[k])
        elif unowned == "nan":
            d[k] = with_canary(np.full(c["n"], np.nan, dtype=np.float32))
        else:
            d[k] = None
    d["p16"] = with_canary(np.full(c["n"], np.nan, dtype=np.float32), torch.bfloat16)
    return d


def launch(c, d, gsq, max_norm, zero_grad=1, p16=True, rule=None, n=None, null=()):
    """hamt_optim_table on the case; returns the status (no exception: the argument-error test reads it)"""
    L, _p, _stream = _lib()
    ends = torch.from_numpy(c["ends"].astype(np.int32)).to(DEV)
    hyp, aux = torch.from_numpy(c["hyp"]).to(DEV), torch.from_numpy(c["aux"]).to(DEV)
    gn = None if gsq is None else torch.tensor([gsq], dtype=torch.float32, device=DEV)
    ptr = lambda k, t: None if (t is None or k in null) else _p(t)
    rc = L.load().hamt_optim_table(c["rule"] if rule is None else rule, c["n"] if n is None else n, ptr("p", d["p"]), ptr("g", d["g"]),
                                   ptr("m", d["m"]), ptr("v", d["v"]), ptr("p16", d["p16"]) if p16 else None, ptr("ends", ends),
                                   ptr("hyp", hyp), ptr("aux", aux), len(c["ends"]), _p(gn), float(max_norm), c["b1"], c["b2"], c["eps"],
                                   int(zero_grad), _stream())
    torch.cuda.synchronize()
    return rc


def clone(d):
    return {k: (None if t is None else t.clone()) for k, t in d.items()}


def check_table(c, init, out, want, zero_grad=1, p16=True):
    """`out` against the float64 restatement `want` and the bit rules of every array"""
    n, rule = c["n"], c["rule"]
    reps = np.diff(np.concatenate([c["begins"], [n]]))
    flag = torch.from_numpy(np.repeat(c["flags"], reps)).to(DEV)
    live, act = flag != 0, c["flags"] != 0
    for k in R.live_arrays(rule):
        got = out[k][:n].cpu().numpy().astype(np.float64)
        err = A.tensor_max(c, got - want[k])[act]
        scale = np.maximum(A.tensor_max(c, want[k])[act], 1e-30)
        i = int(np.argmax(err / scale))
        print(f"[{R.NAMES[rule]} table, {len(c['ends'])} rows] {k}: worst per-tensor error {err[i] / scale[i]:.2e} of max|ref|")
        assert (err <= R.TOL * scale).all(), (k, int(np.flatnonzero(act)[i]), err[i] / scale[i])
        assert not np.isnan(got[act.repeat(reps)]).any(), k
    for k in KEYS:
        if out[k] is None:
            continue
        if k in "mv" and k not in R.live_arrays(rule):        # an arena the rule does not own: not one bit of it
            assert same_bits(out[k], init[k]), k
            continue
        assert same_bits(out[k][:n][~live], init[k][:n][~live]), k     # no gradient: untouched, whatever the slots hold (NaN)
        assert same_bits(out[k][n:], init[k][n:]), k                   # the canary
    if p16:                                          # the shadow of the FINAL value
        assert same_bits(out["p16"][:n][live], out["p"][:n].to(torch.bfloat16)[live])
    else:
        assert same_bits(out["p16"], init["p16"])
    zeroed = (flag == 1) if zero_grad else torch.zeros_like(live)
    assert not bits(out["g"][:n][zeroed]).any()
    assert same_bits(out["g"][:n][~zeroed], init["g"][:n][~zeroed])
    pad = slice(int(c["ends"][-1]), n)               # behind the last tensor: the last row's hyper-parameters on zeros
    for k in R.live_arrays(rule):
        assert torch.isfinite(out[k][pad]).all(), k


def _cases():
    return [(n, r) for n in ("small", "medium") for r in R.RULES] + [("arena", R.ADAMW)]


_ids = lambda x: R.NAMES.get(x, x) if isinstance(x, int) else x


# ------------------------------------------------------------------------------------------------ 6: the kernel
@pytest.mark.parametrize("name,rule", _cases(), ids=_ids)
def test_optim_table_vs_float64(name, rule):
    """every rule on the small and the medium arena, AdamW also on the one of more than a grid sweep: clip below 1, gradient slots
    zeroed, shadow written, un-owned arenas passed as NaN-filled buffers; a second launch from the same inputs is bit-identical"""
    c = R.with_rule(R.layouts()[name](), rule, "hot")
    d = arena_init(c)
    init = clone(d)
    assert launch(c, d, GSQ, MAX_NORM) == 0
    check_table(c, init, d, R.restate(c, A.clip_coef(float(np.float32(GSQ)), MAX_NORM)))
    again = clone(init)
    assert launch(c, again, GSQ, MAX_NORM) == 0
    for k in KEYS:
        assert same_bits(again[k], d[k]), k


@pytest.mark.parametrize("variant", ["keep_grad", "no_shadow", "no_norm", "max_norm_0", "norm_below", "agent", "null_unowned", "flag3"])
@pytest.mark.parametrize("rule", R.RULES, ids=_ids)
@pytest.mark.parametrize("name", ["small", "medium"])
def test_optim_table_variants(name, rule, variant):
    c = R.with_rule(R.layouts()[name](), rule, "agent" if variant == "agent" else "hot")
    gsq, max_norm, zero_grad, p16, unowned = GSQ, MAX_NORM, 1, True, "nan"
    if variant == "keep_grad":
        zero_grad = 0
    elif variant == "no_shadow":
        p16 = False
    elif variant == "no_norm":
        gsq = None
    elif variant == "max_norm_0":
        max_norm = 0.0
    elif variant == "norm_below":
        gsq = 0.25
    elif variant == "null_unowned":
        unowned = "null"
    elif variant == "flag3":                         # 3: like 2 for the update (the norm kernel is what tells them apart)
        c["flags"] = np.where(c["flags"] == 2, 3, c["flags"]).astype(c["flags"].dtype)
        c["hyp"] = c["hyp"].copy()
        c["hyp"][:, 3] = c["flags"]
        assert (c["flags"] == 3).any() and (c["flags"] == 1).any() and (c["flags"] == 0).any()
    coef = A.clip_coef(gsq, max_norm)
    assert (coef == 1.0) == (variant in ("no_norm", "max_norm_0", "norm_below"))
    d = arena_init(c, unowned)
    assert (d["m"] is None) == (unowned == "null" and not R.HAS_M[rule]) and (d["v"] is None) == (unowned == "null" and not R.HAS_V[rule])
    init = clone(d)
    assert launch(c, d, gsq, max_norm, zero_grad, p16) == 0
    check_table(c, init, d, R.restate(c, coef, zero_grad), zero_grad, p16)


@pytest.mark.parametrize("rule", R.RULES, ids=_ids)
def test_optim_table_argument_errors_launch_nothing(rule):
    L, _, _ = _lib()
    c = R.with_rule(A.small_case(), rule, "hot")
    d = arena_init(c)
    init = clone(d)
    bad = [dict(rule=4), dict(rule=-1), dict(n=c["n"] - 2), dict(null=("ends",)), dict(null=("hyp",)), dict(null=("aux",)),
           dict(null=("p",)), dict(null=("g",))]
    if R.HAS_M[rule]:
        bad.append(dict(null=("m",)))
    if R.HAS_V[rule]:
        bad.append(dict(null=("v",)))
    for kw in bad:
        assert launch(c, d, GSQ, MAX_NORM, **kw) == ERR_ARG, kw
        assert "hamt_optim_table" in L.last_error()
        for k in KEYS:
            assert same_bits(d[k], init[k]), (kw, k)
    for k, has in (("m", R.HAS_M[rule]), ("v", R.HAS_V[rule])):      # ... and an arena the rule does not need may be NULL
        if not has:
            assert launch(c, clone(init), GSQ, MAX_NORM, null=(k,)) == 0


# ------------------------------------------------------------------------------------------------ 7: the optimisers, bare parameters
@pytest.mark.parametrize("rule", R.RULES, ids=_ids)
def test_python_steps_vs_torch_float64(rule):
    """Five steps on eight bare parameters in two groups (wd 0.05 / 0), lr of each group changed every step, clip_grad_norm_ at 40 with the
    norm above it in steps 1, 3, 5 and below in 2 and 4; parameters PY_LAG have no gradient in steps 2 and 3.  After every step each
    parameter against torch.optim + torch.nn.utils.clip_grad_norm_ on the CPU in float64."""
    from vln_hamt_amd.optim import clip_grad_norm_
    from vln_hamt_amd.optim.adamw import shadow_only
    pc, ref = R.py_case(), R.py_run_torch(rule)
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in pc["init"]]
    assert shadow_only(params[A.PY_LAG[0]]) and not shadow_only(params[A.PY_LAG[1]])
    opt = _classes()[rule]([{"params": [p for p, g in zip(params, A.PY_GROUP) if g == k], "weight_decay": R.PY_WD[k]} for k in (0, 1)],
                           lr=1e-3, **R.PY_DEFAULTS[rule])
    opt.materialize()
    assert (opt._flat_m is not None) == R.HAS_M[rule] and (opt._flat_v is not None) == R.HAS_V[rule]
    where = [slice(opt._offs[opt._index_of[id(p)]], opt._offs[opt._index_of[id(p)]] + p.numel()) for p in params]
    clipped, worst = [], 0.0
    for s, grads in enumerate(pc["grads"]):
        for p, g in zip(params, grads):
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)
        for k, grp in enumerate(opt.param_groups):
            grp["lr"] = A.PY_LR[s][k]
        before = opt._flat_p.clone()
        gn = clip_grad_norm_(params, R.PY_MAX_NORM, optimizer=opt)
        if s == 2:                                   # a change between the clip and the step: the table is rebuilt, the step counted once
            for k, grp in enumerate(opt.param_groups):
                grp["lr"] = 7.0
            opt._ensure_table()
            for k, grp in enumerate(opt.param_groups):
                grp["lr"] = A.PY_LR[s][k]
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        assert abs(float(gn) - ref[s]["norm"]) <= 1e-5 * ref[s]["norm"], (s, float(gn), ref[s]["norm"])
        clipped.append(ref[s]["norm"] > R.PY_MAX_NORM)
        for i, (p, g, sl) in enumerate(zip(params, grads, where)):
            if g is None:
                assert same_bits(opt._flat_p[sl], before[sl]), (s, i)
                continue
            got, want = p.detach().cpu().numpy().reshape(-1).astype(np.float64), ref[s]["p"][i]
            err = float(np.abs(got - want).max()) / float(np.abs(want).max())
            worst = max(worst, err)
            assert err <= R.TOL, (s, i, err)
            assert same_bits(opt._flat_p16[sl], opt._flat_p[sl].to(torch.bfloat16)), (s, i)
    print(f"[{R.NAMES[rule]} python steps] worst per-tensor error over 5 steps {worst:.2e} of max|ref|")
    assert clipped == [True, False, True, False, True]                    # both sides of the clip happened
    assert opt._steps[[opt._index_of[id(p)] for p in params]].tolist() == [3 if i in A.PY_LAG else 5 for i in range(len(params))]


@pytest.mark.parametrize("rule", [R.ADAMW, R.RMSPROP], ids=_ids)
def test_dropped_pass_takes_its_count_back(rule):
    """clip_grad_norm_ counted the step, zero_grad() without step() drops it: the next real step is the first one, as in torch"""
    from vln_hamt_amd.optim import clip_grad_norm_
    pc = R.py_case()
    runs = []
    for drop in (False, True):
        params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in pc["init"]]
        opt = _classes()[rule](params, lr=1e-2, **R.PY_DEFAULTS[rule])
        if drop:
            for p, g in zip(params, pc["grads"][4]):
                p.grad = torch.from_numpy(g).to(DEV)
            clip_grad_norm_(params, R.PY_MAX_NORM, optimizer=opt)
            assert opt._steps.sum() == len(params)
            opt.zero_grad()
            assert opt._steps.sum() == 0
        for p, g in zip(params, pc["grads"][0]):
            p.grad = torch.from_numpy(g).to(DEV)
        clip_grad_norm_(params, R.PY_MAX_NORM, optimizer=opt)
        opt.step()
        opt.zero_grad()
        runs.append((params, opt))
    torch.cuda.synchronize()
    assert (runs[0][1]._steps == 1).all() and (runs[1][1]._steps == 1).all()
    for a, b in zip(runs[0][0], runs[1][0]):
        assert same_bits(a.detach().reshape(-1), b.detach().reshape(-1))


# ------------------------------------------------------------------------------------------------ 8: the agents' pair
def _agent_models():
    from test_gpu_model import _tiny_navcmt
    from vln_hamt_amd.models.model_HAMT import Critic
    torch.manual_seed(11)
    critic = Critic(types.SimpleNamespace(dropout=0.0, hamt_precision="bf16")).to(DEV).train(True)
    return _tiny_navcmt(train=True, p_drop=0.0), critic


def _agent_batches(n, T=3):
    from _util import tiny_cfg
    from vln_hamt_amd.synth import make_batch
    cfg = tiny_cfg(no_lang_ca=True, act_pred_token="ob")
    out = []
    for i in range(n):
        b = make_batch("sap", 4, cfg, seed=90 + i, txt_len=24, hist_len=T, device=DEV)
        b["step_ids"] = torch.arange(T, device=DEV)
        g = torch.Generator().manual_seed(300 + i)
        b["critic_in"] = torch.randn(T, 4, 768, generator=g).to(DEV)       # (the reference feeds the critic a DETACHED state: its gradients
        b["critic_target"] = torch.randn(T, 4, generator=g).to(DEV)        # do not reach vln_bert, any input serves)
        out.append(b)
    return out


def _agent_loss(vln_bert, critic, b, T=3):
    from test_gpu_model import _rollout_loss
    loss = _rollout_loss(vln_bert, b, T)
    for t in range(T):
        loss = loss + 0.5 * ((critic(b["critic_in"][t]) - b["critic_target"][t]) ** 2).mean()
    return loss


def test_agent_optimizers_vs_float64_twin():
    """three iterations of a 3-step imitation + critic loss through AgentOptimizers.optim_step (--optim adamW); after each backward the
    device's gradients go to a CPU float64 twin that runs clip_grad_norm_(vln_bert twin, 40.) and two torch.optim.AdamW.step() -- the
    twin never computes a gradient of its own (Adam's first steps are lr * sign(g): two backward passes that differ in the last bit
    would not be comparable).  The loss scale makes the clip bite in the second iteration only; a third twin whose CRITIC gradients are
    scaled too must end up visibly elsewhere."""
    from vln_hamt_amd.agent import build_agent_optimizers
    vln_bert, critic = _agent_models()
    ao = build_agent_optimizers(types.SimpleNamespace(optim="adamW", lr=1e-3), vln_bert, critic)
    twins = [[torch.nn.Parameter(p.detach().cpu().double()) for p in m.parameters()] for m in (vln_bert, critic)]
    topt = [torch.optim.AdamW(t, lr=1e-3) for t in twins]
    wrong = [torch.nn.Parameter(p.detach().cpu().double()) for p in critic.parameters()]
    wopt = torch.optim.AdamW(wrong, lr=1e-3)
    scales, bit, worst = [1.0, 300.0, 1.0], [], 0.0
    for it, (b, scale) in enumerate(zip(_agent_batches(3), scales)):
        ao.zero_grad()
        loss = _agent_loss(vln_bert, critic, b) * scale
        loss.backward()
        for model, twin in zip((vln_bert, critic), twins):
            for p, q in zip(model.parameters(), twin):
                q.grad = None if p.grad is None else p.grad.detach().cpu().double().clone()
        critic_grads = [p.grad.detach().clone() for p in critic.parameters()]
        gn = ao.optim_step()
        norm = float(torch.nn.utils.clip_grad_norm_(twins[0], 40.))
        coef = min(1.0, 40.0 / (norm + 1e-6))
        for w, g in zip(wrong, critic_grads):
            w.grad = g.cpu().double() * coef
        for o in topt + [wopt]:
            o.step()
        torch.cuda.synchronize()
        bit.append(norm > 40.0)
        assert abs(float(gn) - norm) <= 1e-5 * norm, (it, float(gn), norm)
        for model, twin, o in zip((vln_bert, critic), twins, ao.optimizers):
            for (name, p), q in zip(model.named_parameters(), twin):
                want = q.detach().numpy()
                err = float(np.abs(p.detach().cpu().numpy().astype(np.float64) - want).max())
                scale_ = float(np.abs(want).max())
                worst = max(worst, err / max(scale_, 1e-30))
                assert err <= R.TOL * scale_, (it, name, err / max(scale_, 1e-30))
            assert same_bits(o._flat_p16, o._flat_p.to(torch.bfloat16))
    print(f"[agent optimizers] vln_bert norms clipped {bit}; worst per-tensor error over 3 iterations {worst:.2e} of max|ref|")
    assert bit == [False, True, False]
    moved = max(float((w.detach() - q.detach()).abs().max()) / (20 * R.TOL * float(q.detach().abs().max())) for w, q in zip(wrong, twins[1]))
    assert moved >= 1.0, moved                                            # a clipped critic would have been noticed


# ------------------------------------------------------------------------------------------------ 9: checkpoints
def _bare(rule, **kw):
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in R.py_case()["init"]]
    return params, _classes()[rule](params, lr=1e-2, **kw)


def _step(params, opt, s):
    from vln_hamt_amd.optim import clip_grad_norm_
    for p, g in zip(params, R.py_case()["grads"][s]):
        p.grad = None if g is None else torch.from_numpy(g).to(DEV)
    clip_grad_norm_(params, R.PY_MAX_NORM, optimizer=opt)
    opt.step()
    opt.zero_grad()


@pytest.mark.parametrize("rule", R.RULES, ids=_ids)
def test_checkpoint_reload_is_bit_identical(rule):
    params, opt = _bare(rule)
    for s in (0, 1):
        _step(params, opt, s)
    sd = copy.deepcopy(opt.state_dict())
    idx = {id(p): i for i, p in enumerate(params)}
    if rule != R.SGD:
        assert sorted(sd["state"]) == list(range(len(params)))
        want_keys = ["step"] + (["exp_avg", "exp_avg_sq"] if R.HAS_M[rule] else ["square_avg"])
        for i, st in sd["state"].items():
            assert list(st) == want_keys and st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and st["step"].dim() == 0
            assert float(st["step"]) == (1.0 if i in A.PY_LAG else 2.0)
    else:
        assert all(st == {"momentum_buffer": None} for st in sd["state"].values())
    fresh, opt2 = _bare(rule)
    with torch.no_grad():
        for a, b in zip(fresh, params):
            a.copy_(b)
    opt2.load_state_dict(sd)
    _step(params, opt, 2)
    _step(fresh, opt2, 2)
    torch.cuda.synchronize()
    for a, b in zip(params, fresh):
        assert same_bits(a.detach().reshape(-1), b.detach().reshape(-1))
    assert same_bits(opt._flat_p16, opt2._flat_p16)


@pytest.mark.parametrize("name", ["AdamW", "RangerLars", "TorchAdamW"])
def test_resume_inside_a_dropped_pass_forgets_the_counted_step(name):
    """A resume inside a NaN guard: backward, clip_grad_norm_ (which counts the step), load_state_dict, zero_grad().  The counted step
    belongs to the counts the load replaced: zero_grad() must not take it back from the LOADED counts, and the next step must build its
    own table.  Eight bare parameters in two groups (_adamw_ref.PY_SHAPES: a GEMM weight in the shadow region, a 5x7 and a 1-element
    tensor behind alignment gaps); `a` takes three steps and saves, `b` resumes from it as above over clones of a's parameters; two
    further steps leave every arena of the two equal bit for bit."""
    from vln_hamt_amd import optim
    pc = A.py_case()

    def make(init):
        params = [torch.nn.Parameter(t) for t in init]
        groups = [{"params": [p for p, g in zip(params, A.PY_GROUP) if g == k], "weight_decay": A.PY_WD[k]} for k in (0, 1)]
        return params, {"AdamW": lambda: optim.AdamW(groups, lr=1e-3), "RangerLars": lambda: optim.RangerLars(groups, alpha=0.5, k=2, lr=1e-3),
                        "TorchAdamW": lambda: optim.TorchAdamW(groups, lr=1e-3)}[name]()

    def backward(params, s):
        for p, g in zip(params, pc["grads"][s]):
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)

    def step(params, opt, s):
        for k, grp in enumerate(opt.param_groups):
            grp["lr"] = A.PY_LR[s][k]
        backward(params, s)
        optim.clip_grad_norm_(params, A.PY_MAX_NORM, optimizer=opt)
        opt.step()
        opt.zero_grad()

    pa, a = make([torch.from_numpy(x.copy()).to(DEV) for x in pc["init"]])
    for s in range(3):
        step(pa, a, s)
    sd = copy.deepcopy(a.state_dict())
    pb, b = make([p.detach().clone() for p in pa])
    backward(pb, 3)
    optim.clip_grad_norm_(pb, A.PY_MAX_NORM, optimizer=b)
    assert b._counted is not None and b._steps.sum() == len(pb)           # the step is counted
    b.load_state_dict(sd)
    b.zero_grad()
    want = [1 if i in A.PY_LAG else 3 for i in range(len(pa))]          # (PY_LAG: no gradient in steps 2 and 3)
    assert [int(a._steps[a._index_of[id(p)]]) for p in pa] == want
    assert b._steps.tolist() == a._steps.tolist()
    for s in (3, 4):
        step(pa, a, s)
        step(pb, b, s)
    torch.cuda.synchronize()
    assert b._steps.tolist() == a._steps.tolist()
    for k in ("_flat_p", "_flat_m", "_flat_v", "_flat_p16") + (("_flat_slow",) if name == "RangerLars" else ()):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    if name == "RangerLars":
        assert a._has_slow.tolist() == b._has_slow.tolist() and a._has_slow.any()


@pytest.mark.parametrize("int_step", [False, True], ids=["tensor_step", "int_step"])
@pytest.mark.parametrize("rule", [R.ADAMW, R.RMSPROP], ids=_ids)
def test_checkpoint_moves_to_and_from_torch(rule, int_step):
    """our state into torch.optim over CPU float64 clones, and torch's state into ours: the next step within TOL, also when 'step' is an
    integer (as checkpoints of the reference's torch version carry it)"""
    def as_int(sd):
        sd = copy.deepcopy(sd)
        for st in sd["state"].values():
            st["step"] = int(st["step"])
        return sd

    grads = R.py_case()["grads"]
    # ours -> torch
    params, opt = _bare(rule)
    for s in (0, 1):
        _step(params, opt, s)
    twin = [torch.nn.Parameter(p.detach().cpu().double()) for p in params]
    topt = R.torch_class(rule)(twin, lr=1e-2)
    sd = opt.state_dict()
    topt.load_state_dict(as_int(sd) if int_step else sd)
    # torch -> ours
    fresh, opt2 = _bare(rule)
    with torch.no_grad():
        for a, b in zip(fresh, twin):
            a.copy_(b.detach().float())
    sd_t = topt.state_dict()
    opt2.load_state_dict(as_int(sd_t) if int_step else sd_t)
    assert opt2._steps.tolist() == opt._steps.tolist()
    for p, g in zip(twin, grads[2]):
        p.grad = None if g is None else torch.from_numpy(g.astype(np.float64))
    torch.nn.utils.clip_grad_norm_(twin, R.PY_MAX_NORM)
    topt.step()
    _step(params, opt, 2)
    _step(fresh, opt2, 2)
    torch.cuda.synchronize()
    for i, (a, b, q) in enumerate(zip(params, fresh, twin)):
        want = q.detach().numpy()
        for got in (a, b):
            err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())
            assert err <= R.TOL * float(np.abs(want).max()), (i, err / float(np.abs(want).max()))


@pytest.mark.parametrize("prefix", [False, True], ids=["plain", "module_prefix"])
def test_agent_checkpoint_round_trip(prefix):
    """AgentOptimizers.state / .load in the reference's layout; a checkpoint saved from DDP-wrapped models ('module.' keys) loads into
    bare ones; with resume_optimizer the second pair's parameters, moments, step counts and shadows are the first one's, bit for bit"""
    from vln_hamt_amd.agent import build_agent_optimizers
    args = types.SimpleNamespace(optim="adamW", lr=1e-3)
    bs = _agent_batches(3)

    def iterate(ao, b):
        ao.zero_grad()
        ao.optim_step(_agent_loss(ao.vln_bert, ao.critic, b))

    vln_bert, critic = _agent_models()
    ao = build_agent_optimizers(args, vln_bert, critic)
    for b in bs[:2]:
        iterate(ao, b)
    states = copy.deepcopy(ao.states(4))
    for name, model in (("vln_bert", vln_bert), ("critic", critic)):          # states() is state() of each held model
        one = ao.state(name, 4, model)
        assert one["epoch"] == states[name]["epoch"] and list(one["state_dict"]) == list(states[name]["state_dict"])
        assert all(torch.equal(one["state_dict"][k], states[name]["state_dict"][k]) for k in one["state_dict"])
        assert one["optimizer"]["param_groups"] == states[name]["optimizer"]["param_groups"]
        assert sorted(one["optimizer"]["state"]) == sorted(states[name]["optimizer"]["state"])
    assert sorted(states) == ["critic", "vln_bert"]
    for name, model in (("vln_bert", vln_bert), ("critic", critic)):
        assert sorted(states[name]) == ["epoch", "optimizer", "state_dict"] and states[name]["epoch"] == 5
        assert list(states[name]["state_dict"]) == list(model.state_dict())
        assert sorted(states[name]["optimizer"]) == ["param_groups", "state"]
    if prefix:
        for name in states:
            states[name]["state_dict"] = {"module." + k: v for k, v in states[name]["state_dict"].items()}
    vb2, cr2 = _agent_models()
    with torch.no_grad():
        for p in list(vb2.parameters()) + list(cr2.parameters()):
            p.add_(1.0)
    ao2 = build_agent_optimizers(args, vb2, cr2)
    assert ao2.load(states, resume_optimizer=True) == 4
    torch.cuda.synchronize()
    # (compared as loaded, not after another iteration: two backward passes of the same launches differ in the last bit -- atomic
    # scatter-adds -- and Adam turns a gradient that is rounding noise into +-lr)
    for (m1, o1), (m2, o2) in (((vln_bert, ao.vln_bert_optimizer), (vb2, ao2.vln_bert_optimizer)), ((critic, ao.critic_optimizer), (cr2, ao2.critic_optimizer))):
        for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
            assert same_bits(a.detach().reshape(-1), b.detach().reshape(-1)), n
        assert (o1._steps == o2._steps).all() and o2._steps.max() == 2
        for k in ("_flat_p", "_flat_m", "_flat_v", "_flat_p16"):
            assert same_bits(getattr(o1, k), getattr(o2, k)), k
    vb3, cr3 = _agent_models()
    ao3 = build_agent_optimizers(args, vb3, cr3)
    ao3.vln_bert_optimizer.materialize()
    assert ao3.load(states, resume_optimizer=False) == 4
    assert (ao3.vln_bert_optimizer._steps == 0).all()
    o = ao3.vln_bert_optimizer
    assert same_bits(o._flat_p16, o._flat_p.to(torch.bfloat16))           # the shadow follows the loaded masters


# ------------------------------------------------------------------------------------------------ 10: graph capture
def test_graphed_rollout_training_step_matches_eager():
    """test_gpu_model.py::test_graphed_rollout_training_step_matches_eager with TorchAdamW: rollout, backward, clip at 40 and the update
    in ONE graph == the eager loop (that test's bounds: losses 5e-4, parameters 1e-4)"""
    from _util import tiny_cfg
    from test_gpu_model import _rollout_loss, _tiny_navcmt
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.optim import TorchAdamW, clip_grad_norm_
    from vln_hamt_amd.synth import make_batch
    T = 3

    def rollout_loss(model, b, _task):
        return _rollout_loss(model, b, T)

    cfg = tiny_cfg(no_lang_ca=True, act_pred_token="ob")
    bs = []
    for i in range(4):
        b = make_batch("sap", 4, cfg, seed=70 + i, txt_len=24, hist_len=T, device=DEV)
        b["step_ids"] = torch.arange(T, device=DEV)
        bs.append(b)
    models = []
    for graphed in (False, True):
        m = _tiny_navcmt(train=True, p_drop=0.0)
        o = TorchAdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1.0)
        losses = []
        if graphed:
            gs = GraphedTrainStep(m, o, 40.0, loss_fn=rollout_loss)
            for b in bs:
                losses.append(float(gs.step("rollout", b, "rollout")))
            gs.finish()
            assert len(gs.graphs) == 1
        else:
            for b in bs:
                loss = rollout_loss(m, b, None)
                loss.backward()
                clip_grad_norm_(m.parameters(), 40.0, optimizer=o)
                o.step()
                o.zero_grad()
                losses.append(float(loss))
        assert o._steps.max() == len(bs)
        models.append((m, losses))
    torch.cuda.synchronize()
    (m1, l1), (m2, l2) = models
    assert max(abs(a - c) for a, c in zip(l1, l2)) < 5e-4, (l1, l2)
    worst = max(float((a - c).abs().max()) for (_, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()))
    print(f"[graphed rollout step, TorchAdamW] losses {l2}; worst parameter difference vs eager {worst:.2e}")
    assert worst < 1e-4, worst


# ------------------------------------------------------------------------------------------------ 11: exchange
def test_exchange_choice_and_refusals():
    from test_gpu_model import _tiny_navcmt
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.parallel import OverlappedGradSync, ShardedGradSync, make_grad_sync
    m = _tiny_navcmt(train=True, p_drop=0.0)
    for rule, cls in _classes().items():
        o = cls(m.parameters(), lr=1e-3).materialize()
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
            GraphedTrainStep(m, o, 40.0, overlap_update=True)


def _one_rank_group():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29578")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1)
    return created


def _schedule_run(rule, exchange):
    """the python-level schedule on bare parameters, optionally with the one-rank exchange between the gradients and the clip; returns
    the parameter arena after every step and the optimiser"""
    from vln_hamt_amd.optim import clip_grad_norm_
    from vln_hamt_amd.parallel import OverlappedGradSync, broadcast_params
    params, opt = _bare(rule, **R.PY_DEFAULTS[rule])
    opt.materialize()
    sync = None
    if exchange:
        broadcast_params(opt)
        sync = OverlappedGradSync(opt, n_groups=3, wire="fp32")
    try:
        trace = []
        for grads in R.py_case()["grads"]:
            for p, g in zip(params, grads):
                p.grad = None if g is None else torch.from_numpy(g).to(DEV)
            if sync is not None:
                sync(opt)
            clip_grad_norm_(params, R.PY_MAX_NORM, optimizer=opt)
            opt.step()
            opt.zero_grad()
            trace.append(opt._flat_p.clone())
    finally:
        if sync is not None:
            sync.close()
    return trace, opt


def test_one_rank_exchange_step_is_the_single_process_step():
    """the python-level schedule with OverlappedGradSync's exchange (one rank, fp32 wire) between the gradients and the clip: every
    parameter after every step equals the single-process run bit for bit, for all four optimisers -- the gradients are given, so
    nothing but the exchange differs"""
    import torch.distributed as dist
    created = _one_rank_group()
    try:
        for rule in R.RULES:
            (t1, o1), (t2, o2) = _schedule_run(rule, False), _schedule_run(rule, True)
            torch.cuda.synchronize()
            assert (o1._steps == o2._steps).all() and o1._steps.max() == 5
            for s, (a, b) in enumerate(zip(t1, t2)):
                assert same_bits(a, b), (rule, s)
            assert same_bits(o1._flat_p16, o2._flat_p16), rule
    finally:
        if created:
            dist.destroy_process_group()


def test_one_rank_exchange_matches_single_process_model():
    """the same through a model, where the exchange runs inside the weight-gradient plan (the shape and the bound of
    test_rangerlars_one_rank_exchange_matches_single_process: two backward passes, so not bit for bit; eps = 1 keeps Adam from
    amplifying last-bit gradient differences)"""
    import torch.distributed as dist
    from test_gpu_rangerlars import build, tiny_sd
    from _util import tiny_cfg
    from vln_hamt_amd import wgrad
    from vln_hamt_amd.optim import TorchAdamW, clip_grad_norm_
    from vln_hamt_amd.parallel import OverlappedGradSync, broadcast_params
    from vln_hamt_amd.synth import make_batch
    if not wgrad.ENABLED:
        pytest.skip("HAMT_NO_DEFER_WGRAD: no queued weight gradients to overlap with")
    cfg, sd = tiny_cfg(), tiny_sd(7)

    def make():
        m = build(cfg, sd, "bf16", train=True)
        return m, TorchAdamW(m.parameters(), lr=1e-3, eps=1.0)

    seq = ["sap", "mlm", "sap", "mrc"]
    batches = {t: make_batch(t, 4, cfg, seed=sum(map(ord, t)), txt_len=20, hist_len=4, ragged=True, device=DEV) for t in set(seq)}
    m1, o1 = make()
    for t in seq:
        m1(batches[t], t, True).mean().backward()
        clip_grad_norm_(m1.parameters(), 40.0, optimizer=o1)
        o1.step()
        o1.zero_grad()
    created = _one_rank_group()
    try:
        m2, o2 = make()
        broadcast_params(o2)
        sync = OverlappedGradSync(o2, n_groups=3, wire="fp32")
        try:
            for t in seq:
                m2(batches[t], t, True).mean().backward()
                sync(o2)
                clip_grad_norm_(m2.parameters(), 40.0, optimizer=o2)
                o2.step()
                o2.zero_grad()
        finally:
            sync.close()
        torch.cuda.synchronize()
        worst = max(float((a - b).abs().max()) for (_, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()))
        print(f"[TorchAdamW one-rank exchange] worst parameter difference after {len(seq)} steps: {worst:.2e}")
        assert worst < 2e-5, worst
    finally:
        if created:
            dist.destroy_process_group()
