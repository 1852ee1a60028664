"""CPU half of the torch-rule optimiser tests (hamt_optim_table, optim.torch_rules, agent.optim): the numpy float64 restatement of
tests/_torch_optim_ref.py IS torch.optim's arithmetic; its arena cases have the layout the kernel's segment walk needs; fp32 arithmetic in
the kernel's operation order stays well inside the 2e-6 bound on them (so the GPU half can hold the kernel to it); and every mistake the
GPU half is meant to catch -- decay on the wrong side of the update, HF's eps placement, L2 for decoupled decay and back, a missing
1 / sqrt(1 - b2^t), RMSprop's eps inside the root, a missing clip coefficient, a neighbour's table row, the global step count -- moves every
live tensor by far more than the bound.  Plus the host-side pieces that need no GPU: constructors, state_dict layout, the agents' mapping,
the exchange choice, the kernels' resources."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import _adamw_ref as A
import _torch_optim_ref as R

COEF = A.clip_coef(25.0, 1.0)          # 1 / (5 + 1e-6)


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    A.make_case.cache_clear()            # (9 M floats x 4 arrays: not kept for the rest of the session)
    A.small_case.cache_clear()
    R.medium_case.cache_clear()


def _active(c):
    return c["flags"] != 0


# ---------------------------------------------------------------------------------------------- 1. the restatement against torch.optim
@pytest.mark.parametrize("wds", [tuple(R.PY_WD), (0.0, 0.0)], ids=["decay", "no_decay"])
@pytest.mark.parametrize("rule", R.RULES, ids=lambda r: R.NAMES[r])
def test_restatement_is_torch(rule, wds):
    """five steps, two groups, learning rates changing every step, two parameters without a gradient in steps 2 and 3 (their step count
    lags), the clip at 40 biting in steps 1, 3, 5 only: numpy float64 against torch.optim in float64, 1e-12 of max|p|"""
    mine, ref = R.py_run_numpy(rule, list(wds)), R.py_run_torch(rule, list(wds))
    assert [t["coef"] < 1.0 for t in mine] == [True, False, True, False, True]
    assert [r["norm"] > R.PY_MAX_NORM for r in ref] == [True, False, True, False, True]
    assert mine[-1]["counts"].tolist() == [5 if i not in A.PY_LAG else 3 for i in range(len(A.PY_SHAPES))]
    worst = 0.0
    for t, r in zip(mine, ref):
        for a, b in zip(t["p"], r["p"]):
            worst = max(worst, float(np.abs(a - b).max()) / float(np.abs(b).max()))
    print(f"[{R.NAMES[rule]}, wd {wds}] numpy restatement vs torch.optim (float64): worst {worst:.2e} of max|p|")
    assert worst <= 1e-12, worst


def test_fp32_scalar_rule_matches_exact_rule():
    """rule_f64 (what the arena cases use: scalars as the kernel receives them) is _exact (what the torch comparison used) once the
    scalars are fp32 values"""
    rng = np.random.Generator(np.random.PCG64(1))
    p, g, m, v = rng.normal(0, 0.02, 64), rng.normal(0, 1e-2, 64), rng.normal(0, 1e-3, 64), rng.uniform(1e-7, 1e-4, 64)
    for rule in R.RULES:
        h, a = R.tables(rule, [3e-2], [0.5], [3])
        sc = [float(x) for x in (h[0, 0], h[0, 1], h[0, 2], a[0, 0], a[0, 1])]
        b1, b2, eps = (float(np.float32(x)) for x in (R.B1, R.B2, R.HOT_EPS))
        one = R.rule_f64(rule, p, g, m, v, 0.2, *sc, R.B1, R.B2, R.HOT_EPS)
        two = R._exact(rule, p, g, m, v, 0.2, *sc, b1, b2, eps)
        for x, y in zip(one, two):
            assert x is None or np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------- 2. arena cases
@pytest.mark.parametrize("name", ["small", "medium", "arena"])
def test_layouts(name):
    base = R.layouts()[name]()
    assert base["n"] % 512 == 0 and base["ends"][-1] < base["n"] and (base["begins"] % 8 == 0).all()
    assert set(np.unique(base["flags"])) == {0.0, 1.0, 2.0} and base["flags"][-1] != 0
    assert (base["n"] > A.SWEEP) == (name == "arena") and base["n"] > 4 * A.CHUNK
    lo, hi = base["begins"], base["begins"] + base["sizes"] - 1
    assert ((lo // A.CHUNK) != (hi // A.CHUNK)).any()                       # a chunk boundary inside a parameter
    assert (np.diff(lo // A.CHUNK) == 0).sum() > 50                         # many parameters inside one chunk
    z = base["zero"]
    assert z >= 0 and base["flags"][z] != 0 and not base["p"][base["begins"][z]:base["ends"][z]].any()
    dead = np.repeat(base["flags"] == 0, np.diff(np.concatenate([base["begins"], [base["n"]]])))
    for k in ("p", "g", "m", "v"):
        assert (np.isnan(base[k]) == dead).all(), k
    for rule in R.RULES:
        for kind in ("hot", "agent"):
            c = R.with_rule(base, rule, kind)
            assert c["hyp"].dtype == np.float32 and c["aux"].dtype == np.float32 and c["aux"].shape == (len(c["sizes"]), 4)
            assert np.array_equal(c["hyp"][:, 3], base["flags"]) and not c["aux"][:, 2:].any()
            if kind == "hot":                      # adjacent rows never share lr (the last row's neighbour in shifted() is row 0)
                assert (c["hyp"][:, 0] != np.roll(c["hyp"][:, 0], -1)).all()
                assert (c["hyp"][:, 2] > 0).all() and len(np.unique(c["hyp"][:, 2])) == 2
                if R.HAS_M[rule]:
                    assert (c["aux"][:, 0] != np.roll(c["aux"][:, 0], -1)).all() and len(np.unique(c["t"])) == 10
            else:
                assert set(np.unique(c["t"])) == {1, 7, 1000} and c["eps"] == 1e-8
                assert np.allclose(c["hyp"][:, 0], 1e-5) and np.allclose(c["hyp"][:, 2], 1e-2)
            if not R.HAS_M[rule]:
                assert np.array_equal(c["hyp"][:, 1], c["hyp"][:, 0]) and (c["aux"][:, 0] == 1).all()


def _cases():
    """(layout, rule): small and medium for every rule, the sweep-sized arena for ADAMW only"""
    return [(n, r) for n in ("small", "medium") for r in R.RULES] + [("arena", R.ADAMW)]


# ---------------------------------------------------------------------------------------------- 3. headroom
@pytest.mark.parametrize("kind", ["hot", "agent"])
@pytest.mark.parametrize("name,rule", _cases(), ids=lambda x: R.NAMES.get(x, x) if isinstance(x, int) else x)
def test_fp32_arithmetic_has_headroom(name, rule, kind):
    """optim_one's operations in numpy float32 against the float64 restatement: at least 4 x inside the bound on every tensor, at the
    exaggerated hyper-parameters of the sensitivity tests and at the agents' real ones (lr 1e-5, eps 1e-8, wd 1e-2, t in {1, 7, 1000})"""
    c = R.with_rule(R.layouts()[name](), rule, kind)
    ref, got = R.restate(c, COEF), R.emulate32(c, COEF)
    act = _active(c)
    for k in R.live_arrays(rule):
        err = A.tensor_max(c, got[k].astype(np.float64) - ref[k])[act]
        scale = np.maximum(A.tensor_max(c, ref[k])[act], 1e-30)
        worst = float((err / scale).max())
        print(f"[{R.NAMES[rule]} fp32 emulation, {name}, {kind}] {k}: worst per-tensor error {worst:.2e} of max|ref| (bound {R.TOL:g})")
        assert worst * 4 <= R.TOL, (k, worst)
    assert np.array_equal(got["g"].view(np.int32), ref["g"].astype(np.float32).view(np.int32))
    for k in set("mv") - set(R.live_arrays(rule)):         # an arena the rule does not own: never touched
        assert np.array_equal(ref[k].astype(np.float32).view(np.int32), c[k].view(np.int32))


# ---------------------------------------------------------------------------------------------- 4. sensitivity
def _moved(c, a, b):
    """per active tensor: max|a.p - b.p| over 20 x its tolerance in b (the criterion of test_adamw_ref)"""
    act = _active(c)
    d = A.tensor_max(c, a["p"] - b["p"])[act]
    tol = R.TOL * A.tensor_max(c, b["p"])[act]
    live = tol > 0                                  # (the all-zero tensor stays zero under every rule: tolerance 0)
    assert live.sum() == act.sum() - 1
    return float((d[live] / (20 * tol[live])).min())


MUTANTS = {R.ADAMW: ("decay_after", "hf_eps", "swap_decay", "no_a0"), R.ADAM: ("hf_eps", "swap_decay", "no_a0"),
           R.RMSPROP: ("eps_in_root",), R.SGD: ()}


@pytest.mark.parametrize("name,rule", _cases(), ids=lambda x: R.NAMES.get(x, x) if isinstance(x, int) else x)
def test_cases_are_sensitive(name, rule):
    c = R.with_rule(R.layouts()[name](), rule, "hot")
    ref = R.restate(c, COEF)
    moved = {v: _moved(c, R.restate(c, COEF, variant=v), ref) for v in MUTANTS[rule]}
    moved["neighbour's row"] = _moved(c, R.restate(R.shifted(c), COEF), ref)
    moved["clip dropped"] = _moved(c, R.restate(c, 1.0), ref)
    print(f"[{R.NAMES[rule]} case {name}] least movement over 20 x tolerance: " + ", ".join(f"{k} {v:.1f}" for k, v in moved.items()))
    for k, v in moved.items():
        assert v >= 1.0, (k, v)
    # what the GPU half compares bit for bit: untouched slots, gradient slots
    dead = np.isnan(c["p"])
    for k in ("p", "g", "m", "v"):
        assert np.array_equal(ref[k][dead].view(np.int64), c[k][dead].astype(np.float64).view(np.int64))
    f = np.repeat(c["flags"], np.diff(np.concatenate([c["begins"], [c["n"]]])))
    assert not ref["g"][f == 1].any() and np.array_equal(ref["g"][f == 2], c["g"][f == 2].astype(np.float64))
    keep = R.restate(c, COEF, zero_grad=0)
    assert np.array_equal(keep["g"][f != 0], c["g"][f != 0].astype(np.float64))


@pytest.mark.parametrize("rule", [R.ADAMW, R.ADAM], ids=lambda r: R.NAMES[r])
def test_python_case_step_counts_are_visible(rule):
    """the python-level schedule: parameters PY_LAG miss steps 2 and 3, so in steps 4 and 5 their own step count is 2 behind the global
    one; one step from the same state with the global count instead moves them by >= 20 x the bound.  (RMSprop and SGD have no t.)"""
    tr = R.py_run_numpy(rule)
    grads = R.py_case()["grads"]
    worst = np.inf
    for s in (3, 4):
        p0, m0, v0 = tr[s]["before"]
        for i in A.PY_LAG:
            assert tr[s]["used"][i] == s + 1 - 2
            g = grads[s][i].reshape(-1)
            own = R.py_update(rule, s, i, tr[s]["used"][i], p0[i], g, m0[i], v0[i], tr[s]["coef"])[0]
            glob = R.py_update(rule, s, i, s + 1, p0[i], g, m0[i], v0[i], tr[s]["coef"])[0]
            worst = min(worst, float(np.abs(own - glob).max()) / (20 * R.TOL * float(np.abs(own).max())))
    print(f"[{R.NAMES[rule]} python case] global instead of own step count: least movement over 20 x tolerance {worst:.1f}")
    assert worst >= 1.0, worst


@pytest.mark.parametrize("rule", R.RULES, ids=lambda r: R.NAMES[r])
def test_python_case_is_within_reach_of_fp32(rule):
    """the python-level schedule with the state kept in fp32 and the kernel's operation order (py_run_f32) against torch.optim in
    float64, after every step: 4 x inside the bound the GPU half applies on every tensor but the one-element one, which RMSprop takes
    from 0.03 to 0.008 -- its roundings were made at four times the magnitude its error is then measured against -- and which stays
    inside the bound itself."""
    ref, got = R.py_run_torch(rule), R.py_run_f32(rule)
    one = A.PY_SHAPES.index((1,))
    err = np.array([[float(np.abs(a.astype(np.float64) - b).max()) / float(np.abs(b).max()) for a, b in zip(g, r["p"])] for g, r in zip(got, ref)])
    print(f"[{R.NAMES[rule]} python case, fp32 emulation] worst per-tensor error after each step: " + ", ".join(f"{w:.2e}" for w in err.max(1)))
    assert np.delete(err, one, axis=1).max() * 4 <= R.TOL, err
    assert err[:, one].max() <= R.TOL, err[:, one]


@pytest.mark.parametrize("rule", R.RULES, ids=lambda r: R.NAMES[r])
def test_python_case_clip_and_decay_groups_are_visible(rule):
    """in the python-level schedule, dropping the clip (steps 1, 3, 5) or giving group 0 group 1's weight decay moves parameters by
    >= 20 x the bound"""
    ref = R.py_run_torch(rule)
    grads = R.py_case()["grads"]
    unclipped = R.py_run_torch(rule, grads=[[None if g is None else g / 1000.0 for g in gs] for gs in grads])     # same schedule, norm < 40
    assert all(r["norm"] < R.PY_MAX_NORM for r in unclipped)
    no_wd = R.py_run_torch(rule, wds=[0.0, 0.0])
    i = 0                                           # a group-0 GEMM weight with a gradient in every step
    d = float(np.abs(no_wd[-1]["p"][i] - ref[-1]["p"][i]).max()) / (20 * R.TOL * float(np.abs(ref[-1]["p"][i]).max()))
    assert d >= 1.0, d
    tr = R.py_run_numpy(rule)
    p0, m0, v0 = tr[2]["before"]
    g = grads[2][i].reshape(-1)
    a = R.py_update(rule, 2, i, 3, p0[i], g, m0[i], v0[i], tr[2]["coef"])[0]
    b = R.py_update(rule, 2, i, 3, p0[i], g, m0[i], v0[i], 1.0)[0]
    assert tr[2]["coef"] < 1.0
    assert float(np.abs(a - b).max()) >= 20 * R.TOL * float(np.abs(a).max())


# ---------------------------------------------------------------------------------------------- 5. host-side pieces
def _classes():
    from vln_hamt_amd.optim import TorchAdam, TorchAdamW, TorchRMSprop, TorchSGD
    return {R.ADAMW: TorchAdamW, R.ADAM: TorchAdam, R.RMSPROP: TorchRMSprop, R.SGD: TorchSGD}


def _params():
    return [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(3))]


def test_constructor_defaults_are_torchs():
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd.optim import AdamW, ArenaOptimizer
    for rule, cls in _classes().items():
        kw = dict(lr=0.1) if rule == R.SGD else {}
        mine, ref = cls(_params(), **kw), R.torch_class(rule)(_params(), **kw)
        assert isinstance(mine, ArenaOptimizer) and not isinstance(mine, AdamW) and mine.rule == rule == getattr(L, "OPT_" + R.NAMES[rule].upper())
        assert mine.defaults == ref.defaults
        a, b = mine.state_dict(), ref.state_dict()
        assert a["param_groups"] == b["param_groups"] and a["state"] == {} == b["state"]
    with pytest.raises(TypeError):
        _classes()[R.SGD](_params())                # lr is required, as the issue's signature says


@pytest.mark.parametrize("rule,option,value", [(R.ADAMW, "amsgrad", True), (R.ADAMW, "maximize", True), (R.ADAM, "amsgrad", True),
                                               (R.ADAM, "maximize", True), (R.RMSPROP, "momentum", 0.9), (R.RMSPROP, "centered", True),
                                               (R.RMSPROP, "maximize", True), (R.SGD, "momentum", 0.9), (R.SGD, "nesterov", True),
                                               (R.SGD, "dampening", 0.1), (R.SGD, "maximize", True)])
def test_constructor_refuses_what_the_kernel_lacks(rule, option, value):
    kw = dict(lr=0.1)
    kw[option] = value
    with pytest.raises(ValueError, match=option):
        _classes()[rule](_params(), **kw)


def test_constructor_keeps_torchs_own_checks():
    cls = _classes()
    with pytest.raises(ValueError):
        cls[R.ADAMW](_params(), lr=-1.0)
    with pytest.raises(ValueError):
        cls[R.ADAM](_params(), betas=(1.0, 0.999))
    with pytest.raises(ValueError):
        cls[R.RMSPROP](_params(), alpha=-0.1)
    with pytest.raises(ValueError):
        cls[R.SGD](_params(), lr=0.1, weight_decay=-1.0)


def test_host_tables_are_float64_rounded_once():
    """host_table()'s columns for given step counts, without a device: the entries of _torch_optim_ref.tables"""
    for rule, cls in _classes().items():
        o = cls([dict(params=_params()[:1], weight_decay=0.3), dict(params=_params()[1:], weight_decay=0.0, lr=0.02)], lr=0.05)
        o._built = True                              # (the arenas are not needed for the table)
        o._params = [p for g in o.param_groups for p in g["params"]]
        o._gidx_np = np.array([0, 1])
        o._keep = np.array([2.0, 1.0], dtype=np.float32)
        o._steps = np.array([6, 999], dtype=np.int64)
        tab = o.host_table(active=[True, True])
        assert o._steps.tolist() == [7, 1000] and tab.shape == (2, 2, 4) and tab.dtype == np.float32
        kw = o.param_groups[0]
        b1, b2 = kw.get("betas", (0.0, kw.get("alpha", 0.0)))
        h3, aux = R.tables(rule, [0.05, 0.02], [0.3, 0.0], [7, 1000], b1, b2)
        assert np.array_equal(tab[0, :, :3], h3) and np.array_equal(tab[1], aux) and tab[0, :, 3].tolist() == [2.0, 1.0]
        again = o.host_table(active=[True, False], advance=False)
        assert o._steps.tolist() == [7, 1000] and again[0, :, 3].tolist() == [2.0, 0.0]


def test_state_entries_have_torchs_layout():
    """a stepped parameter's state entry (arenas faked on the CPU) against what the installed torch writes after one step; SGD keeps
    {'momentum_buffer': None}, the layout of the reference's torch version"""
    for rule, cls in _classes().items():
        p = torch.nn.Parameter(torch.ones(4, 3))
        o = cls([p], lr=0.1)
        o._steps = np.array([3], dtype=np.int64)
        o._flat_m = torch.arange(16.0) if R.HAS_M[rule] else None
        o._flat_v = torch.arange(16.0) * 2 if R.HAS_V[rule] else None
        st = o._state_of(0, p, 2)
        q = torch.nn.Parameter(torch.ones(4, 3))
        ref = R.torch_class(rule)([q], lr=0.1)
        q.grad = torch.ones(4, 3)
        ref.step()
        want = ref.state_dict()["state"].get(0, {})
        if rule == R.SGD:
            assert st == {"momentum_buffer": None} and want in ({}, {"momentum_buffer": None})
            continue
        assert list(st) == list(want)
        assert st["step"].dtype == want["step"].dtype == torch.float32 and st["step"].dim() == 0 and st["step"].device.type == "cpu"
        assert float(st["step"]) == 3.0
        for k in st:
            assert st[k].shape == want[k].shape and st[k].dtype == want[k].dtype, k
        last = "exp_avg_sq" if R.HAS_M[rule] else "square_avg"
        assert torch.equal(st[last].reshape(-1), torch.arange(2.0, 14.0) * 2)
        if R.HAS_M[rule]:
            assert torch.equal(st["exp_avg"].reshape(-1), torch.arange(2.0, 14.0))


def test_update_bytes_per_rule():
    """34 / 34 / 26 / 18 bytes per element where the gradient slot is zeroed, 4 fewer where it is left to its producer (layout faked on
    the CPU); `moments` asks for another rule's count over the same arena, `active` for a subset"""
    for rule, cls in _classes().items():
        o = cls(_params(), lr=0.1)
        o._built = True
        o._ends = torch.tensor([16, 512], dtype=torch.int32)
        o._keep = np.array([2.0, 1.0], dtype=np.float32)
        per = {R.ADAMW: 34, R.ADAM: 34, R.RMSPROP: 26, R.SGD: 18}[rule]
        assert o.update_bytes() == 16 * (per - 4) + 496 * per
        assert o.update_bytes(active=[False, True]) == 496 * per
        assert o.update_bytes(moments=0) == 16 * 14 + 496 * 18 and o.update_bytes(moments=2) == 16 * 30 + 496 * 34


def test_exchange_choice_and_attach():
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd import parallel
    from vln_hamt_amd.optim import AdamW, ArenaOptimizer, Ralamb, RangerLars
    assert not parallel.per_tensor_update(AdamW(_params()))
    assert parallel.per_tensor_update(Ralamb(_params())) and parallel.per_tensor_update(RangerLars(_params()))
    # the seven public classes: each an ArenaOptimizer, none a subclass of another rule's class but RangerLars(Ralamb); only AdamW's
    # update has a range form, and every other class refuses attach() with its own reason
    assert AdamW.owned_slice_update and AdamW.attach is not ArenaOptimizer.attach
    for cls in (Ralamb, RangerLars, *_classes().values()):
        o = cls(_params(), lr=0.1)
        assert isinstance(o, ArenaOptimizer) and not isinstance(o, AdamW) and not o.owned_slice_update
        assert isinstance(o, Ralamb) == (cls in (Ralamb, RangerLars))
        reason = "trust ratio needs its whole norm" if isinstance(o, Ralamb) else "hamt_optim_table has no range form"
        with pytest.raises(L.HamtError, match=f"{cls.__name__}: .*attach / overlap_update.*{reason}"):
            o.attach(torch.nn.Linear(2, 2))
    assert issubclass(AdamW, ArenaOptimizer)
    for rule, cls in _classes().items():
        o = cls(_params(), lr=0.1)
        assert parallel.per_tensor_update(o) and not o.owned_slice_update
        with pytest.raises(L.HamtError, match="range form"):
            o.attach(torch.nn.Linear(2, 2))
        with pytest.raises(ValueError, match="OverlappedGradSync"):
            parallel.ShardedGradSync(o)


def test_build_agent_optimizers_mapping_and_refusals():
    from vln_hamt_amd.agent import AgentOptimizers, build_agent_optimizers
    cls = _classes()
    vln_bert, critic = torch.nn.Linear(4, 3), torch.nn.Linear(3, 1)
    for name, rule in (("rms", R.RMSPROP), ("adam", R.ADAM), ("adamW", R.ADAMW), ("sgd", R.SGD)):
        ao = build_agent_optimizers(types.SimpleNamespace(optim=name, lr=1e-5), vln_bert, critic)
        assert isinstance(ao, AgentOptimizers) and ao.optimizers == (ao.vln_bert_optimizer, ao.critic_optimizer)
        ref = R.torch_class(rule)(vln_bert.parameters(), lr=1e-5)
        for o, model in zip(ao.optimizers, (vln_bert, critic)):
            assert type(o) is cls[rule] and len(o.param_groups) == 1
            assert [id(p) for p in o.param_groups[0]["params"]] == [id(p) for p in model.parameters()]
            assert {k: v for k, v in o.param_groups[0].items() if k != "params"} == {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    for bad in ("adamw", "AdamW", "rmsprop", "ranger", "", None):
        with pytest.raises(AssertionError):
            build_agent_optimizers(types.SimpleNamespace(optim=bad, lr=1e-5), vln_bert, critic)


def test_optim_kernels_do_not_spill(tmp_path):
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
            if not name or "optim_table_kernel" not in name.group(1):
                continue
            seen[name.group(1)] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                                   int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                                   int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert len(seen) == 4, seen                     # one instantiation per rule
    assert all(v == (0, 0, 0) for v in seen.values()), seen
