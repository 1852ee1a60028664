"""Plain numpy float64 restatement of torch.optim's AdamW / Adam / RMSprop (momentum 0, not centered) / SGD (momentum 0) -- the rules of
hamt_optim_table -- and the synthetic cases of its op-level tests, built on the arena layouts of tests/_adamw_ref.py (the new kernel keeps
adamw_table_kernel's sweep and segment walk).  test_torch_optim_ref.py proves on the CPU that the restatement IS torch's arithmetic and that
the cases can tell a wrong kernel from a right one; test_gpu_torch_optim.py runs the kernel and the optimisers on them.  Nothing here touches
the GPU or the package under test."""
import functools

import numpy as np

import _adamw_ref as A

TOL = A.TOL
ADAMW, ADAM, RMSPROP, SGD = 0, 1, 2, 3            # hamt_opt_rule
RULES = (ADAMW, ADAM, RMSPROP, SGD)
NAMES = {ADAMW: "adamw", ADAM: "adam", RMSPROP: "rmsprop", SGD: "sgd"}
HAS_M = {ADAMW: True, ADAM: True, RMSPROP: False, SGD: False}
HAS_V = {ADAMW: True, ADAM: True, RMSPROP: True, SGD: False}
B1, B2 = 0.9, 0.98                                # (RMSprop: B2 is its alpha)
HOT_EPS = 3e-3                                    # of the size of sqrt(v) in the cases (v in [1e-7, 1e-4], g ~ 1e-2)


# ---------------------------------------------------------------------------------------------- the rules
def rule_f64(rule, p, g, m, v, coef, lr, step, wd, a0, a1, b1, b2, eps, variant=None):
    """one update in float64; arrays are fp32 values widened, scalars (or per-element arrays) the fp32 values the kernel receives:
    step = lr / (1 - b1^t), a0 = 1 / sqrt(1 - b2^t), a1 = 1 - lr * wd.  `variant` names a deliberate mistake (the sensitivity tests)."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    m = None if m is None else np.asarray(m, dtype=np.float64)
    v = None if v is None else np.asarray(v, dtype=np.float64)
    b1, b2, eps = (float(np.float32(x)) for x in (b1, b2, eps))
    gg = g * coef
    decoupled = rule == ADAMW
    if variant == "swap_decay":
        decoupled = not decoupled
    if variant == "no_a0":
        a0 = 1.0
    if decoupled and variant != "decay_after":
        p = p * a1
    if not decoupled:
        gg = gg + wd * p
    if rule in (ADAMW, ADAM):
        m = b1 * m + (1.0 - b1) * gg
        v = b2 * v + (1.0 - b2) * gg * gg
        if variant == "hf_eps":                   # HF's placement: the bias correction folded into the step, eps next to the raw root
            p = p - (step / a0) * m / (np.sqrt(v) + eps)
        else:
            p = p - step * m / (np.sqrt(v) * a0 + eps)
        if decoupled and variant == "decay_after":
            p = p * a1
    elif rule == RMSPROP:
        v = b2 * v + (1.0 - b2) * gg * gg
        p = p - lr * gg / (np.sqrt(v + eps) if variant == "eps_in_root" else np.sqrt(v) + eps)
    else:
        p = p - lr * gg
    return p, m, v


def rule_f32(rule, p, g, m, v, coef, lr, step, wd, a0, a1, b1, b2, eps):
    """the kernel's optim_one in numpy float32, same operation order (no fused multiply-add)"""
    f = np.float32
    p, g, lr, step, wd, a0, a1 = (np.asarray(a, dtype=f) for a in (p, g, lr, step, wd, a0, a1))
    m = None if m is None else np.asarray(m, dtype=f)
    v = None if v is None else np.asarray(v, dtype=f)
    coef, b1, b2, eps, one = f(coef), f(b1), f(b2), f(eps), f(1.0)
    gg = g * coef
    if rule == ADAMW:
        p = p * a1
    else:
        gg = gg + wd * p
    if rule in (ADAMW, ADAM):
        m = m * b1 + (one - b1) * gg
        v = v * b2 + (one - b2) * gg * gg
        p = p - step * (m / (np.sqrt(v) * a0 + eps))
    elif rule == RMSPROP:
        v = v * b2 + (one - b2) * gg * gg
        p = p - lr * (gg / (np.sqrt(v) + eps))
    else:
        p = p - lr * gg
    return p, m, v


# ---------------------------------------------------------------------------------------------- arena cases
def tables(rule, lr, wd, t, b1=B1, b2=B2):
    """the fp32 {lr, step, wd} and {a0, a1} columns the host forms in float64 and rounds once (optim.torch_rules.host_table); the bias
    corrections are those of the betas the kernel receives (floats), so that its moments and their corrections belong together"""
    lr, wd, t = (np.asarray(a, dtype=np.float64) for a in (lr, wd, t))
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    if rule in (ADAMW, ADAM):
        step, a0 = lr / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)
    else:
        step, a0 = lr, np.ones_like(lr)
    a1 = 1.0 - lr * wd
    return np.stack([lr, step, wd], 1).astype(np.float32), np.stack([a0, a1, 0 * a0, 0 * a0], 1).astype(np.float32)


def with_rule(case, rule, kind="hot", eps=None):
    """an _adamw_ref arena case (layout, flags and values shared, never written) with this rule's tables.
    hot:   lr alternates 3e-2 / 1e-1 from row to row (last row: 6e-2), wd 0.1 / 0.5 every two rows, t = 1 + row % 9 (last row: 10), eps = HOT_EPS
           -- exaggerated, so that
           every mistake of the sensitivity tests is far above the fp32 bound (at the agent's values most are far below it);
    agent: lr 1e-5, wd 1e-2, eps 1e-8, torch's default betas / alpha, t cycling through 1, 7, 1000 -- the finetune recipes' real values."""
    idx = np.arange(len(case["sizes"]))
    if kind == "hot":
        lr, wd, t = np.where(idx % 2 == 0, 3e-2, 1e-1), np.where((idx // 2) % 2 == 0, 0.1, 0.5), 1 + idx % 9
        lr[-1] = 6e-2                             # (the last row's neighbour in shifted() is row 0: whatever the row count, they differ)
        t[-1] = 10
        eps = HOT_EPS if eps is None else eps
    else:
        lr, wd, t = np.full(len(idx), 1e-5), np.full(len(idx), 1e-2), np.array([1, 7, 1000])[idx % 3]
        eps = 1e-8 if eps is None else eps
    b1, b2 = (B1, B2) if kind == "hot" else (0.9, 0.99 if rule == RMSPROP else 0.999)          # agent: torch's defaults
    c = dict(case)
    h3, c["aux"] = tables(rule, lr, wd, t, b1, b2)
    c["hyp"] = np.concatenate([h3, case["flags"].astype(np.float32)[:, None]], 1)
    c["rule"], c["t"], c["eps"], c["b1"], c["b2"] = rule, t, eps, b1, b2
    return c


@functools.lru_cache(maxsize=None)
def medium_case(seed=7):
    """the tail of _adamw_ref.make_case's layout as an arena of its own (~620 000 floats, ~150 chunks): the last 200 tiny tensors and
    every MEDIUM one -- tensors that span many chunks, a cut inside a parameter at most chunk boundaries, the table's last row active"""
    c = A.make_case()
    nt = len(c["sizes"])
    m = A.cut_case(c, nt - len(A.MEDIUM) - 200, nt, seed)
    assert m["flags"][-1] != 0 and 600000 < m["n"] < 700000
    return m


def layouts():
    """name -> arena case, smallest first; 'arena' (more than one grid sweep) is needed for one rule only"""
    return {"small": A.small_case, "medium": medium_case, "arena": A.make_case}


def _per_element(case):
    n, begins = case["n"], case["begins"]
    reps = np.diff(np.concatenate([begins, [n]]))
    return [np.repeat(case["hyp"][:, k], reps) for k in range(4)] + [np.repeat(case["aux"][:, k], reps) for k in range(2)]


def _apply(case, coef, zero_grad, dtype, variant=None):
    rule = case["rule"]
    lr, step, wd, flag, a0, a1 = _per_element(case)
    act = flag != 0
    out = {k: case[k].astype(dtype) for k in ("p", "g", "m", "v")}          # (m / v of a rule that does not own them: returned unchanged)
    sel = lambda a: a[act].astype(dtype)
    args = (case["p"][act], case["g"][act], case["m"][act] if HAS_M[rule] else None, case["v"][act] if HAS_V[rule] else None, coef,
            sel(lr), sel(step), sel(wd), sel(a0), sel(a1), case["b1"], case["b2"], case["eps"])
    with np.errstate(invalid="ignore"):
        p, m, v = rule_f64(rule, *args, variant=variant) if dtype == np.float64 else rule_f32(rule, *args)
    out["p"][act] = p
    if HAS_M[rule]:
        out["m"][act] = m
    if HAS_V[rule]:
        out["v"][act] = v
    if zero_grad:
        out["g"][flag == 1] = 0
    return out


def restate(case, coef, zero_grad=1, variant=None):
    """float64 over an arena case: flag-0 tensors are left alone; the gradient becomes 0 where the flag is 1 and zero_grad is set"""
    return _apply(case, float(coef), zero_grad, np.float64, variant)


def emulate32(case, coef, zero_grad=1):
    return _apply(case, np.float32(coef), zero_grad, np.float32)


def shifted(case):
    """the same case with every tensor given the NEXT row's hyp / aux entries (the last one: the first row's)"""
    c = dict(case)
    c["hyp"] = case["hyp"].copy()
    c["hyp"][:, :3] = np.roll(case["hyp"][:, :3], -1, axis=0)
    c["aux"] = np.roll(case["aux"], -1, axis=0)
    return c


def live_arrays(rule):
    return ("p",) + (("m",) if HAS_M[rule] else ()) + (("v",) if HAS_V[rule] else ())


# ---------------------------------------------------------------------------------------------- the python-level schedule
# _adamw_ref's shapes, groups, learning rates and lagging parameters; gradients 40 x its own, so that their norm (~ 76 in steps 1, 3, 5,
# ~ 7.6 in steps 2, 4) lies on both sides of the agents' max_norm of 40; torch's default eps and betas
PY_MAX_NORM = 40.0
PY_WD = [0.05, 0.0]                               # per group.  (Not larger: with L2 decay, wd * p near g * coef cancels in some element, and
                                                  # RMSprop's first step, lr * gg / (sqrt(0.01 gg^2) + 1e-8), turns that element's fp32 rounding
                                                  # into 1e-5 of max|p| at wd 0.3 -- the case would test the conditioning, not the kernel.)
PY_DEFAULTS = {ADAMW: dict(betas=(0.9, 0.999), eps=1e-8), ADAM: dict(betas=(0.9, 0.999), eps=1e-8), RMSPROP: dict(alpha=0.99, eps=1e-8), SGD: {}}


@functools.lru_cache(maxsize=None)
def py_case():
    c = A.py_case()
    grads = [[None if g is None else (g * np.float32(40.0)).astype(np.float32) for g in gs] for gs in c["grads"]]
    return dict(init=c["init"], grads=grads)


def py_coef(grads, max_norm=PY_MAX_NORM):
    gsq = sum(float((g.astype(np.float64) ** 2).sum()) for g in grads if g is not None)
    return A.clip_coef(gsq, max_norm), gsq


def py_run_numpy(rule, wds=PY_WD, per_parameter=True, steps=5):
    """the schedule through rule_f64 with float64 state and float64 scalars (torch's Python scalars); returns per step the parameters
    after it, the state before it and the step counts used"""
    c = py_case()
    kw = PY_DEFAULTS[rule]
    b1, b2 = kw.get("betas", (0.0, kw.get("alpha", 0.0)))
    eps = kw.get("eps", 0.0)
    p = [a.astype(np.float64).reshape(-1) for a in c["init"]]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    counts = np.zeros(len(p), dtype=np.int64)
    trace = []
    for s, grads in enumerate(c["grads"][:steps]):
        coef, _ = py_coef(grads)
        before = ([a.copy() for a in p], [a.copy() for a in m], [a.copy() for a in v])
        used = {}
        for i, g in enumerate(grads):
            if g is None:
                continue
            counts[i] += 1
            t = used[i] = int(counts[i]) if per_parameter else s + 1
            p[i], m[i], v[i] = py_update(rule, s, i, t, p[i], g.reshape(-1), m[i], v[i], coef, wds)
        trace.append(dict(before=before, used=used, coef=coef, p=[a.copy() for a in p], counts=counts.copy()))
    return trace


def py_run_f32(rule, wds=PY_WD, steps=5):
    """the schedule as the optimiser runs it: state kept in fp32, the table entries of `tables`, rule_f32's operation order; returns
    the parameters after every step"""
    c = py_case()
    kw = PY_DEFAULTS[rule]
    b1, b2 = kw.get("betas", (0.0, kw.get("alpha", 0.0)))
    p = [a.reshape(-1).copy() for a in c["init"]]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    counts = np.zeros(len(p), dtype=np.int64)
    out = []
    for s, grads in enumerate(c["grads"][:steps]):
        coef, _ = py_coef(grads)
        for i, g in enumerate(grads):
            if g is None:
                continue
            counts[i] += 1
            h, a = tables(rule, [A.PY_LR[s][A.PY_GROUP[i]]], [wds[A.PY_GROUP[i]]], [counts[i]], b1, b2)
            p[i], mi, vi = rule_f32(rule, p[i], g.reshape(-1), m[i], v[i], coef, h[0, 0], h[0, 1], h[0, 2], a[0, 0], a[0, 1], b1, b2,
                                    kw.get("eps", 0.0))
            m[i], v[i] = (m[i] if mi is None else mi), (v[i] if vi is None else vi)
        out.append([a.copy() for a in p])
    return out


def py_update(rule, s, i, t, p, g, m, v, coef, wds=PY_WD):
    kw = PY_DEFAULTS[rule]
    b1, b2 = kw.get("betas", (0.0, kw.get("alpha", 0.0)))
    lr, wd = A.PY_LR[s][A.PY_GROUP[i]], wds[A.PY_GROUP[i]]
    if rule in (ADAMW, ADAM):
        step, a0 = lr / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)
    else:
        step, a0 = lr, 1.0
    return _exact(rule, p, g, m, v, coef, lr, step, wd, a0, 1.0 - lr * wd, b1, b2, kw.get("eps", 0.0))


def _exact(rule, p, g, m, v, coef, lr, step, wd, a0, a1, b1, b2, eps):
    """rule_f64 with the scalars as they are (no rounding to fp32): torch in float64"""
    gg = np.asarray(g, dtype=np.float64) * coef
    if rule == ADAMW:
        p = p * a1
    else:
        gg = gg + wd * p
    if rule in (ADAMW, ADAM):
        m = b1 * m + (1.0 - b1) * gg
        v = b2 * v + (1.0 - b2) * gg * gg
        p = p - step * m / (np.sqrt(v) * a0 + eps)
    elif rule == RMSPROP:
        v = b2 * v + (1.0 - b2) * gg * gg
        p = p - lr * gg / (np.sqrt(v) + eps)
    else:
        p = p - lr * gg
    return p, m, v


def torch_class(rule):
    import torch
    return {ADAMW: torch.optim.AdamW, ADAM: torch.optim.Adam, RMSPROP: torch.optim.RMSprop, SGD: torch.optim.SGD}[rule]


def py_run_torch(rule, wds=PY_WD, steps=5, grads=None):
    """the schedule through torch.optim on the CPU in float64, with torch.nn.utils.clip_grad_norm_ at PY_MAX_NORM; returns per step the
    parameters after it and the norm clip_grad_norm_ returned.  `grads`: per step a list of arrays / None to use instead of py_case's."""
    import torch
    c = py_case()
    ps = [torch.nn.Parameter(torch.from_numpy(a.astype(np.float64))) for a in c["init"]]
    groups = [dict(params=[p for p, gi in zip(ps, A.PY_GROUP) if gi == k], weight_decay=wds[k], lr=A.PY_LR[0][k]) for k in (0, 1)]
    opt = torch_class(rule)(groups, **PY_DEFAULTS[rule])
    out = []
    for s, gs in enumerate((grads or c["grads"])[:steps]):
        for k in (0, 1):
            opt.param_groups[k]["lr"] = A.PY_LR[s][k]
        for p, g in zip(ps, gs):
            p.grad = None if g is None else torch.from_numpy(np.asarray(g, dtype=np.float64).reshape(p.shape).copy())
        norm = float(torch.nn.utils.clip_grad_norm_(ps, PY_MAX_NORM))
        opt.step()
        out.append(dict(p=[p.detach().numpy().reshape(-1).copy() for p in ps], norm=norm))
    return out
