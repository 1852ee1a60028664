"""-m gpu: the AdamW, gradient-norm and clip kernels of csrc/optim.hip at op level against the float64 restatement of tests/_adamw_ref.py
(tests/test_adamw_ref.py shows on the CPU that the cases tell a wrong kernel from a right one):
  A  hamt_adamw_table over an arena of more than one grid sweep, chunks that hold dozens of parameters, flags 0 / 1 / 2;
  B  hamt_adamw_table_range: ranges that start and end inside parameters, their union == the one-launch result, bit for bit;
  C  hamt_adamw_flat: tails and the grid-stride loop;
  D  hamt_sumsq, hamt_sumsq_partials, hamt_clip_scale and the generic clip_grad_norm_ path;
  E  optim.AdamW on bare parameters over five steps with lagging per-parameter step counts."""
import math

import numpy as np
import pytest
import torch

import _adamw_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 1024                      # elements behind every array that no launch may touch
CANARY_VALUE = 1234.5
KEYS = ("p", "g", "m", "v", "p16")


def _lib():
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd.ops import _p, _stream
    return L, _p, _stream


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def with_canary(a, dtype=torch.float32):
    """`a` (numpy fp32) on the device with CANARY elements behind it"""
    t = torch.full((a.size + CANARY,), CANARY_VALUE, dtype=dtype, device=DEV)
    t[:a.size] = torch.from_numpy(a).to(DEV).to(dtype)
    return t


def nan_shadow(n):
    """a bf16 array of n NaNs + the canary"""
    t = torch.full((n + CANARY,), CANARY_VALUE, dtype=torch.bfloat16, device=DEV)
    t[:n] = float("nan")
    return t


def arena_init(c):
    d = {k: with_canary(c[k]) for k in ("p", "g", "m", "v")}
    d["p16"] = nan_shadow(c["n"])
    return d


def launch_table(c, d, gsq, max_norm, zero_grad=1, p16=True, first=0, n=None):
    """hamt_adamw_table (first == 0 and n None) or hamt_adamw_table_range with the pointers advanced by `first`"""
    L, _p, _stream = _lib()
    ends = torch.from_numpy(c["ends"].astype(np.int32)).to(DEV)
    hyp = torch.from_numpy(c["hyp"]).to(DEV)
    gn = None if gsq is None else torch.tensor([gsq], dtype=torch.float32, device=DEV)
    args = [_p(d[k][first:]) for k in ("p", "g", "m", "v")] + [_p(d["p16"][first:]) if p16 else None, _p(ends), _p(hyp), len(c["ends"]), _p(gn),
                                                              float(max_norm), c["b1"], c["b2"], c["eps"], int(zero_grad), _stream()]
    if n is None:
        L.check(L.load().hamt_adamw_table(c["n"], *args), "hamt_adamw_table")
    else:
        L.check(L.load().hamt_adamw_table_range(first, n, *args), "hamt_adamw_table_range")
    torch.cuda.synchronize()


def check_table(c, init, out, want, zero_grad=1, p16=True):
    """`out` against the float64 restatement `want` and the bit rules of every array"""
    n = c["n"]
    flag = torch.from_numpy(np.repeat(c["flags"], np.diff(np.concatenate([c["begins"], [n]])))).to(DEV)
    live, act = flag != 0, c["flags"] != 0
    for k in ("p", "m", "v"):
        got = out[k][:n].cpu().numpy().astype(np.float64)
        err = R.tensor_max(c, got - want[k])[act]
        scale = np.maximum(R.tensor_max(c, want[k])[act], 1e-30)
        i = int(np.argmax(err / scale))
        print(f"[adamw table, {len(c['ends'])} rows] {k}: worst per-tensor error {err[i] / scale[i]:.2e} of max|ref|")
        assert (err <= R.TOL * scale).all(), (k, int(np.flatnonzero(act)[i]), err[i] / scale[i])
        assert not np.isnan(got[act.repeat(np.diff(np.concatenate([c["begins"], [n]])))]).any(), k
    for k in KEYS:                                   # no gradient: untouched, bit for bit, whatever the slots hold; and the canary
        assert same_bits(out[k][:n][~live], init[k][:n][~live]), k
        assert same_bits(out[k][n:], init[k][n:]), k
    if p16:                                          # the shadow of the FINAL value
        assert same_bits(out["p16"][:n][live], out["p"][:n].to(torch.bfloat16)[live])
    else:
        assert same_bits(out["p16"], init["p16"])
    zeroed = (flag == 1) if zero_grad else torch.zeros_like(live)
    assert not bits(out["g"][:n][zeroed]).any()
    assert same_bits(out["g"][:n][~zeroed], init["g"][:n][~zeroed])
    pad = slice(int(c["ends"][-1]), n)               # behind the last tensor: the last row's hyper-parameters on zeros
    for k in ("p", "m", "v"):
        assert torch.isfinite(out[k][pad]).all(), k


GSQ, MAX_NORM = 25.0, 1.0                            # clip coefficient 1 / (5 + 1e-6) < 1


@pytest.fixture(scope="module")
def whole():
    """test A's launch, once: the case, its inputs and the kernel's outputs (host tensors, canary included); dropped with the module"""
    c = R.make_case()
    d = arena_init(c)
    init = {k: t.cpu() for k, t in d.items()}
    launch_table(c, d, GSQ, MAX_NORM)
    yield c, init, {k: t.cpu() for k, t in d.items()}
    R.make_case.cache_clear()
    R.small_case.cache_clear()


def test_adamw_table_vs_float64(whole):
    c, init, out = whole
    assert c["n"] > R.SWEEP
    want = R.restate(c, R.clip_coef(float(np.float32(GSQ)), MAX_NORM))
    check_table(c, {k: t.to(DEV) for k, t in init.items()}, {k: t.to(DEV) for k, t in out.items()}, want)
    d = {k: t.to(DEV) for k, t in init.items()}      # a second launch from the same inputs: bit-identical
    launch_table(c, d, GSQ, MAX_NORM)
    for k in KEYS:
        assert same_bits(d[k].cpu(), out[k]), k


@pytest.mark.parametrize("variant", ["keep_grad", "no_shadow", "no_norm", "max_norm_0", "norm_below", "eps_1e-8"])
def test_adamw_table_variants(variant):
    c = R.small_case()
    gsq, max_norm, zero_grad, p16 = GSQ, MAX_NORM, 1, True
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
    elif variant == "eps_1e-8":
        c = dict(c, eps=1e-8)
    coef = R.clip_coef(gsq, max_norm)
    assert (coef == 1.0) == (variant in ("no_norm", "max_norm_0", "norm_below"))
    d = arena_init(c)
    init = {k: t.clone() for k, t in d.items()}
    launch_table(c, d, gsq, max_norm, zero_grad, p16)
    check_table(c, init, d, R.restate(c, coef, zero_grad), zero_grad, p16)


def test_adamw_table_range_union_is_the_whole(whole):
    """Ranges cut at multiples of 4 that are not multiples of 4 096, inside parameters (the large tensor, the tiny run), one at a
    parameter end, one range shorter than a chunk, one longer than a grid sweep; pointers advanced by `first` (launch_step_overlapped).
    After each call: inside the range == the one-launch result, outside untouched; so after all of them == the one-launch result."""
    c, init, out = whole
    b, e, n = c["begins"], c["ends"], c["n"]
    cuts = [0, 1028, int(b[2900]) + 4, int(e[2950]), int(b[2990]) + 4, n]
    assert all(x % 4 == 0 for x in cuts) and all(x % 4096 for x in cuts[1:-1])
    assert cuts[1] < e[0] and b[2900] < cuts[2] < b[2900] + c["sizes"][2900] and b[2990] < cuts[4] < b[2990] + c["sizes"][2990]
    assert cuts[2] - cuts[1] > R.SWEEP and cuts[4] - cuts[3] < R.CHUNK and cuts[1] + R.SWEEP < e[R.N_TINY]
    d = {k: t.to(DEV) for k, t in init.items()}
    expect = {k: t.to(DEV) for k, t in init.items()}
    res = {k: t.to(DEV) for k, t in out.items()}
    for first, last in zip(cuts[:-1], cuts[1:]):
        launch_table(c, d, GSQ, MAX_NORM, first=first, n=last - first)
        for k in KEYS:
            expect[k][first:last] = res[k][first:last]
            assert same_bits(d[k], expect[k]), (k, first, last)
    for k in KEYS:
        assert same_bits(d[k], res[k]), k


# ------------------------------------------------------------------------------------------------ C: hamt_adamw_flat
FLAT_N = [1, 2, 3, 5, 4099, 4_194_304 + 3075]       # the last: beyond 4 096 blocks x 256 threads x 4 (grid-stride loop) with a tail of 3
FLAT_CFG = [(0.05, 1, True, "clip"), (0.0, 0, False, "null"), (0.05, 0, False, "clip"), (0.0, 1, True, "max_norm_0")]


@pytest.mark.parametrize("cfg", range(len(FLAT_CFG)))
@pytest.mark.parametrize("n", FLAT_N)
def test_adamw_flat_vs_float64(n, cfg):
    L, _p, _stream = _lib()
    wd, zero_grad, p16, norm = FLAT_CFG[cfg]
    rng = np.random.Generator(np.random.PCG64(100 + cfg))
    a = dict(p=rng.normal(0, 0.02, n), g=rng.normal(0, 1e-2, n), m=rng.normal(0, 1e-3, n), v=rng.uniform(1e-7, 1e-4, n))
    a = {k: x.astype(np.float32) for k, x in a.items()}
    lr = np.float32(1e-2)
    step = np.float32(1e-2 * R.bias_correction(3))
    b1, b2, eps = R.B1, R.B2, 1e-6
    max_norm = 0.0 if norm == "max_norm_0" else 1.0
    d = {k: with_canary(x) for k, x in a.items()}
    d["p16"] = nan_shadow(n)
    init = {k: t.clone() for k, t in d.items()}
    hyper = torch.tensor([lr, step, max_norm], dtype=torch.float32, device=DEV)
    gn = None if norm == "null" else torch.tensor([GSQ], dtype=torch.float32, device=DEV)
    L.check(L.load().hamt_adamw_flat(n, _p(d["p"]), _p(d["g"]), _p(d["m"]), _p(d["v"]), _p(d["p16"]) if p16 else None, _p(hyper), _p(gn),
                                     b1, b2, eps, wd, zero_grad, _stream()), "hamt_adamw_flat")
    torch.cuda.synchronize()
    coef = R.clip_coef(GSQ, max_norm) if norm != "null" else 1.0
    assert (coef < 1.0) == (norm == "clip")
    want = R.adamw_f64(a["p"], a["g"], a["m"], a["v"], coef, float(lr), float(step), float(np.float32(wd)), b1, b2, eps)
    for k, ref in zip(("p", "m", "v"), want):
        got = d[k][:n].cpu().numpy().astype(np.float64)
        err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
        assert err <= R.TOL, (k, err)
    for k in KEYS:
        assert same_bits(d[k][n:], init[k][n:]), k
    if p16:
        assert same_bits(d["p16"][:n], d["p"][:n].to(torch.bfloat16))
    else:
        assert same_bits(d["p16"], init["p16"])
    if zero_grad:
        assert not bits(d["g"][:n]).any()
    else:
        assert same_bits(d["g"], init["g"])


# ------------------------------------------------------------------------------------------------ D: norm and clip
SUMSQ_TOL = 1e-5                                     # relative: the bound of test_sumsq_table_active_only
PRESET = 3.5


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 1_048_576 + 4098])      # the last: beyond the 1 024-block grid
def test_sumsq_vs_float64(n, accumulate):
    L, _p, _stream = _lib()
    g = np.random.Generator(np.random.PCG64(n)).normal(0, 1.0, n).astype(np.float32)
    dg = with_canary(g)
    dg[n:] = float("nan")                            # (reading behind n would poison the sum)
    out = torch.tensor([PRESET], dtype=torch.float32, device=DEV)
    ws = torch.zeros(1024, dtype=torch.float32, device=DEV)
    L.check(L.load().hamt_sumsq(n, _p(dg), _p(out), accumulate, _p(ws), _stream()), "hamt_sumsq")
    ref = float((g.astype(np.float64) ** 2).sum()) + (PRESET if accumulate else 0.0)
    assert abs(float(out) - ref) <= SUMSQ_TOL * ref, (float(out), ref)
    assert same_bits(dg[:n].cpu(), torch.from_numpy(g))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 4095, 4097, 18001])
def test_sumsq_partials_vs_float64(n, accumulate):
    L, _p, _stream = _lib()
    x = np.random.Generator(np.random.PCG64(n)).uniform(0, 1.0, n).astype(np.float32)
    dx = with_canary(x)
    dx[n:] = float("nan")
    got = []
    for _ in range(2):
        out = torch.tensor([PRESET], dtype=torch.float32, device=DEV)
        L.check(L.load().hamt_sumsq_partials(n, _p(dx), _p(out), accumulate, _stream()), "hamt_sumsq_partials")
        got.append(out.cpu())
    ref = float(x.astype(np.float64).sum()) + (PRESET if accumulate else 0.0)
    assert abs(float(got[0]) - ref) <= SUMSQ_TOL * ref, (float(got[0]), ref)
    assert same_bits(got[0], got[1])                 # a fixed order: bit-identical from launch to launch


@pytest.mark.parametrize("n", [1, 7, 1_048_576 + 5])                  # the last: beyond 4 096 blocks x 256 threads
def test_clip_scale_vs_float64(n):
    """|got - g * coef| <= 1e-6 |g| elementwise, coef in float64: four fp32 roundings (sqrt, add, divide, multiply) of at most 2^-24 each
    = 2.4e-7, 4 x inside the bound.  A norm below max_norm leaves the array bit-unchanged."""
    L, _p, _stream = _lib()
    g = np.random.Generator(np.random.PCG64(n)).normal(0, 1.0, n).astype(np.float32)
    for gsq, scaled in ((GSQ, True), (0.25, False)):
        dg = with_canary(g)
        init = dg.clone()
        gn = torch.tensor([gsq], dtype=torch.float32, device=DEV)
        L.check(L.load().hamt_clip_scale(n, _p(dg), _p(gn), MAX_NORM, _stream()), "hamt_clip_scale")
        torch.cuda.synchronize()
        assert same_bits(dg[n:], init[n:])
        coef = R.clip_coef(gsq, MAX_NORM)
        assert (coef < 1.0) == scaled
        if scaled:
            g64 = g.astype(np.float64)
            assert (np.abs(dg[:n].cpu().numpy().astype(np.float64) - g64 * coef) <= 1e-6 * np.abs(g64)).all()
        else:
            assert same_bits(dg, init)


def test_clip_grad_norm_generic_path():
    """clip_grad_norm_ on plain tensors that no optimizer owns; one gradient is a view at an 8-byte offset of a larger buffer (the
    clone-and-copy-back branch).  Against torch.nn.utils.clip_grad_norm_ on float64 copies: the norm to the sumsq bound; the scaled
    gradients to 6e-6 |ref| -- the coefficient max_norm / (sqrt(gsq) + 1e-6) inherits half the relative error of gsq (<= 1e-5, the sumsq
    bound: 5e-6) and the four roundings of test_clip_scale_vs_float64 (1e-6 with its margin)."""
    from vln_hamt_amd.optim import clip_grad_norm_
    gen = torch.Generator().manual_seed(3)
    shapes = [(33,), (4, 5), (1000,), (257, 3), (2,)]
    params = [torch.randn(s, generator=gen).to(DEV).requires_grad_(True) for s in shapes]
    grads = [torch.randn(s, generator=gen) for s in shapes]
    buf = torch.full((1000 + 64,), CANARY_VALUE, device=DEV)
    odd = 2
    for i, (p, g) in enumerate(zip(params, grads)):
        if i == odd:
            view = buf[2:2 + p.numel()]
            view.copy_(g)
            p.grad = view
            assert p.grad.data_ptr() % 16 == 8 and p.grad.data_ptr() == buf.data_ptr() + 8
        else:
            p.grad = g.to(DEV)
    ref_params = [torch.zeros(s, dtype=torch.float64).requires_grad_(True) for s in shapes]
    for p, g in zip(ref_params, grads):
        p.grad = g.double()
    max_norm = 5.0
    ref_norm = float(torch.nn.utils.clip_grad_norm_(ref_params, max_norm))
    assert ref_norm > 2 * max_norm
    gn = clip_grad_norm_(params, max_norm)
    assert abs(float(gn) - ref_norm) <= SUMSQ_TOL * ref_norm, (float(gn), ref_norm)
    for i, (p, q) in enumerate(zip(params, ref_params)):
        ref = q.grad
        assert ((p.grad.cpu().double() - ref).abs() <= 6e-6 * ref.abs()).all(), i
    assert params[odd].grad.data_ptr() == buf.data_ptr() + 8                     # scaled in place, through the copy back
    rest = torch.cat([buf[:2], buf[2 + params[odd].numel():]])
    assert same_bits(rest, torch.full_like(rest, CANARY_VALUE))                  # the neighbours in its buffer: untouched


# ------------------------------------------------------------------------------------------------ E: optim.AdamW, bare parameters
def test_adamw_python_steps_vs_float64():
    """Five steps of optim.AdamW on eight bare parameters in two groups (wd 0.01 / 0), lr of each group changed every step,
    clip_grad_norm_ without an optimizer argument, the clip active in steps 1, 3, 5 only; parameters PY_LAG have no gradient in steps
    2 and 3.  After every step each parameter against the float64 restatement of THAT step from the device's own p, m, v before it,
    with the parameter's own step count in the bias correction."""
    from vln_hamt_amd.optim import AdamW, clip_grad_norm_
    from vln_hamt_amd.optim.adamw import shadow_only
    pc = R.py_case()
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in pc["init"]]
    assert [shadow_only(p) for p in params] == [True, True] + [False] * 6
    assert shadow_only(params[R.PY_LAG[0]]) and not shadow_only(params[R.PY_LAG[1]])
    opt = AdamW([{"params": [p for p, g in zip(params, R.PY_GROUP) if g == k], "weight_decay": R.PY_WD[k]} for k in (0, 1)],
                lr=1e-3, betas=R.PY_BETAS, eps=R.PY_EPS)
    opt.materialize()
    where = [slice(opt._offs[opt._index_of[id(p)]], opt._offs[opt._index_of[id(p)]] + p.numel()) for p in params]
    arenas = dict(p=opt._flat_p, m=opt._flat_m, v=opt._flat_v, p16=opt._flat_p16)
    counts = np.zeros(len(params), dtype=np.int64)
    worst = 0.0
    for s, grads in enumerate(pc["grads"]):
        for p, g in zip(params, grads):
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)
        for k, grp in enumerate(opt.param_groups):
            grp["lr"] = R.PY_LR[s][k]
        torch.cuda.synchronize()
        before = {k: t.clone() for k, t in arenas.items()}
        gn = clip_grad_norm_(params, R.PY_MAX_NORM)
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        coef, gsq = R.py_coef(grads)
        assert (coef < 1.0) == (s % 2 == 0)
        assert abs(float(gn) - math.sqrt(gsq)) <= SUMSQ_TOL * math.sqrt(gsq), (s, float(gn), math.sqrt(gsq))
        for i, (p, g, sl) in enumerate(zip(params, grads, where)):
            assert p.data_ptr() == opt._flat_p.data_ptr() + 4 * sl.start
            if g is None:                            # the reference's `continue`: nothing of it moves
                for k in arenas:
                    assert same_bits(arenas[k][sl], before[k][sl]), (s, i, k)
                continue
            counts[i] += 1
            p0, m0, v0 = (before[k][sl].cpu().numpy() for k in ("p", "m", "v"))
            want = R.py_update(s, i, int(counts[i]), p0, g.reshape(-1), m0, v0, coef)
            for k, ref in zip(("p", "m", "v"), want):
                got = arenas[k][sl].cpu().numpy().astype(np.float64)
                err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
                worst = max(worst, err)
                assert err <= R.TOL, (s, i, k, err)
            assert same_bits(opt._flat_p16[sl], opt._flat_p[sl].to(torch.bfloat16)), (s, i)
    print(f"[adamw python steps] worst per-tensor error over 5 steps {worst:.2e} of max|ref|")
    assert counts.tolist() == [3 if i in R.PY_LAG else 5 for i in range(len(params))]
    order = [p for grp in opt.param_groups for p in grp["params"]]
    state = opt.state_dict()["state"]
    for j, p in enumerate(order):
        i = next(k for k, q in enumerate(params) if q is p)
        assert state[j]["step"] == counts[i], (i, state[j]["step"], counts[i])
