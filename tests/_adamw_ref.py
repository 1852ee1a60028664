"""Plain numpy float64 restatement of the reference's HF AdamW (optim/adamw.py:53-112 of the modelled project) and the synthetic cases
of the op-level tests (test_adamw_ref.py proves on the CPU that the cases can tell a wrong kernel from a right one, test_gpu_adamw.py
runs the kernels on them).  Nothing here touches the GPU or the package under test."""
import functools

import numpy as np

SWEEP = 2048 * 4096          # floats one sweep of adamw_table_kernel's grid covers: 2 048 blocks x 16-KiB chunks of each array
CHUNK = 4096                 # floats per chunk
TOL = 2e-6                   # max|got - ref| <= TOL * max|ref| per tensor: the bound of test_ralamb_table_op_vs_float64
B1, B2 = 0.9, 0.98
MEDIUM = (4096, 4104, 12296, 100008, 500000)
N_TINY = 3000


def clip_coef(gsq, max_norm):
    """torch clip_grad_norm_'s coefficient; 1 without a norm or with max_norm <= 0"""
    if gsq is None or max_norm <= 0:
        return 1.0
    return min(1.0, float(max_norm) / (float(np.sqrt(np.float64(gsq))) + 1e-6))


def bias_correction(t, b1=B1, b2=B2):
    t = np.asarray(t, dtype=np.float64)
    return np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def adamw_f64(p, g, m, v, coef, lr, step, wd, b1, b2, eps):
    """one AdamW update in float64; arrays are fp32 values widened, scalars (or per-element arrays) the fp32 values the kernel receives"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2, eps = (float(np.float32(x)) for x in (b1, b2, eps))
    gg = g * coef
    m = b1 * m + (1.0 - b1) * gg
    v = b2 * v + (1.0 - b2) * gg * gg
    p = p - step * m / (np.sqrt(v) + eps)
    p = np.where(np.asarray(wd) > 0, p - lr * wd * p, p)       # decoupled decay on the UPDATED p, only where wd > 0
    return p, m, v


def adamw_f32(p, g, m, v, coef, lr, step, wd, b1, b2, eps):
    """the kernel's adamw_one in numpy float32, same operation order (no fused multiply-add)"""
    f = np.float32
    p, g, m, v, lr, step, wd = (np.asarray(a, dtype=f) for a in (p, g, m, v, lr, step, wd))
    coef, b1, b2, eps, one = f(coef), f(b1), f(b2), f(eps), f(1.0)
    gg = g * coef
    m = m * b1 + (one - b1) * gg
    v = v * b2 + (one - b2) * gg * gg
    p = p - step * (m / (np.sqrt(v) + eps))
    p = np.where(wd > 0, p - lr * wd * p, p)
    return p, m, v


def _rows(case):
    """per-element {lr, step, wd, flag} of an arena case: row i owns [begins[i], begins[i + 1]); the padding behind the last tensor
    takes the last row's, as the kernel gives it"""
    n, begins = case["n"], case["begins"]
    reps = np.diff(np.concatenate([begins, [n]]))
    return [np.repeat(case["hyp"][:, k], reps) for k in range(4)]


def _apply(case, coef, zero_grad, fn, dtype):
    lr, step, wd, flag = _rows(case)
    act = flag != 0
    out = {k: case[k].astype(dtype) for k in ("p", "g", "m", "v")}
    with np.errstate(invalid="ignore"):
        p, m, v = fn(case["p"][act], case["g"][act], case["m"][act], case["v"][act], coef, lr[act].astype(dtype), step[act].astype(dtype),
                     wd[act].astype(dtype), case["b1"], case["b2"], case["eps"])
    out["p"][act], out["m"][act], out["v"][act] = p, m, v
    if zero_grad:
        out["g"][flag == 1] = 0
    return out


def restate(case, coef, zero_grad=1):
    """float64 AdamW over an arena case: flag-0 tensors are left alone; the gradient becomes 0 where the flag is 1 and zero_grad is set"""
    return _apply(case, float(coef), zero_grad, adamw_f64, np.float64)


def emulate32(case, coef, zero_grad=1):
    return _apply(case, np.float32(coef), zero_grad, adamw_f32, np.float32)


def tensor_max(case, x):
    """max|x| per row of the table (flag-0 rows: 0)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    a[np.isnan(a)] = 0.0
    return np.maximum.reduceat(a, case["begins"])


def _finish(sizes, flags, hyp3, rng, zero, eps):
    sizes = np.asarray(sizes, dtype=np.int64)
    padded = (sizes + 7) // 8 * 8
    ends = np.cumsum(padded)
    begins = ends - padded
    n = int((ends[-1] + 511) // 512 * 512)
    if n == ends[-1]:
        n += 512                                   # (always some padding that belongs to no tensor)
    p, g, m, v = (np.zeros(n, np.float32) for _ in range(4))
    for i, sz in enumerate(sizes):
        lo, hi = int(begins[i]), int(ends[i])
        if flags[i] == 0:
            for a in (p, g, m, v):
                a[lo:hi] = np.nan
            continue
        if i == zero:
            continue
        p[lo:lo + sz] = rng.normal(0, 0.02, sz)
        g[lo:lo + sz] = rng.normal(0, 1e-2, sz)
        m[lo:lo + sz] = rng.normal(0, 1e-3, sz)
        v[lo:lo + sz] = rng.uniform(1e-7, 1e-4, sz)
    hyp = np.concatenate([np.asarray(hyp3, dtype=np.float64), np.asarray(flags, dtype=np.float64)[:, None]], 1).astype(np.float32)
    return dict(n=n, sizes=sizes, begins=begins, ends=ends, hyp=hyp, flags=hyp[:, 3].copy(), p=p, g=g, m=m, v=v, zero=zero, b1=B1, b2=B2, eps=eps)


@functools.lru_cache(maxsize=None)
def make_case(seed=5, eps=1e-6):
    """The arena of test A, in arena order (offsets multiples of 8, as optim.AdamW lays them out):
      1. one large tensor that ends a little before float offset SWEEP;
      2. N_TINY tensors of 8 to 40 elements that straddle SWEEP: block 0's second chunk starts inside this run and the block walks its
         parameter index over about half of it, each following block a few hundred entries further;
      3. MEDIUM, the last of which is the table's last row;
      4. padding up to a multiple of 512 that belongs to no tensor.
    Flags cycle 1, 2, 0 (large, all-zero and last tensor active; flag-0 slots hold NaN in p, g, m, v); lr alternates 1e-2 / 3e-2 from row
    to row, the step size is lr times the bias correction of step 1 + row % 9, wd alternates 0 / 0.05 every two rows: adjacent rows never
    share lr.  The returned arrays are shared: do not write to them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    tiny = rng.integers(8, 41, N_TINY)
    tiny_padded = int(((tiny + 7) // 8 * 8).sum())
    big = SWEEP - tiny_padded // 2 - 5             # (ends 5 elements before a multiple of 8: the gap counts as its tail)
    sizes = [big] + [int(s) for s in tiny] + list(MEDIUM)
    nt = len(sizes)
    idx = np.arange(nt)
    flags = np.array([1, 2, 0])[idx % 3]
    zero = 1 + N_TINY                              # the 4 096-element tensor: all zero and active
    flags[0], flags[zero], flags[-1] = 1, 1, 1
    lr = np.where(idx % 2 == 0, 1e-2, 3e-2)
    step = lr * bias_correction(1 + idx % 9)
    wd = np.where((idx // 2) % 2 == 0, 0.0, 0.05)
    return _finish(sizes, flags, np.stack([lr, step, wd], 1), rng, zero, eps)


def cut_case(case, i0, i1, seed=6):
    """rows [i0, i1) of `case`'s table as an arena of their own (same sizes, flags and hyper-parameters, fresh values)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    zero = case["zero"] - i0 if i0 <= case["zero"] < i1 else -1
    return _finish(case["sizes"][i0:i1], case["flags"][i0:i1].astype(np.int64), case["hyp"][i0:i1, :3].astype(np.float64), rng, zero,
                   case["eps"])


@functools.lru_cache(maxsize=None)
def small_case(seed=6, eps=1e-6):
    """a 40 000-float cut of make_case's layout: the end of its tiny run and the first three medium tensors (the last one active)"""
    c = make_case()
    i1 = 1 + N_TINY + 3
    i0 = int(np.searchsorted(c["begins"], c["ends"][i1 - 1] - 40000, side="left"))
    s = cut_case(c, i0, i1, seed)
    s["eps"] = eps
    assert s["flags"][-1] != 0 and 39000 < s["n"] < 41000
    return s


def shifted(case):
    """the same case with every tensor given the NEXT row's {lr, step, wd} (the last one: the first row's)"""
    c = dict(case)
    c["hyp"] = case["hyp"].copy()
    c["hyp"][:, :3] = np.roll(case["hyp"][:, :3], -1, axis=0)
    return c


# ---------------------------------------------------------------------------------------------- the python-level case (test E)
PY_SHAPES = [(64, 128), (128, 64), (128,), (128,), (5, 7), (1,), (300, 64), (256,)]
PY_GROUP = [0, 0, 1, 1, 0, 1, 0, 1]               # group 0: wd 0.01, group 1: wd 0
PY_WD = [0.01, 0.0]
PY_LR = [(1e-3, 2e-3), (2e-3, 1e-3), (3e-3, 5e-4), (2.5e-3, 1.5e-3), (1.5e-3, 2.5e-3)]     # per step, per group
PY_GRAD_SCALE = [1e-2, 1e-3, 1e-2, 1e-3, 1e-2]    # gradient norm ~ 190 x scale: clipped (max_norm 1) in steps 1, 3, 5, not in 2 and 4
PY_LAG = (1, 2)                                   # no gradient in steps 2 and 3: a GEMM weight (bf16-shadow region) and a bias (fp32 region)
PY_MAX_NORM = 1.0
PY_BETAS, PY_EPS = (0.9, 0.999), 1e-6


@functools.lru_cache(maxsize=None)
def py_case(seed=9):
    rng = np.random.Generator(np.random.PCG64(seed))
    init = [rng.normal(0, 0.02, s).astype(np.float32) for s in PY_SHAPES]
    grads = []
    for s, scale in enumerate(PY_GRAD_SCALE):
        grads.append([None if (s + 1 in (2, 3) and i in PY_LAG) else rng.normal(0, scale, sh).astype(np.float32)
                      for i, sh in enumerate(PY_SHAPES)])
    return dict(init=init, grads=grads)


def py_coef(grads):
    gsq = sum(float((g.astype(np.float64) ** 2).sum()) for g in grads if g is not None)
    return clip_coef(gsq, PY_MAX_NORM), gsq


def py_hyper(step_index, i, t):
    """the fp32 {lr, step size, wd} of parameter i in training step step_index + 1 when its own step count is t (optim.AdamW.host_table)"""
    lr = PY_LR[step_index][PY_GROUP[i]]
    b1, b2 = PY_BETAS
    return float(np.float32(lr)), float(np.float32(lr * bias_correction(t, b1, b2))), float(np.float32(PY_WD[PY_GROUP[i]]))


def py_update(step_index, i, t, p, g, m, v, coef):
    lr, ss, wd = py_hyper(step_index, i, t)
    return adamw_f64(p, g, m, v, coef, lr, ss, wd, PY_BETAS[0], PY_BETAS[1], PY_EPS)


def py_run(per_parameter=True):
    """the five steps in float64 (each result rounded to fp32, as the arenas hold it); returns per step the state BEFORE it, the step
    counts used in it, and the parameters after it"""
    c = py_case()
    p = [a.astype(np.float64).reshape(-1) for a in c["init"]]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    counts = np.zeros(len(p), dtype=np.int64)
    trace = []
    for s, grads in enumerate(c["grads"]):
        coef, _ = py_coef(grads)
        before = ([a.copy() for a in p], [a.copy() for a in m], [a.copy() for a in v])
        used = {}
        for i, g in enumerate(grads):
            if g is None:
                continue
            counts[i] += 1
            used[i] = int(counts[i]) if per_parameter else s + 1
            out = py_update(s, i, used[i], p[i], g.reshape(-1), m[i], v[i], coef)
            p[i], m[i], v[i] = (a.astype(np.float32).astype(np.float64) for a in out)
        trace.append(dict(before=before, used=used, coef=coef, p=[a.copy() for a in p], counts=counts.copy()))
    return trace
