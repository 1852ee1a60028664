"""Cases and caps of the packed attention forms with 129 .. 256 tokens on a side (hamt_attn_varlen_* above the 128 of the s128 backward:
attn_s128_fwd_kernel in two query chunks / with key blocks 9 .. 16, the PACKED form of attn_wide_bwd_kernel), on top of tests/_attn_ref.py: the same
float64 statement, the same restatement (a packed call is restated with the fast exp -- the single-pass rounding, which is the packed wide
backward's too), the same units.  test_attn_long_ref.py proves on the CPU that the cases tell a wrong kernel from a right one,
test_gpu_attn_long.py runs the kernels on them.  Nothing here touches torch, the GPU or the package under test."""
import contextlib
import functools

import numpy as np

import _attn_ref as R

CHUNK = 128                              # queries per workgroup of the single-pass forward; the longest side of the s128 backward


def bwd_kernel(c):
    """hamt_attn16_bwd_launch for a packed call: a side above 128 -> the packed wide kernel, else s128"""
    assert c["path"] == "bf16" and c["form"] != "pad"
    return "attn_wide_bwd_kernel<packed>" if max(c["Sq"], c["Sk"]) > CHUNK else "attn_s128_bwd_kernel"


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case (bf16 path, 2 heads).  The arrays are shared: do not write to them."""
    out = {}
    n = [0]

    def add(name, *a, rot=None, **kw):
        out[name] = R.make_case(name, *a, seed=700 + n[0], rot=n[0] if rot is None else rot, **kw)
        n[0] += 1
    add("long self 256 p 0.1", "bf16", 256, 256, 0.1, form="vself", lens_q=(1, 129, 0, 250, 256, 144, 17, 128))
    add("long self 250 bf16io", "bf16", 250, 250, 0.0, io="bf16", form="vself", lens_q=(250, 1, 0, 129, 177, 64))
    add("long q 250x70 pair p 0.1", "bf16", 250, 70, 0.1, form="vq", lens_q=(5, 0, 250, 129, 17, 200), pair=(2, -1, 0, 1, -1, 3),
        rot=6)                               # key sides nomask, randn, peaked, ramp; the next case's: headmask, allmask, lastonly
    add("long q 128x140 fillers behind p 0.1 bf16io", "bf16", 128, 140, 0.1, io="bf16", form="vq", lens_q=(80, 33, 128, 7, 20), n_pairs=3)
    add("long k 70x250 pair p 0.1", "bf16", 70, 250, 0.1, form="vk", lens_k=(3, 250, 0, 129, 17), pair=(1, -1, 0, 3, 2, 4))
    add("long k 200x256 p 0.5 bf16io", "bf16", 200, 256, 0.5, io="bf16", form="vk", lens_k=(256, 1, 130))
    return out


def short_case():
    """a packed call with both sides <= 128: it stays on attn_s128_bwd_kernel"""
    return R.cases()["packed q pair p 0.1"]


@functools.lru_cache(maxsize=None)
def nan_case():
    """B = 3, lengths no multiple of 16 and on both sides of 128; the GPU test overwrites the middle sequence's q, k, v, dO with NaN"""
    return R.make_case("nan neighbour long self p 0.1", "bf16", 250, 250, 0.1, form="vself", lens_q=(130, 250, 37), seed=790, rot=1)


# ---------------------------------------------------------------------------------------------- the long-sequence mistakes
def keys_from_128_ignored(c):
    """the result of a kernel that stops at key block 8: the restatement of the case with the keys from 128 on masked out"""
    m = np.zeros((c["Bk"], c["Sk"]), dtype=R.F32) if c["mask"] is None else c["mask"].copy()
    m[:, CHUNK:] = -np.inf
    return R.restate(dict(c, mask=m))


def chunk1_draws_chunk0(c):
    """query rows from 128 on hash the dropout row of chunk 0 (the chunk offset left out of the row), forward and backward alike"""
    F = c["F"].copy()
    F[:, :, CHUNK:] = F[:, :, :c["Sq"] - CHUNK]
    return R.restate(dict(c, F=F))


def _per_sequence(c, res, fn):
    got = {k: v.copy() for k, v in res.items()}
    for b, _, rq, _ in R.pairs(c):
        if rq.stop - rq.start > CHUNK:
            fn(got, b, rq)
    return got


def chunk1_unwritten(c):
    """query rows from 128 on left as the (zero) buffer held them: out, lse, dq"""
    def fn(got, b, rq):
        got["out"][rq.start + CHUNK:rq.stop], got["dq"][rq.start + CHUNK:rq.stop] = 0.0, 0.0
        got["lse"][b, :, CHUNK:rq.stop - rq.start] = 0.0
    return _per_sequence(c, R.restate(c), fn)


def chunk1_takes_chunk0_statistics(c):
    """query rows from 128 on hold the lse of the row 128 before them (the chunk offset left out of the statistics' index)"""
    def fn(got, b, rq):
        n = rq.stop - rq.start
        got["lse"][b, :, CHUNK:n] = got["lse"][b, :, :n - CHUNK]
    return _per_sequence(c, R.restate(c), fn)


# ---------------------------------------------------------------------------------------------- caps
# The elementwise maximum of _attn_ref.MEASURED (bf16 paths) and of the restatement's worst error against attn64 over cases() and nan_case(),
# per (path, output, row kind), rounded up to two digits; printed and asserted by test_attn_long_ref.py.  Same GPU_MARGIN on top.
# MEASURED_TABLES
MEASURED = {
    "bf16": {
        "out": {"allmask": 0.0064, "filler": 0, "headmask": 0.0053, "lastonly": 0.0048, "nomask": 0.0083, "peaked": 0.0066, "ramp": 0.0064, "randn": 0.0062},
        "lse": {"allmask": 0.0007, "filler": 0, "headmask": 0.00041, "lastonly": 0.0016, "nomask": 0.00083, "peaked": 4.5e-07, "ramp": 0.00062, "randn": 0.0008},
        "dq": {"allmask": 0.0072, "filler": 0, "headmask": 0.0084, "lastonly": 0.0048, "nomask": 0.017, "peaked": 0.06, "ramp": 0.029, "randn": 0.029},
        "dk": {"allmask": 0.0084, "allmask q1": 0.33, "headmask": 0.0069, "headmask q1": 0.17, "lastonly": 0.00066, "lastonly q1": 0.0011, "nomask": 0.0084, "nomask q1": 0.14, "peaked": 0.069, "peaked q1": 0.4, "ramp": 0.0062, "ramp q1": 0.066, "randn": 0.0061, "randn q1": 0.2},
        "dv": {"allmask": 0.005, "allmask q1": 0.014, "headmask": 0.0054, "headmask q1": 0.014, "lastonly": 0.0031, "lastonly q1": 0.0048, "nomask": 0.0066, "nomask q1": 0.013, "peaked": 0.0066, "peaked q1": 0.0062, "ramp": 0.0033, "ramp q1": 0.0083, "randn": 0.0065, "randn q1": 0.012},
    },
    "bf16/bf16": {
        "out": {"allmask": 0.0035, "filler": 0, "headmask": 0.0026, "lastonly": 0.0042, "nomask": 0.0037, "peaked": 0.0056, "ramp": 0.0042, "randn": 0.0036},
        "lse": {"allmask": 0.00011, "filler": 0, "headmask": 1.1e-07, "lastonly": 5.4e-08, "nomask": 9.9e-08, "peaked": 3.3e-07, "ramp": 2.6e-07, "randn": 1.1e-07},
        "dq": {"allmask": 0.0036, "filler": 0, "headmask": 0.0036, "lastonly": 0.0025, "nomask": 0.0092, "peaked": 0.032, "ramp": 0.0065, "randn": 0.0049},
        "dk": {"allmask": 0.0036, "headmask": 0.0036, "lastonly": 0.00048, "lastonly q1": 0.00092, "nomask": 0.0041, "peaked": 0.045, "ramp": 0.0029, "randn": 0.0048},
        "dv": {"allmask": 0.0039, "headmask": 0.0043, "lastonly": 0.0035, "lastonly q1": 0.0035, "nomask": 0.0037, "peaked": 0.0063, "ramp": 0.0028, "randn": 0.0049},
    },
}


def long_cases():
    return list(cases().values()) + [nan_case()]


def merged_measure():
    """max(_attn_ref.MEASURED, measure(the long cases)) per (path, output, kind) of the bf16 paths"""
    new = R.measure(long_cases())
    tab = {}
    for path in ("bf16", "bf16/bf16"):
        for name in R.OUTPUTS:
            old, nw = R.MEASURED[path][name], new.get(path, {}).get(name, {})
            tab.setdefault(path, {})[name] = {k: max(old.get(k, 0.0), nw.get(k, 0.0)) for k in sorted(set(old) | set(nw))}
    return tab


@contextlib.contextmanager
def long_caps():
    """_attn_ref's cap / bound / worst_ratio (and test_gpu_attn's check, which calls them) read this module's table inside the block"""
    old = R.MEASURED
    R.MEASURED = dict(old, **MEASURED)
    try:
        yield
    finally:
        R.MEASURED = old
