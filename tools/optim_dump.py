#!/usr/bin/env python3
"""Every output of the table optimiser and gradient-norm entry points of csrc/optim.hip on the GPU tests' own inputs, from a given
libhamt_hip.so: the evidence for "a change to csrc/optim.hip moved no bit" (a reordered sum is a difference here, not noise).

    python tools/optim_dump.py --lib PATH/libhamt_hip.so --out a.json       # once per library, each in a fresh process
    python tools/optim_dump.py --compare a.json b.json [--report FILE]     # exit status 1 unless every array is equal

(i)    hamt_adamw_table on tests/_adamw_ref.make_case(); hamt_adamw_table_range over the cuts of
       test_adamw_table_range_union_is_the_whole (the arenas after every range); the six variants of test_adamw_table_variants;
(ii)   hamt_optim_table, all four rules, on the cases of test_optim_table_vs_float64 and every variant of test_optim_table_variants;
(iii)  hamt_sumsq_table, plain and HAMT_SUMSQ_SPARSE, accumulate 0 and 1, on the tables of test_sumsq_table_active_only;
(iv)   hamt_wire_unpack_sumsq on test_wire_unpack_sumsq's case and on test_wire_unpack_sumsq_beyond_one_sweep's, accumulate 0 and 1;
(v)    hamt_sumsq and hamt_sumsq_partials on the sizes of test_sumsq_vs_float64 / test_sumsq_partials_vs_float64, accumulate 0 and 1.
The inputs are built by the test modules' own helpers.  A dump holds dtype, shape and the SHA-256 of each array's raw bytes (the arenas
of (i) are 170 MB per launch); the one-element sums carry their bit pattern too."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from image_dump import compare  # noqa: E402  (the same file format)

SPARSE = 2                                              # HAMT_SUMSQ_SPARSE


def dump(lib, out):
    import torch
    from vln_hamt_amd import _lib as L
    L.LIB_PATH = os.path.abspath(lib)                   # before the first load
    import _adamw_ref as A
    import _torch_optim_ref as R
    import test_gpu_adamw as TA
    import test_gpu_ops as TO
    import test_gpu_torch_optim as TT
    from vln_hamt_amd.ops import _p, _stream
    lib_, dev = L.load(), "cuda"
    arrays = {}

    def put(name, t):
        a = np.ascontiguousarray(t.detach().cpu().view(torch.uint8).numpy())
        arrays[name] = [str(t.dtype), list(t.shape), hashlib.sha256(a.tobytes()).hexdigest()] + ([a.tobytes().hex()] if t.numel() == 1 else [])

    def put_arenas(tag, d):
        for k, t in d.items():
            if t is not None:
                put(f"{tag}/{k}", t)

    # (i)
    c = A.make_case()
    d = TA.arena_init(c)
    init = TA.arena_init(c)
    TA.launch_table(c, d, TA.GSQ, TA.MAX_NORM)
    put_arenas("adamw_table/whole", d)
    b, e, n = c["begins"], c["ends"], c["n"]
    cuts = [0, 1028, int(b[2900]) + 4, int(e[2950]), int(b[2990]) + 4, n]
    for first, last in zip(cuts[:-1], cuts[1:]):
        TA.launch_table(c, init, TA.GSQ, TA.MAX_NORM, first=first, n=last - first)
        put_arenas(f"adamw_table_range/{first}-{last}", init)
    del d, init
    for variant, kw in (("keep_grad", dict(zero_grad=0)), ("no_shadow", dict(p16=False)), ("no_norm", dict(gsq=None)), ("max_norm_0", dict(max_norm=0.0)),
                        ("norm_below", dict(gsq=0.25)), ("eps_1e-8", dict(eps=1e-8))):
        c = A.small_case()
        if "eps" in kw:
            c = dict(c, eps=kw["eps"])
        d = TA.arena_init(c)
        TA.launch_table(c, d, kw.get("gsq", TA.GSQ), kw.get("max_norm", TA.MAX_NORM), kw.get("zero_grad", 1), kw.get("p16", True))
        put_arenas(f"adamw_table/{variant}", d)
    # (ii)
    for name, rule in TT._cases():
        c = R.with_rule(R.layouts()[name](), rule, "hot")
        d = TT.arena_init(c)
        assert TT.launch(c, d, TT.GSQ, TT.MAX_NORM) == 0
        put_arenas(f"optim_table/{name}/{R.NAMES[rule]}", d)
    for name in ("small", "medium"):
        for rule in R.RULES:
            for variant in ("keep_grad", "no_shadow", "no_norm", "max_norm_0", "norm_below", "agent", "null_unowned", "flag3"):
                c = R.with_rule(R.layouts()[name](), rule, "agent" if variant == "agent" else "hot")
                if variant == "flag3":
                    c["flags"] = np.where(c["flags"] == 2, 3, c["flags"]).astype(c["flags"].dtype)
                    c["hyp"] = c["hyp"].copy()
                    c["hyp"][:, 3] = c["flags"]
                d = TT.arena_init(c, "null" if variant == "null_unowned" else "nan")
                assert TT.launch(c, d, None if variant == "no_norm" else 0.25 if variant == "norm_below" else TT.GSQ,
                                 0.0 if variant == "max_norm_0" else TT.MAX_NORM, int(variant != "keep_grad"), variant != "no_shadow") == 0
                put_arenas(f"optim_table/{name}/{R.NAMES[rule]}/{variant}", d)
    # (iii)
    ws = torch.empty(1024, device=dev)
    for nparams in (5, 300, 1500):
        sizes, flags, ends, hyp, first, n = TO.sumsq_table_case(nparams)
        g = TO.rnd(sum(sizes), seed=5).to(dev)
        g[torch.cat([torch.full((sz,), f == 0.0) for sz, f in zip(sizes, flags)]).to(dev)] = float("nan")
        for sparse in (0, SPARSE):
            for acc in (0, 1):
                o = torch.full((1,), 2.0, device=dev)
                L.check(lib_.hamt_sumsq_table(first, n, _p(g[first:first + n]), _p(ends), _p(hyp), nparams, _p(o), acc | sparse, _p(ws), _stream()), "hamt_sumsq_table")
                put(f"sumsq_table/{nparams}/sparse{sparse}/acc{acc}", o)
    # (iv)
    sizes, flags = [1024, 2048, 512, 4096, 1536], [1.0, 0.0, 2.0, 3.0, 1.0]
    ends = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=dev)
    hyp = torch.zeros(len(sizes), 4, device=dev)
    hyp[:, 3] = torch.tensor(flags)
    small = (sizes, ends, hyp, 512, sum(sizes) - 512 - 1024)
    sizes, flags, ends, hyp, first, n = TO.sumsq_table_case(1500)
    for tag, (sizes, ends, hyp, first, n) in (("two_chunks", small), ("beyond_one_sweep", (sizes, ends, hyp, first, n))):
        y = TO.rnd(sum(sizes), seed=4).to(torch.bfloat16).to(dev)
        for acc in (0, 1):
            g = torch.full((sum(sizes),), float("nan"), device=dev)
            o = torch.full((1,), 3.0, device=dev)
            L.check(lib_.hamt_wire_unpack_sumsq(first, n, _p(y[first:first + n]), _p(g[first:first + n]), _p(ends), _p(hyp), len(sizes), _p(o), acc,
                                                _p(ws), _stream()), "hamt_wire_unpack_sumsq")
            put(f"wire_unpack_sumsq/{tag}/acc{acc}/g", g)
            put(f"wire_unpack_sumsq/{tag}/acc{acc}/sum", o)
    # (v)
    for n in (1, 3, 4, 1027, 1_048_576 + 4098):
        g = TA.with_canary(np.random.Generator(np.random.PCG64(n)).normal(0, 1.0, n).astype(np.float32))
        for acc in (0, 1):
            o = torch.tensor([TA.PRESET], dtype=torch.float32, device=dev)
            L.check(lib_.hamt_sumsq(n, _p(g), _p(o), acc, _p(ws), _stream()), "hamt_sumsq")
            put(f"sumsq/{n}/acc{acc}", o)
    for n in (1, 3, 4, 4095, 4097, 18001):
        x = TA.with_canary(np.random.Generator(np.random.PCG64(n)).uniform(0, 1.0, n).astype(np.float32))
        for acc in (0, 1):
            o = torch.tensor([TA.PRESET], dtype=torch.float32, device=dev)
            L.check(lib_.hamt_sumsq_partials(n, _p(x), _p(o), acc, _stream()), "hamt_sumsq_partials")
            put(f"sumsq_partials/{n}/acc{acc}", o)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(arrays, f, indent=0)
    print(f"optim_dump: {len(arrays)} arrays from {L.LIB_PATH} -> {out}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.report))
    dump(a.lib, a.out)
