#!/usr/bin/env python3
"""Micro-benchmark of the RangerLars update alone on the R2R-canon arena (174.8 M parameters), HIP-event timed, next to AdamW's.

Algorithmic bytes per element (optim.rangerlars.Ralamb.update_bytes): pass 1 reads p, g, m, v and writes m, v (24 B), pass 3 reads
p, m, v and writes p and the bf16 shadow (18 B), + 4 B where the gradient slot is zeroed, + 8 B (slow weights) on a Lookahead
sync; AdamW: 30 B + 4 B where the slot is zeroed (optim.AdamW.update_bytes).  Every parameter active, as after a full backward.
usage: rangerlars_bench.py [iters=20]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import build_model
from vln_hamt_amd.optim import AdamW, RangerLars
from vln_hamt_amd.optim.misc import NO_DECAY


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main(iters=20):
    dev = torch.device("cuda", 0)
    model, _ = build_model("bf16", dev)
    named = list(model.named_parameters())
    groups = lambda: [{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
                      {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]
    out = {}
    for name, cls in (("adamw", AdamW), ("rangerlars", RangerLars)):
        opt = cls(groups(), lr=5e-5, betas=(0.9, 0.98)).materialize()
        opt._flat_g.normal_(std=1e-3)
        act = [True] * len(opt._params)
        kinds = [("update", None)] if name == "adamw" else [("update", False), ("update_lookahead_sync", True)]
        for kind, sync in kinds:
            opt._packed = True
            table = opt.host_table(act)
            if sync is not None:
                table[1, :, 1] = 2.0 if sync else 0.0      # every parameter interpolates (a sync after the first), or none
                table[0, :, 1] = 1e-5                       # (a fixed step size: the timing does not depend on it)
            opt.upload_table(table)
            us = timeit(lambda: opt.launch_step(), iters)
            nbytes = opt.update_bytes(act, sync=bool(sync)) if sync is not None else opt.update_bytes(act)
            out[f"{name}_{kind}"] = {"us": round(us, 1), "bytes_GB": round(nbytes / 1e9, 3), "TB_per_s": round(nbytes / us / 1e6, 2)}
            print(f"{name:10s} {kind:22s} {us:8.1f} us  {nbytes / 1e9:6.3f} GB  {nbytes / us / 1e6:5.2f} TB/s", flush=True)
        out["parameters_M"] = round(opt._n / 1e6, 1)
        assert bool(torch.isfinite(opt._flat_p).all())
        del opt
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
