#!/usr/bin/env python3
"""REVERIE's rollout step: `agent.ReverieRolloutRecorder.step` (ops.policy_ref_step, one launch) against the composition that was
available before it -- torch.max + cat + masked_fill, two F.cross_entropy, ops.policy_step on the V + 1 row, a blocking `.cpu()` of the
action and of the object logits and the host loop of the predicted object (finetune_src/reverie/agent.py:253-307).

    python tools/reverie_step_bench.py            # B 8 / 64, V 40, O 20; sample / argmax; forward / forward + backward -> one JSON line

Both paths alternate in one process; a cell is the median (min-max) of `--repeats` blocks of `--steps` steps, host clock around a block
that ends in a device synchronise.  `launches` counts the device kernels of one step of the new path (torch.profiler).  No threshold:
this is a first measurement.  Needs a GPU (no CPU timing)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
V, O, A, IGNORE = 40, 20, 4, -100


def make_inputs(B, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    n_nav = torch.randint(2, 9, (B,), generator=g)
    act = torch.randn(B, V, generator=g) * 2 + 2
    act[torch.arange(V)[None] >= n_nav[:, None]] = -float("inf")
    obj_len = torch.randint(0, O + 1, (B,), generator=g)
    obj = torch.randn(B, O, generator=g)
    obj[torch.arange(O)[None] >= obj_len.clamp(min=1)[:, None]] = -float("inf")
    target = (torch.rand(B, generator=g) * n_nav).long()
    target[::4] = V
    ref_target = torch.where((target == V) & (obj_len > 0), torch.zeros(B, dtype=torch.long), torch.full((B,), IGNORE))
    bt = torch.zeros(B, V, dtype=torch.bool)
    bt[torch.arange(B), (target.clamp(max=V - 1) + 1) % n_nav] = True
    bt[torch.arange(B)[target < V], target[target < V]] = False
    t = lambda x: x.to(dev)
    return dict(act=t(act), obj=t(obj), obj_len=t(obj_len.to(torch.int32)), obj_len_host=obj_len.tolist(), cand_len=t((n_nav + 1).to(torch.int32)),
                target=t(target), ref_target=t(ref_target), bt=t(bt), bt_u8=t(bt.to(torch.uint8)), ob_ang=t(torch.randn(B, V, A, generator=g)))


class Composed:
    """the step as it could be written before ops.policy_ref_step"""

    def __init__(self, B, dev):
        from vln_hamt_amd.agent import RolloutRecorder
        self.rec = RolloutRecorder(1, B, dev)
        self.cl = torch.full((B,), V + 1, dtype=torch.int32, device=dev)      # STOP is slot V of the V + 1 row
        self.zero_col = torch.zeros(B, 1, dtype=torch.bool, device=dev)
        self.pred = [None] * B

    def step(self, x, act, obj, feedback):
        from vln_hamt_amd import ops
        rec = self.rec.reset(fresh_draws=False)
        best = obj.max(1)[1]
        row = torch.cat([act, best.unsqueeze(1).float()], 1).masked_fill(torch.cat([x["bt"], self.zero_col], 1), -float("inf"))
        ml = F.cross_entropy(row, x["target"], ignore_index=IGNORE, reduction="sum")
        ref = F.cross_entropy(obj, x["ref_target"], ignore_index=IGNORE, reduction="sum")
        ang = F.pad(x["ob_ang"], (0, 0, 0, 1))
        _, logp, ent, a_t, env, prev = ops.policy_step(row, self.cl, rec.ended, rec.mask[0], mode=feedback, ob_ang=ang, hist_len=rec.hist_len)
        a_host, obj_host = a_t.cpu().numpy(), obj.detach().cpu()
        for i, a in enumerate(a_host):                                            # (:299-304; every step of this bench is the last one)
            n = x["obj_len_host"][i]
            self.pred[i] = None if n == 0 else int(obj_host[i, :n].max(0)[1])
        return ml + ref + logp.sum() + (ent.sum() if ent is not None else 0.0)


class Fused:
    def __init__(self, B, dev):
        from vln_hamt_amd.agent import ReverieRolloutRecorder
        self.rec = ReverieRolloutRecorder(1, B, dev)

    def step(self, x, act, obj, feedback):
        rec = self.rec.reset(fresh_draws=False)
        rec.step(0, act, obj, x["obj_len"], target=x["target"], cand_lens=x["cand_len"], bt_mask=x["bt_u8"], ob_ang_feats=x["ob_ang"],
                 feedback=feedback, ref_target=x["ref_target"])
        ml, logp, ent = rec.rows(0)
        return ml.sum() + rec._rows["ref"][0].sum() + logp.sum() + (ent.sum() if ent is not None else 0.0)


def block(path, x, feedback, backward, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        if backward:
            act, obj = x["act"].requires_grad_(True), x["obj"].requires_grad_(True)
            act.grad = obj.grad = None
            path.step(x, act, obj, feedback).backward()
        else:
            with torch.no_grad():
                path.step(x, x["act"], x["obj"], feedback)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def launches(path, x, feedback, backward, steps=20):
    from torch.profiler import ProfilerActivity, profile
    block(path, x, feedback, backward, 3)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        block(path, x, feedback, backward, steps)
    names = {}
    for e in prof.events():
        if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower():
            names[e.name] = names.get(e.name, 0) + 1
    return {k: round(v / steps, 2) for k, v in sorted(names.items())} or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reverie_step_bench: needs a GPU (no CPU fallback, no CPU timing)")
    dev = torch.device("cuda")
    out = {"V": V, "O": O, "steps": args.steps, "repeats": args.repeats, "cells": {}}
    for B in (8, 64):
        x = make_inputs(B, dev)
        paths = {"composed": Composed(B, dev), "fused": Fused(B, dev)}
        for feedback in ("sample", "argmax"):
            for backward in (False, True):
                for p in paths.values():
                    block(p, x, feedback, backward, 20)                           # warm-up of this cell's shapes
                times = {k: [] for k in paths}
                for _ in range(args.repeats):
                    for k, p in paths.items():                                    # alternating
                        times[k].append(block(p, x, feedback, backward, args.steps))
                cell = {k: {"us_per_step": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}
                cell["launches_fused"] = launches(paths["fused"], x, feedback, backward)
                out["cells"][f"B{B} {feedback} {'fwd bwd' if backward else 'fwd'}"] = cell
    print(json.dumps(out))


if __name__ == "__main__":
    main()
