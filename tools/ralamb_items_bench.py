#!/usr/bin/env python3
"""The RangerLars update on the config-4 arena (the image-input model's parameters, pretrain_r2r_e2e.json) on ONE GPU: the whole
`hamt_ralamb_table` next to what rank 0 of a simulated world of 1, 2, 4 and 8 runs under parallel.ShardedItemSync --
`hamt_ralamb_moments_items` over its owned items, `hamt_ralamb_trust` over all parameters, `hamt_ralamb_apply_items` over its owned
items -- with and without a Lookahead sync.  No process group, no collective: the partial slots' all-reduce, the reduce-scatter and
the all-gathers are NOT in these numbers, and nothing here ran on more than one GPU.

Every cell has its own item table (the world's cuts: optim.rangerlars.item_table), partial slots and RangerLars table; the cells
alternate inside one process, `inner` launches per HIP-event window, one window per cell per round; reported: median and p10 / p90
over the rounds, algorithmic bytes (42 B per owned element, + 8 on a sync, + 4 where the gradient slot is zeroed; the trust pass
reads 8 B per item of the WHOLE table) and the rate they give.  Before timing, the union of the eight ranks' calls of world 8 is
compared with the whole launch on the same arenas, bit for bit.
usage: ralamb_items_bench.py [rounds=30] [inner=10] [out=profiles/ralamb_items_mi355x.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vln_hamt_amd import _lib as L
from vln_hamt_amd.ops import _p, _stream
from vln_hamt_amd.optim import RangerLars
from vln_hamt_amd.optim.misc import NO_DECAY
from vln_hamt_amd.optim.rangerlars import INTERPOLATE, item_table, owned_item_runs
from vln_hamt_amd.parallel import shard_cuts

WORLDS = (1, 2, 4, 8)
SYNC_WORLDS = (2, 8)
B1, B2, EPS = 0.9, 0.98, 1e-6


def build_optimizer(dev):
    from vln_hamt_amd.model.image_pretrain import MultiStepNavImagePreTraining
    from vln_hamt_amd.modeling import HamtConfig
    cfg = HamtConfig(hamt_precision="bf16", pretrain_tasks={"mlm", "sap", "sar", "sprel", "mrc", "itm"})
    model = MultiStepNavImagePreTraining(cfg).to(dev).train()
    named = list(model.named_parameters())
    opt = RangerLars([{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
                      {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}], lr=5e-5, betas=(B1, B2), eps=EPS)
    return model, opt.materialize()


class World:
    """item table, partial slots and rank 0's item runs of a simulated world (the construction of parallel.ShardedItemSync)"""

    def __init__(self, opt, world, parts=4):
        sc = shard_cuts(opt._n, opt._n_shadow_only, world, parts)
        self.ranges = [(lo, hi) for lo, hi in zip(sc[:-1], sc[1:]) if hi > lo]
        cuts = {lo + r * ((hi - lo) // world) for lo, hi in self.ranges for r in range(world + 1)}
        tab, self.nitems = item_table(opt._ends.cpu().numpy(), opt._n, cuts)
        self.tab = tab
        self.items = torch.from_numpy(tab).to(opt._flat_p.device)
        self.partials = torch.zeros(2 * self.nitems, dtype=torch.float32, device=opt._flat_p.device)
        self.world = world
        self.runs = [owned_item_runs(tab, self.nitems, self.owned(r)) for r in range(world)]

    def owned(self, rank):
        return [(lo + rank * ((hi - lo) // self.world), (hi - lo) // self.world) for lo, hi in self.ranges]


class Arenas:
    def __init__(self, opt, clone=False):
        f = (lambda t: t.clone()) if clone else (lambda t: t)
        self.p, self.g, self.m, self.v, self.p16, self.slow = (f(t) for t in (opt._flat_p, opt._flat_g, opt._flat_m, opt._flat_v, opt._flat_p16, opt._flat_slow))

    def equal(self, o):
        return all(torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                               b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))
                   for a, b in zip((self.p, self.g, self.m, self.v, self.p16, self.slow), (o.p, o.g, o.m, o.v, o.p16, o.slow)))


def launches(opt, a, w, rl, stats, gn):
    lib, npar = L.load(), len(opt._params)

    def whole():
        L.check(lib.hamt_ralamb_table(_p(a.p), _p(a.g), _p(a.m), _p(a.v), _p(a.p16), _p(a.slow), _p(w.items), w.nitems, _p(opt._hyp), _p(rl), npar,
                                      _p(w.partials), _p(stats), _p(gn), 5.0, B1, B2, 1 - B1, 1 - B2, EPS, 1, _stream()), "hamt_ralamb_table")

    def moments(rank):
        for f, c in w.runs[rank]:
            L.check(lib.hamt_ralamb_moments_items(_p(a.p), _p(a.g), _p(a.m), _p(a.v), _p(w.items), w.nitems, f, c, _p(opt._hyp), _p(rl), npar,
                                                  _p(w.partials), _p(gn), 5.0, B1, B2, 1 - B1, 1 - B2, EPS, 1, _stream()), "hamt_ralamb_moments_items")

    def trust():
        L.check(lib.hamt_ralamb_trust(_p(w.items), w.nitems, _p(opt._hyp), npar, _p(w.partials), _p(stats), _stream()), "hamt_ralamb_trust")

    def apply(rank):
        for f, c in w.runs[rank]:
            L.check(lib.hamt_ralamb_apply_items(_p(a.p), _p(a.m), _p(a.v), _p(a.p16), _p(a.slow), _p(w.items), w.nitems, f, c, _p(opt._hyp), _p(rl),
                                                npar, _p(stats), EPS, _stream()), "hamt_ralamb_apply_items")

    def rank0():
        w.partials.zero_()
        moments(0)
        trust()
        apply(0)

    return whole, moments, trust, apply, rank0


def cell_bytes(opt, w, sync, rank=None):
    """algorithmic HBM bytes: the whole update (rank None) or rank `rank`'s share + the trust pass over the whole table"""
    ends = opt._ends.cpu().numpy().astype(np.int64)
    begins = np.concatenate([[0], ends[:-1]])
    per = 42.0 + (8.0 if sync else 0.0) + np.where(opt._keep == 2.0, 0.0, 4.0)
    if rank is None:
        return float(((ends - begins) * per).sum())
    total = 0.0
    for f, c in w.owned(rank):
        ov = np.clip(np.minimum(ends, f + c) - np.maximum(begins, f), 0, None)
        total += float((ov * per).sum())
    return total + 8.0 * w.nitems + 32.0 * len(ends) + 8.0 * w.nitems       # + zeroing the partial slots


def main(rounds=30, inner=10, out_path=None):
    dev = torch.device("cuda", 0)
    model, opt = build_optimizer(dev)
    opt._flat_g.normal_(std=1e-3)
    opt._flat_m.normal_(std=1e-4)
    opt._flat_v.uniform_(1e-8, 1e-6)
    opt._flat_slow.copy_(opt._flat_p)
    act = [True] * len(opt._params)
    opt._packed = True
    table = opt.host_table(act)
    table[0, :, 1] = 1e-5                                   # (a fixed step size: the timing does not depend on it)
    opt.upload_table(table)
    rl_none = opt._rl.clone()
    rl_none[:, 1] = 0.0
    rl_sync = rl_none.clone()
    rl_sync[:, 1] = INTERPOLATE
    stats = torch.zeros(len(opt._params), 4, device=dev)
    gn = torch.full((1,), 4.0, device=dev)
    worlds = {w: World(opt, w) for w in WORLDS}
    plain = World(opt, 1, parts=1)                          # cuts at region ends only: parameter boundaries anyway -> today's table
    assert np.array_equal(plain.tab, opt._items_np)
    # ---- results must not change: world 8, every rank's calls in a scrambled order against the whole launch, on copies
    a1, a2 = Arenas(opt, clone=True), Arenas(opt, clone=True)
    w8 = worlds[8]
    s1, s2 = stats.clone(), stats.clone()
    launches(opt, a1, w8, rl_sync, s1, gn)[0]()
    pw = w8.partials.clone()
    w8.partials.fill_(float("nan"))
    _, moments, trust, apply, _ = launches(opt, a2, w8, rl_sync, s2, gn)
    for r in (5, 0, 7, 2, 1, 6, 3, 4):
        moments(r)
    trust()
    for r in (3, 6, 0, 4, 7, 1, 5, 2):
        apply(r)
    torch.cuda.synchronize()
    union_ok = bool(a1.equal(a2) and torch.equal(s1, s2) and torch.equal(pw.view(torch.int32), w8.partials.view(torch.int32)))
    print(f"world 8: union of the ranks' item calls == whole launch, bit for bit: {union_ok}", flush=True)
    assert union_ok
    del a1, a2
    torch.cuda.empty_cache()
    # ---- cells
    a = Arenas(opt)
    cells = {}
    for sync, rl in ((False, rl_none), (True, rl_sync)):
        tag = "_sync" if sync else ""
        cells["whole" + tag] = (launches(opt, a, plain, rl, stats, gn)[0], cell_bytes(opt, plain, sync), plain.nitems, 1)
        for wn in (SYNC_WORLDS if sync else WORLDS):
            w = worlds[wn]
            cells[f"items_world{wn}_rank0{tag}"] = (launches(opt, a, w, rl, stats, gn)[4], cell_bytes(opt, w, sync, 0), w.nitems, len(w.runs[0]))
    for fn, *_ in cells.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cells}
    for _ in range(rounds):
        for k, (fn, *_r) in cells.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) / inner * 1e3)
    assert bool(torch.isfinite(opt._flat_p).all())
    res = {}
    for k, (fn, nbytes, nitems, nruns) in cells.items():
        t = np.asarray(times[k])
        med = float(np.median(t))
        res[k] = {"us_median": round(med, 1), "us_p10": round(float(np.percentile(t, 10)), 1), "us_p90": round(float(np.percentile(t, 90)), 1),
                  "bytes_GB": round(nbytes / 1e9, 3), "TB_per_s": round(nbytes / med / 1e6, 2), "items_in_table": nitems, "item_runs": nruns}
        print(f"{k:32s} {med:9.1f} us  [{res[k]['us_p10']:9.1f}, {res[k]['us_p90']:9.1f}]  {nbytes / 1e9:7.3f} GB  {res[k]['TB_per_s']:5.2f} TB/s", flush=True)
    out = {"what": "RangerLars update on the config-4 arena, one GPU: whole hamt_ralamb_table vs rank 0's moments_items + trust + apply_items of a simulated world",
           "device": torch.cuda.get_device_name(0), "parameters_M": round(opt._n / 1e6, 1), "parameter_tensors": len(opt._params),
           "rounds": rounds, "launches_per_window": inner, "timer": "HIP events around `inner` back-to-back updates; cells alternate inside every round",
           "union_of_world8_ranks_equals_whole_bitwise": union_ok, "cells": res,
           "ratios_whole_over_rank0": {k: round(res["whole" + ("_sync" if k.endswith("_sync") else "")]["us_median"] / v["us_median"], 2)
                                       for k, v in res.items() if k.startswith("items_")},
           "notes": ["no collective was timed: the partial slots' all-reduce, the reduce-scatter, the norm's all-reduce and the parameter all-gathers are not in these numbers",
                     "no run on more than one GPU (N > 1) was made: the worlds are simulated, rank 0's share of the kernels on one device",
                     "arithmetic expectation, not a promise: 42 / world bytes per element (50 on a Lookahead sync) + a constant trust pass over the whole item table"]}
    out_path = out_path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ralamb_items_mi355x.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["ratios_whole_over_rank0"]))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30, int(sys.argv[2]) if len(sys.argv) > 2 else 10, sys.argv[3] if len(sys.argv) > 3 else None)
