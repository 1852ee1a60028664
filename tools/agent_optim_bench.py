#!/usr/bin/env python3
"""The optimiser step of a finetune iteration (finetune_src/r2r/agent_cmt.py:561-567, 597-602), three ways, alternating in one process:

  a  what an UNCHANGED agent loop runs today on this package's models: torch.nn.utils.clip_grad_norm_(vln_bert.parameters(), 40.) +
     two torch.optim.AdamW.step() + two zero_grad(), plus the re-cast of every bf16 weight shadow that the foreign update made stale
     (ops.weight_operand on each GEMM weight of the bf16 path: exactly the call, and the one hamt_cast_f32_bf16 launch per weight, that
     the next forward makes on first use -- timed here right after the step instead of spread over that forward);
  b  agent.AgentOptimizers.optim_step() + zero_grad() without the backward (--optim adamW);
  c  hamt_adamw_table with its hamt_sumsq_table launches over the SAME vln_bert arena (the pretraining update's kernels, launches only).
  b_kernels is b's device part for vln_bert alone (the norm + hamt_optim_table, launches only): what c compares with like for like.

Shape: VLNBertCMT at run_r2r.sh's configuration + Critic, bf16 mode, a gradient present for EVERY parameter (also those the recipe
freezes: the case without --fix_lang_embedding); in b the GEMM weights' gradients sit in their arena slots, as the weight-gradient
launch leaves them, the others are separate tensors that the step packs.  Device-synchronised host clock around each call, warm-up
first, median and min-max over the rounds.  Also: bytes per rule from the shapes and each rule's achieved rate (hamt_optim_table alone).

    python tools/agent_optim_bench.py --out profiles/agent_optim_mi355x.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/agent_optim_bench.py --segments
    python tools/agent_optim_bench.py --parse DIR --out profiles/agent_optim_mi355x.json     # adds kernel launches per iteration of a and b
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SEG_ITERS = 4
RULE_BYTES = {"adamw": 2, "adam": 2, "rmsprop": 1, "sgd": 0}        # moment arenas the rule owns


def r2r_args():
    """run_r2r.sh's flags (and the parser's defaults for what it leaves out), no checkpoint"""
    return types.SimpleNamespace(dataset="r2r", tokenizer="bert", image_feat_size=768, angle_feat_size=4, num_l_layers=9, num_h_layers=0,
                                 num_x_layers=4, hist_enc_pano=True, hist_pano_num_layers=2, fix_lang_embedding=True, fix_hist_embedding=True,
                                 fix_obs_embedding=False, no_lang_ca=False, act_pred_token="ob_txt", feat_dropout=0.4, dropout=0.5,
                                 bert_ckpt_file=None, hamt_precision="bf16", optim="adamW", lr=1e-5)


def build_pair(dev):
    from vln_hamt_amd.models.model_HAMT import Critic, VLNBertCMT
    args = r2r_args()
    torch.manual_seed(0)
    return args, VLNBertCMT(args).to(dev).train(), Critic(args).to(dev).train()


def make_cells(dev):
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import build_agent_optimizers
    from vln_hamt_amd.ops import _p, _stream
    from vln_hamt_amd.optim.adamw import shadow_only
    # ---- a: plain models, torch's optimisers
    args, vb_a, cr_a = build_pair(dev)
    pa = list(vb_a.parameters()) + list(cr_a.parameters())
    ga = [torch.randn_like(p) * 1e-3 for p in pa]
    gemm_w = [p for p in pa if shadow_only(p)]
    oa = [torch.optim.AdamW(vb_a.parameters(), lr=args.lr), torch.optim.AdamW(cr_a.parameters(), lr=args.lr)]

    def feed_a():
        for p, g in zip(pa, ga):
            p.grad = g

    def cell_a():
        torch.nn.utils.clip_grad_norm_(vb_a.parameters(), 40.)
        for o in oa:
            o.step()
        for o in oa:
            o.zero_grad()
        for w in gemm_w:
            ops.weight_operand(w, "bf16")

    # ---- b: the arenas
    args, vb_b, cr_b = build_pair(dev)
    ao = build_agent_optimizers(args, vb_b, cr_b)
    for o in ao.optimizers:
        o.materialize()
    pb = list(vb_b.parameters()) + list(cr_b.parameters())
    gb = [p._hamt_grad_slot if shadow_only(p) else torch.randn_like(p) * 1e-3 for p in pb]

    def feed_b():
        for o in ao.optimizers:
            o._flat_g.normal_(0.0, 1e-3)
            o._packed, o._table_ready, o._active = False, False, None      # (the launch-only cells leave them set)
        for p, g in zip(pb, gb):
            p.grad = g

    def cell_b():
        ao.optim_step()
        ao.zero_grad()

    # ---- c and b_kernels: launches only, over vln_bert's arena with the table of a step in which everything is active
    o = ao.vln_bert_optimizer
    lib = L.load()
    b1, b2, eps = o._launch_scalars(o.param_groups[0])

    def feed_k():
        o._flat_g.normal_(0.0, 1e-3)
        o._packed = True
        o.upload_table(o.host_table([True] * len(o._params), advance=False))
        o._table_ready, o._table_lrs = True, [g["lr"] for g in o.param_groups]

    def cell_c():
        gsq = o.global_grad_sumsq()
        L.check(lib.hamt_adamw_table(o._n, _p(o._flat_p), _p(o._flat_g), _p(o._flat_m), _p(o._flat_v), _p(o._flat_p16), _p(o._ends), _p(o._hyp),
                                     len(o._params), _p(gsq), 40.0, b1, b2, eps, 1, _stream()), "hamt_adamw_table")

    def cell_bk():
        o._pending_clip = (o.global_grad_sumsq(), 40.0)
        o.launch_step()

    def rule_cell(rule):
        def run():
            L.check(lib.hamt_optim_table(rule, o._n, _p(o._flat_p), _p(o._flat_g), _p(o._flat_m), _p(o._flat_v), _p(o._flat_p16), _p(o._ends),
                                         _p(o._hyp), _p(o._aux), len(o._params), None, 0.0, b1, b2, eps, 1, _stream()), "hamt_optim_table")
        return run

    bytes_per_rule = {k: o.update_bytes(moments=nm) for k, nm in RULE_BYTES.items()}
    info = dict(vln_bert_parameters=int(sum(p.numel() for p in vb_b.parameters())), critic_parameters=int(sum(p.numel() for p in cr_b.parameters())),
                vln_bert_tensors=len(o._params), arena_elements=int(o._n), gemm_weights_recast_in_a=len(gemm_w),
                update_bytes_per_rule=bytes_per_rule, bytes_per_element={k: 18 + 8 * nm for k, nm in RULE_BYTES.items()},
                sumsq_bytes=float(4.0 * o._n))
    cells = {"a": (feed_a, cell_a), "b": (feed_b, cell_b), "c": (feed_k, cell_c), "b_kernels": (feed_k, cell_bk)}
    rules = {k: (feed_k, rule_cell(i)) for i, k in enumerate(RULE_BYTES)}
    return cells, rules, info


def timed(feed, run):
    feed()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def stats(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1), "rounds": len(xs)}


def bench(dev, rounds, warmup):
    cells, rules, info = make_cells(dev)
    both = dict(cells, **{"rule_" + k: v for k, v in rules.items()})
    for _ in range(warmup):
        for feed, run in both.values():
            timed(feed, run)
    times = {k: [] for k in both}
    for _ in range(rounds):                      # alternating: every round runs every cell once
        for k, (feed, run) in both.items():
            times[k].append(timed(feed, run))
    res = {"workload": "optimiser step of a finetune iteration: VLNBertCMT (run_r2r.sh) + Critic, bf16 mode, a gradient for every parameter",
           "clock": "host perf_counter around one call, device-synchronised before and after; cells alternate within each round",
           "cell_a_shadow_share": "included: after the step, ops.weight_operand(w, 'bf16') on every GEMM weight of the bf16 path (the next "
                                  "forward's own call on first use: one hamt_cast_f32_bf16 launch per weight)",
           "shape": info, "cells": {k: stats(times[k]) for k in cells}, "rules": {}}
    for k in rules:
        s = stats(times["rule_" + k])
        s["bytes"] = info["update_bytes_per_rule"][k]
        s["achieved_TB_per_s"] = round(s["bytes"] / s["median_us"] / 1e6, 3)
        res["rules"][k] = s
    c, bk = res["cells"]["c"], res["cells"]["b_kernels"]
    res["b_kernels_minus_c_us"] = round(bk["median_us"] - c["median_us"], 1)
    res["c_spread_us"] = round(c["max_us"] - c["min_us"], 1)
    return res


def run_segments(dev):
    """for a kernel trace: [marker] a x SEG_ITERS [marker] b x SEG_ITERS [marker]; the marker is hamt_mse_fwd, which neither cell uses"""
    from vln_hamt_amd import ops
    cells, _, _ = make_cells(dev)
    x = torch.zeros(1, device=dev)
    for k in ("a", "b"):
        for _ in range(2):
            timed(*cells[k])
    for k in ("a", "b"):
        feed, run = cells[k]
        for _ in range(SEG_ITERS):
            feed()
            torch.cuda.synchronize()
            ops.mse_loss(x, x)
            run()
            torch.cuda.synchronize()
            ops.mse_loss(x, x)
    torch.cuda.synchronize()
    print("segments done", flush=True)


def parse_trace(path):
    """kernel launches per iteration of a and b: the dispatches between the two markers around each timed call"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {path}"
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            low = {k.lower(): v for k, v in r.items()}
            rows.append((int(low["start_timestamp"]), low["kernel_name"]))
    rows.sort()
    marks = [i for i, (_, n) in enumerate(rows) if "mse_fwd_kernel" in n]
    assert len(marks) >= 4 * SEG_ITERS, len(marks)
    marks = marks[-4 * SEG_ITERS:]
    out = {}
    for ci, k in enumerate(("a", "b")):
        counts, kinds = [], {}
        for it in range(SEG_ITERS):
            lo, hi = marks[2 * (ci * SEG_ITERS + it)], marks[2 * (ci * SEG_ITERS + it) + 1]
            seg = [n for _, n in rows[lo + 1:hi]]
            counts.append(len(seg))
            for n in seg:
                n = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0][-60:]
                kinds[n] = kinds.get(n, 0) + 1
        out[k] = {"kernel_launches_per_iteration": round(sum(counts) / SEG_ITERS, 2), "per_iteration": counts,
                  "kernels": {n: round(c / SEG_ITERS, 2) for n, c in sorted(kinds.items(), key=lambda kv: -kv[1])[:12]}}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", action="store_true")
    ap.add_argument("--parse", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 7, "at least 7 rounds"
    if a.parse:
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        res["launches"] = parse_trace(a.parse)
        res["launches"]["source"] = "rocprofv3 --kernel-trace --stats, a run of its own (--segments)"
    else:
        if not torch.cuda.is_available():
            raise SystemExit("agent_optim_bench: needs a GPU (no CPU fallback, no CPU timing)")
        dev = torch.device("cuda")
        if a.segments:
            run_segments(dev)
            sys.exit(0)
        res = bench(dev, a.rounds, a.warmup)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
