#!/usr/bin/env python3
"""The agent's per-step action choice and losses: the reference's statement sequence as torch ops on the GPU -- today's
path, the BASELINE -- against agent.RolloutRecorder.step (one HIP launch, one more for the backward).

    python tools/policy_step_bench.py                      # the timing table + the graphed inference step -> one JSON line
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/policy_step_bench.py --segments
    python tools/policy_step_bench.py --parse DIR          # kernel launches per step of every cell, from that trace

Cells: B = 8 (BASELINE config 5) and B = 64, V = 37, feedback `sample` and `argmax`, forward and forward + backward.  Both variants
get what the agent has at that point: the logits on the device, the teacher's answer, the back-track mask and the candidate counts;
both must leave the environment's action on the HOST (the simulator needs it) and the chosen candidate's angle on the device.
  aten    agent_cmt.py:336-401 as written: cross_entropy, masked_fill_, softmax / Categorical / entropy / sample / log_prob (or max /
          log_softmax / gather), `.cpu()`, the two Python loops, the upload of the angle features, the hist_lens / ended book-keeping;
  fused   RolloutRecorder.step.
The backward is torch.autograd.backward on (ml, logp, ent) with ready-made gradients for both, so no loss arithmetic is timed.
The two variants alternate round by round in one process; the median over the rounds is reported, with the spread.
`--segments` runs every cell for a fixed number of steps with a marker kernel (hamt_mse_fwd, used by neither variant) between cells, so
that a kernel trace can be cut into cells; `--parse` counts the dispatches per cell and names the fused cells' kernels.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

V, A, IGNORE = 37, 4, -100
CELLS = [(B, fb, bwd) for B in (8, 64) for fb in ("sample", "argmax") for bwd in (False, True)]
SEG_STEPS = 50


def make_inputs(B, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(3, V + 1, (B,), generator=g)
    logit = torch.randn(B, V, generator=g) * 2
    logit[torch.arange(V)[None] >= n[:, None]] = -float("inf")
    bt = (torch.rand(B, V, generator=g) < 0.1) & (torch.arange(V)[None] < (n - 1)[:, None])
    ang = torch.randn(B, V, A, generator=g)
    s = dict(B=B, logit=logit.to(dev).requires_grad_(True), target=(torch.rand(B, generator=g) * (n - 1)).long().to(dev), bt=bt.to(dev),
             bt_u8=bt.to(torch.uint8).to(dev), cand_len=n.tolist(), cand_len_dev=n.to(torch.int32).to(dev), ang=ang.to(dev),
             ang_host=ang.numpy(), ended=np.zeros(B, bool), hist_lens=[1] * B,
             g=[torch.randn(B, generator=g).to(dev) for _ in range(3)], g_ml=torch.ones((), device=dev))
    return s


def aten_step(s, feedback, bwd, criterion):
    """agent_cmt.py:336-401 on the GPU, statement by statement (the reference masks in place; a leaf needs the out-of-place form)"""
    B, ended = s["B"], s["ended"]
    ctx = torch.enable_grad() if bwd else torch.no_grad()
    with ctx:
        logit = s["logit"]
        ml_loss = criterion(logit, s["target"])                                                       # :339
        logit = logit.masked_fill(s["bt"], -float("inf"))                                              # :350
        ent = None
        if feedback == "argmax":
            _, a_t = logit.max(1)                                                                      # :356
            a_t = a_t.detach()
            log_probs = F.log_softmax(logit, 1)
            lp = log_probs.gather(1, a_t.unsqueeze(1))                                                 # :359
        else:
            probs = F.softmax(logit, 1)                                                                # :361
            c = torch.distributions.Categorical(probs)
            ent = c.entropy()                                                                          # :364
            a_t = c.sample().detach()
            lp = c.log_prob(a_t)                                                                       # :366
    cpu_a_t = a_t.cpu().numpy()                                                                        # :372
    for i, next_id in enumerate(cpu_a_t):
        if next_id == (s["cand_len"][i] - 1) or next_id == IGNORE or ended[i]:
            cpu_a_t[i] = -1
    prev_act_angle = np.zeros((B, A), np.float32)                                                      # :382-386
    for i, next_id in enumerate(cpu_a_t):
        if next_id != -1:
            prev_act_angle[i] = s["ang_host"][i, next_id]
    prev_act_angle = torch.from_numpy(prev_act_angle).cuda()
    for i, i_ended in enumerate(ended):                                                                # :399-401
        if not i_ended:
            s["hist_lens"][i] += 1
    mask = torch.from_numpy((~ended).astype(np.float32)).cuda()                                        # :418-420, :490 (uploaded for the A2C loss)
    # (:447 `ended[:] = ...` is left out: the statements above cost the same whatever `ended` holds, as does the fused kernel)
    if bwd:
        s["logit"].grad = None
        outs, gs = [ml_loss, lp.reshape(B)], [s["g_ml"], s["g"][1]]
        if ent is not None:
            outs.append(ent); gs.append(s["g"][2])
        torch.autograd.backward(outs, gs)
    return cpu_a_t, prev_act_angle, mask


def fused_step(rec, s, feedback, bwd):
    ctx = torch.enable_grad() if bwd else torch.no_grad()
    with ctx:
        a_t, env, prev = rec.step(0, s["logit"], target=s["target"], cand_lens=s["cand_len_dev"], bt_mask=s["bt_u8"], ob_ang_feats=s["ang"],
                                  feedback=feedback)
    if bwd:
        s["logit"].grad = None
        ml, lp, ent = rec.rows(0)
        outs, gs = [ml, lp], [s["g"][0], s["g"][1]]
        if ent is not None:
            outs.append(ent); gs.append(s["g"][2])
        torch.autograd.backward(outs, gs)
    return env, prev


def _time(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def _variants(dev):
    from vln_hamt_amd.agent import RolloutRecorder
    criterion = torch.nn.CrossEntropyLoss(ignore_index=IGNORE, reduction="sum")                        # agent_cmt.py: size_average=False
    out = {}
    for B, fb, bwd in CELLS:
        s = make_inputs(B, dev)
        rec = RolloutRecorder(1, B, dev)

        out[(B, fb, bwd)] = {"aten": (lambda s=s, fb=fb, bwd=bwd: aten_step(s, fb, bwd, criterion)),
                             "fused": (lambda rec=rec, s=s, fb=fb, bwd=bwd: fused_step(rec, s, fb, bwd)), "rec": rec}
    return out


def _live(rec):
    """a fresh rollout state in front of every timed block (outside the timed loop)"""
    rec.ended.zero_()
    rec.hist_len.fill_(1)


def bench_cells(dev, rounds, iters):
    cells, res = _variants(dev), {}
    for key, v in cells.items():
        for name in ("aten", "fused"):
            for _ in range(20):
                v[name]()
        samples = {"aten": [], "fused": []}
        for _ in range(rounds):
            for name in ("aten", "fused"):                     # alternating, same process, same box
                _live(v["rec"])
                samples[name].append(_time(v[name], iters))
        B, fb, bwd = key
        r = {n: {"us_per_step": round(statistics.median(x), 2), "min": round(min(x), 2), "max": round(max(x), 2)} for n, x in samples.items()}
        r["fused_not_slower"] = r["fused"]["us_per_step"] <= r["aten"]["us_per_step"]
        res[f"B{B}_{fb}_{'fwd_bwd' if bwd else 'fwd'}"] = r
        print(f"[policy step] B {B:3d} {fb:7s} {'fwd+bwd' if bwd else 'fwd    '}: aten {r['aten']['us_per_step']:8.1f} us ({r['aten']['min']:.1f}-{r['aten']['max']:.1f})"
              f"   fused {r['fused']['us_per_step']:8.1f} us ({r['fused']['min']:.1f}-{r['fused']['max']:.1f})", flush=True)
    return res


def bench_graphed(dev, rounds, iters, n_hist=10, B=8, L=160, feat=512):
    """The full graphed inference step at the config-5 shape: `visual` and `history` as two GraphedInference replays with the aten choice
    (and its `.cpu()` and upload) between them, against ONE captured graph visual -> RolloutRecorder.step(sync=False) -> history followed
    by the copy of the environment action."""
    from vln_hamt_amd.agent import RolloutRecorder
    from vln_hamt_amd.graph import GraphedInference
    from vln_hamt_amd.modeling import HamtConfig
    from vln_hamt_amd.models.vilmodel_cmt import NavCMT
    cfg = HamtConfig(hamt_precision="bf16", image_feat_size=feat, hist_enc_pano=True, num_h_pano_layers=2, no_lang_ca=True, act_pred_token="ob_txt",
                     fix_lang_embedding=False, fix_hist_embedding=False, fix_obs_embedding=False, update_lang_bert=True, vocab_size=250002 // 8 * 8)
    torch.manual_seed(0)
    model = NavCMT(cfg).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    r = lambda *sh: torch.randn(*sh, generator=g).to(dev)
    txt_ids = torch.randint(5, 30000, (B, L), generator=g).to(dev)
    txt_masks = torch.ones(B, L, dtype=torch.bool, device=dev)
    hist, hm = r(B, n_hist, 768), torch.ones(B, n_hist, dtype=torch.bool, device=dev)
    oi, oa, himg, pimg, pang = r(B, V, feat), r(B, V, A), r(B, feat), r(B, 36, feat), r(B, 36, A)
    nav = torch.zeros(B, V, dtype=torch.long, device=dev); nav[:, :6] = 1; nav[:, V - 1] = 2
    ob_masks = torch.ones(B, V, dtype=torch.bool, device=dev)
    sid = torch.tensor([n_hist - 1], device=dev)
    s = make_inputs(B, dev)
    s["cand_len"], s["cand_len_dev"] = [V] * B, torch.full((B,), V, dtype=torch.int32, device=dev)
    s["ang_host"] = oa.cpu().numpy()
    out = {}
    with torch.no_grad():
        lang = model("language", txt_ids=txt_ids, txt_masks=txt_masks)
        visual = lambda h_, m_, i_, a_: model("visual", txt_embeds=lang, hist_embeds=h_, txt_masks=txt_masks, hist_masks=m_, ob_img_feats=i_,
                                               ob_ang_feats=a_, ob_nav_types=nav, ob_masks=ob_masks)[0]
        history = lambda i_, a_, p_, pa_: model("history", hist_img_feats=i_, hist_ang_feats=a_, ob_step_ids=sid, hist_pano_img_feats=p_, hist_pano_ang_feats=pa_)
        for fb in ("argmax", "sample"):
            gv, gh = GraphedInference(visual), GraphedInference(history)
            rec = RolloutRecorder(1, B, dev)

            def whole(h_, m_, i_, a_, hi_, p_, pa_, rec=rec, fb=fb):
                logit = visual(h_, m_, i_, a_)
                a_t, env, prev = rec.step(0, logit, cand_lens=s["cand_len_dev"], ob_ang_feats=a_, feedback=fb, sync=False)
                return env, history(hi_, prev, p_, pa_)
            gw = GraphedInference(whole, state=(rec.ended, rec.hist_len))

            def step_aten(fb=fb):
                logit = gv("v", hist, hm, oi, oa)
                if fb == "argmax":
                    _, a_t = logit.max(1)
                else:
                    a_t = torch.distributions.Categorical(F.softmax(logit, 1)).sample()
                cpu_a_t = a_t.cpu().numpy()
                for i, next_id in enumerate(cpu_a_t):
                    if next_id == (s["cand_len"][i] - 1) or next_id == IGNORE or s["ended"][i]:
                        cpu_a_t[i] = -1
                prev = np.zeros((B, A), np.float32)
                for i, next_id in enumerate(cpu_a_t):
                    if next_id != -1:
                        prev[i] = s["ang_host"][i, next_id]
                return cpu_a_t, gh("h", himg, torch.from_numpy(prev).cuda(), pimg, pang)

            def step_fused(rec=rec):
                env, h = gw("w", hist, hm, oi, oa, himg, pimg, pang)
                return rec.to_host(env), h
            fns = {"aten_between_two_graphs": step_aten, "fused_one_graph": step_fused}
            for f in fns.values():
                for _ in range(5):
                    f()
            samples = {k: [] for k in fns}
            for _ in range(rounds):
                for k, f in fns.items():
                    _live(rec)
                    samples[k].append(_time(f, iters))
            out[fb] = {k: {"us_per_step": round(statistics.median(x), 1), "min": round(min(x), 1), "max": round(max(x), 1)} for k, x in samples.items()}
            print(f"[graphed step] B {B} {fb:7s}: " + "   ".join(f"{k} {v['us_per_step']:.1f} us ({v['min']:.1f}-{v['max']:.1f})" for k, v in out[fb].items()), flush=True)
            del gv, gh, gw
    out["shape"] = {"B": B, "txt_len": L, "hist_tokens": n_hist, "views": V, "image_feat": feat}
    return out


def _marker(dev):
    from vln_hamt_amd import ops
    x = torch.zeros(1, device=dev)
    return lambda: ops.mse_loss(x, x)


def run_segments(dev):
    """for a kernel trace: [marker] cell 0 aten x SEG_STEPS [marker] cell 0 fused x SEG_STEPS [marker] cell 1 aten ... [marker]"""
    cells = _variants(dev)
    mark = _marker(dev)
    for v in cells.values():
        for name in ("aten", "fused"):
            for _ in range(5):
                v[name]()
    torch.cuda.synchronize()
    for key, v in cells.items():
        for name in ("aten", "fused"):
            _live(v["rec"])
            torch.cuda.synchronize()
            mark()
            for _ in range(SEG_STEPS):
                v[name]()
            torch.cuda.synchronize()
    mark()
    torch.cuda.synchronize()
    print("segments done", flush=True)


def parse_trace(path):
    files = [f for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)]
    assert files, f"no *kernel_trace.csv under {path}"
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            low = {k.lower(): v for k, v in r.items()}
            rows.append((int(low["start_timestamp"]), low["kernel_name"]))
    rows.sort()
    marks = [i for i, (_, n) in enumerate(rows) if "mse_fwd_kernel" in n]
    n_seg = 2 * len(CELLS)
    assert len(marks) >= n_seg + 1, (len(marks), n_seg)
    marks = marks[-(n_seg + 1):]                                # (the warm-up runs no marker; anything earlier is not ours)
    out, i = {}, 0
    for B, fb, bwd in CELLS:
        cell = {}
        for name in ("aten", "fused"):
            seg = [n for _, n in rows[marks[i] + 1:marks[i + 1]]]
            cell[name] = {"kernel_launches_per_step": round(len(seg) / SEG_STEPS, 2)}
            if name == "fused":
                kinds = {}
                for n in seg:
                    n = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0][-60:]
                    kinds[n] = kinds.get(n, 0) + 1
                cell[name]["kernels"] = {k: round(c / SEG_STEPS, 2) for k, c in kinds.items()}
            i += 1
        out[f"B{B}_{fb}_{'fwd_bwd' if bwd else 'fwd'}"] = cell
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", action="store_true")
    ap.add_argument("--parse", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--no-graphed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parse:
        res = {"launches": parse_trace(a.parse)}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("policy_step_bench: needs a GPU (no CPU fallback, no CPU timing)")
        dev = torch.device("cuda")
        if a.segments:
            run_segments(dev)
            sys.exit(0)
        res = {"workload": "per-step action choice + losses of the finetune agents, V = 37: aten statement sequence (baseline) vs RolloutRecorder.step",
               "rounds": a.rounds, "iters_per_round": a.iters, "cells": bench_cells(dev, a.rounds, a.iters)}
        if not a.no_graphed:
            res["graphed_inference_step"] = bench_graphed(dev, max(3, a.rounds // 2), 100)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
