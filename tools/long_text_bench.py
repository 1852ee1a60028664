#!/usr/bin/env python3
"""Does the packed text path pay at RxR's instruction length?  The pre-training step at the sizes of the reference's
rxr_xlm_model_config.json (hidden 768, 12 heads, 9 + 4 layers, two panorama layers, 512-d image features, the 250 002-token XLM-R
vocabulary) on ragged synthetic batches -- instruction lengths uniform in [62, 250], history lengths uniform in [0, T] -- with the packing
limit (vilmodel.PACK_MAX_LEN) at 128, where such a batch takes the padded kernels, against 256, where its text runs packed.

One process, one GPU; fails without one.  Per (B, T): the five tasks of pretrain_rxr.json, one batch each, as captured training steps
(forward, backward, clip, AdamW) -- one graph per (task, limit); every timed window alternates the two limits step by step; a step's time
is taken by device events around one replay.  Window 0 warms up and is dropped.  Reported per task and as the recipe's 5 : 1 : 1 : 1 : 2
mix of the per-task medians: median and p10-p90 in ms.  The losses of the two limits are compared first (dropout draws differ between
the layouts, so it is the eval-mode losses that are compared: 1e-2, reported, and the exit status says so).

Then the backward kernels alone, on the text self-attention of one B = 64 batch (12 heads, the same real tokens): hamt_attn_varlen_bwd
(attn_wide_bwd_kernel<packed>) on the packed rows against hamt_attn_small_bwd on the batch padded to 250 (attn16_bwd_kernel, the tiled
backward the padded layers run at this length), and the two forwards likewise; 50 launches per sample between two device events.

usage: long_text_bench.py [--batches 8,64] [--hist 5,20] [--reps 4] [--windows 5] [--eager] [--out profiles/long_text_pack_mi355x.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

TASKS, MIX = ("mlm", "sap", "sar", "sprel", "itm"), (5, 1, 1, 1, 2)      # pretrain_rxr.json: tasks, mix_ratio
L_TXT = 250                                                             # pretrain_rxr.json: max_txt_len
RXR = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, image_feat_size=512, angle_feat_size=4, image_prob_size=1000,
           num_l_layers=9, num_r_layers=0, num_h_layers=0, num_x_layers=4, num_h_pano_layers=2, max_position_embeddings=514,
           max_action_steps=100, vocab_size=250002, type_vocab_size=2)
LIMITS = (128, 256)


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "p10_p90": [round(float(np.percentile(xs, q)), 4) for q in (10, 90)], "n": len(xs)}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def build(dev):
    from vln_hamt_amd.model.pretrain_cmt import MultiStepNavCMTPreTraining
    from vln_hamt_amd.modeling import HamtConfig
    from vln_hamt_amd.optim import AdamW
    from vln_hamt_amd.optim.misc import NO_DECAY
    cfg = HamtConfig(hamt_precision="bf16", pretrain_tasks=set(TASKS), **RXR)
    torch.manual_seed(0)
    model = MultiStepNavCMTPreTraining(cfg).to(dev)
    named = list(model.named_parameters())
    opt = AdamW([{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
                 {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}], lr=5e-5, betas=(0.9, 0.98))
    opt.materialize()
    return cfg, model, opt


def step_bench(B, T, args, dev, cfg, model, opt):
    from vln_hamt_amd import ops
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.model import vilmodel
    from vln_hamt_amd.optim import clip_grad_norm_
    from vln_hamt_amd.synth import make_batch, make_itm_rng
    batches = {}
    for i, task in enumerate(TASKS):
        b = make_batch(task, B, cfg, seed=4100 + i, txt_len=L_TXT, hist_len=T, ragged=True, device=dev)
        if task == "itm":
            r = make_itm_rng(b, seed=i)
            b["itm_neg_idxs"], b["itm_shuffled_pos_ids"] = r["neg_idxs"], r["shuffled_pos_ids"]
        assert "txt_pack_idx" in b, "the batch carries no packing plan (nothing is padding)"
        batches[task] = b
    real = {t: int(b["txt_masks"].sum()) for t, b in batches.items()}
    padded = {t: int(b["txt_masks"].numel()) for t, b in batches.items()}
    # ---- the two limits compute the same loss (eval mode: no dropout)
    model.eval()
    agree = {}
    with torch.no_grad():
        for task, b in batches.items():
            ls = []
            for lim in LIMITS:
                vilmodel.PACK_MAX_LEN = lim
                ls.append(model(b, task, True).float().mean().item())
            agree[task] = abs(ls[0] - ls[1]) / max(1.0, abs(ls[0]))
    model.train()
    graphed = None if args.eager else GraphedTrainStep(model, opt, max_grad_norm=5.0)
    static = {}

    def step(task, lim):
        vilmodel.PACK_MAX_LEN = lim                       # read when the forward is built: at capture for a graphed step, every step otherwise
        if graphed is not None:
            key = (task, lim)
            loss = graphed.step(key, static.get(key, batches[task]), task)
            static[key] = graphed.static_batch(key)       # go on with the captured step's own input tensors: nothing to copy per step
            return loss
        loss = model(batches[task], task, True).mean()
        loss.backward()
        clip_grad_norm_(model.parameters(), 5.0, optimizer=opt)
        opt.step()
        opt.zero_grad()
        ops.advance_rng_epoch(dev)
        return loss

    ms = {(t, lim): [] for t in TASKS for lim in LIMITS}
    try:
        for task in TASKS:                                # capture (or first eager launch of) every shape, then one replay
            for lim in LIMITS:
                step(task, lim)
                step(task, lim)
        torch.cuda.synchronize()
        for w in range(args.windows + 1):
            for task in TASKS:
                for _ in range(args.reps):
                    for lim in LIMITS:                    # alternating inside the window
                        dt = event_ms(lambda: step(task, lim))
                        if w:
                            ms[task, lim].append(dt)
    finally:
        vilmodel.PACK_MAX_LEN = 128
    res = {"B": B, "T": T, "mode": "eager" if graphed is None else "captured steps", "real_text_tokens": real, "padded_text_tokens": padded,
           "eval_loss_rel_diff_between_limits": {t: round(v, 6) for t, v in agree.items()}, "step_ms": {}}
    for task in TASKS:
        res["step_ms"][task] = {f"limit_{lim}": stats(ms[task, lim]) for lim in LIMITS}
    mix = {lim: sum(m * statistics.median(ms[t, lim]) for t, m in zip(TASKS, MIX)) / sum(MIX) for lim in LIMITS}
    res["mix_5_1_1_1_2_of_medians_ms"] = {f"limit_{lim}": round(v, 4) for lim, v in mix.items()}
    res["packed_over_padded"] = round(mix[256] / mix[128], 4)
    res["losses_agree"] = all(v <= 1e-2 for v in agree.values())
    del graphed, static
    torch.cuda.empty_cache()
    return res


def kernel_bench(args, dev, B=64, heads=12, launches=50, samples=20):
    """the text self-attention of one ragged batch: packed rows through hamt_attn_varlen_*, the padded batch through hamt_attn_small_*"""
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd import ops
    lib, p, st = L.load(), ops._p, ops._stream()
    rng_np = np.random.default_rng(7)
    lens = rng_np.integers(L_TXT // 4, L_TXT + 1, size=B)
    lens[0] = L_TXT
    H, M, Mp = heads * 64, int(lens.sum()), B * L_TXT
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(3)
    qkv = torch.randn(M, 3 * H, device=dev, generator=g).bfloat16()
    do = torch.randn(M, H, device=dev, generator=g).bfloat16()
    valid = torch.from_numpy(np.arange(L_TXT)[None] < lens[:, None]).to(dev)
    rows = valid.reshape(-1).nonzero().squeeze(1)
    qkv_pad = torch.zeros(Mp, 3 * H, dtype=torch.bfloat16, device=dev)
    qkv_pad[rows] = qkv
    do_pad = torch.zeros(Mp, H, dtype=torch.bfloat16, device=dev)
    do_pad[rows] = do
    mask = ((~valid).float() * -10000.0).contiguous()
    ops.manual_seed(11, dev)
    rng = ops.rng_state(dev)

    def bufs(n):
        return (torch.empty(n, H, dtype=torch.bfloat16, device=dev), torch.empty(B * heads * L_TXT, dtype=torch.float32, device=dev),
                torch.empty(n, 3 * H, dtype=torch.bfloat16, device=dev))
    (o1, lse1, d1), (o0, lse0, d0) = bufs(M), bufs(Mp)
    desc = L.AttnDesc(B, heads, L_TXT, L_TXT, 64, 3 * H, 3 * H, 3 * H, H, L.HAMT_BF16, L.HAMT_BF16, 0.125, 0.1, 1, L.PREC_BF16)
    cols = lambda t: (t[:, :H], t[:, H:2 * H], t[:, 2 * H:])  # noqa: E731
    (q1, k1, v1), (q0, k0, v0), (a1, b1, c1), (a0, b0, c0) = cols(qkv), cols(qkv_pad), cols(d1), cols(d0)
    calls = {
        "fwd_packed": lambda: L.check(lib.hamt_attn_varlen_fwd(C.byref(desc), p(q1), p(k1), p(v1), p(cu), p(o1), p(lse1), p(rng), st), "varlen_fwd"),
        "fwd_padded": lambda: L.check(lib.hamt_attn_small_fwd(C.byref(desc), p(q0), p(k0), p(v0), p(mask), p(o0), p(lse0), p(rng), st), "small_fwd"),
        "bwd_packed": lambda: L.check(lib.hamt_attn_varlen_bwd(C.byref(desc), p(q1), p(k1), p(v1), p(cu), p(o1), p(do), p(lse1), p(a1), p(b1), p(c1), p(rng), st), "varlen_bwd"),
        "bwd_padded": lambda: L.check(lib.hamt_attn_small_bwd(C.byref(desc), p(q0), p(k0), p(v0), p(mask), p(o0), p(do_pad), p(lse0), None, p(a0), p(b0), p(c0), p(rng), st), "small_bwd"),
    }
    kernels = {}
    for name, fn in calls.items():                        # warm-up; the backward kernels' names; the two layouts agree on the real tokens
        fn()
        kernels[name] = L.last_kernel() if name.startswith("bwd") else "attn_s128_fwd_kernel"
    torch.cuda.synchronize()
    diff = {"out": float((o1.float() - o0[rows].float()).abs().max()), "dq": float((a1.float() - a0[rows].float()).abs().max()),
            "dk": float((b1.float() - b0[rows].float()).abs().max()), "dv": float((c1.float() - c0[rows].float()).abs().max())}
    scale = {"out": float(o0[rows].float().abs().max()), "dq": float(a0[rows].float().abs().max()), "dk": float(b0[rows].float().abs().max()),
             "dv": float(c0[rows].float().abs().max())}
    assert all(diff[k] <= 0.05 * scale[k] for k in diff), (diff, scale)      # two kernels' bf16 roundings of the same sums
    us = {k: [] for k in calls}
    for s in range(samples + 1):
        for name, fn in calls.items():                    # alternating
            dt = event_ms(lambda: [fn() for _ in range(launches)])
            if s:
                us[name].append(dt * 1e3 / launches)
    return {"what": f"text self-attention, B={B}, {heads} heads, lengths U[{L_TXT // 4}, {L_TXT}] ({M} real of {Mp} padded rows), bf16 in / out, p 0.1",
            "launches_per_sample": launches, "kernels": kernels, "max_abs_diff_on_real_rows": {k: round(v, 5) for k, v in diff.items()},
            "us_per_launch": {k: stats(v) for k, v in us.items()},
            "bwd_packed_over_padded": round(statistics.median(us["bwd_packed"]) / statistics.median(us["bwd_padded"]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--hist", default="5,20")
    ap.add_argument("--reps", type=int, default=4, help="steps per task, limit and window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--eager", action="store_true", help="eager steps instead of captured ones")
    ap.add_argument("--out", default=None, help="write the result as JSON here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_text_bench: needs a GPU (nothing here is measured on a CPU)")
    dev = torch.device("cuda", 0)
    res = {"what": "RxR-shaped pre-training step (rxr_xlm_model_config.json sizes, max_txt_len 250), ragged text: packing limit 128 (padded kernels) "
                   "against 256 (packed text), alternating in one process; device events",
           "gpu": torch.cuda.get_device_name(0), "steps": [], "attention_kernels": kernel_bench(args, dev)}
    print(json.dumps(res["attention_kernels"]), flush=True)
    cfg, model, opt = build(dev)
    for B in (int(x) for x in args.batches.split(",")):
        for T in (int(x) for x in args.hist.split(",")):
            res["steps"].append(step_bench(B, T, args, dev, cfg, model, opt))
            print(json.dumps(res["steps"][-1]), flush=True)
            if args.out:                                  # (kept current: a later configuration that fails leaves the earlier ones on disk)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
    if not all(r["losses_agree"] for r in res["steps"]):
        raise SystemExit("long_text_bench: the two limits disagree on an eval-mode loss (see eval_loss_rel_diff_between_limits)")


if __name__ == "__main__":
    main()
