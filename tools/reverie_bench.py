#!/usr/bin/env python3
"""ms per agent step of REVERIE's NavRefCMT at run_reverie.sh's shape (H 768, 9 + 4 layers, 2 panorama layers, 768-wide image and
object features, no_lang_ca; B 8, 60 tokens, 37 views, 20 objects, 3 history steps), next to NavCMT at the same shape without
objects (the comparison line).  Three cases per model:

  eager     no-grad: one `visual` decision + one `history` step (the agent's per-step calls), launched eagerly
  graphed   the same two calls as graph.GraphedInference replays
  train     a 3-step rollout (per step: visual, action CE [+ object CE], history), ONE backward, AdamW; reported per step

    python tools/reverie_bench.py [--steps 30] [--warmup 5] [--prec bf16]

Prints one JSON line per (model, case).  Weights are the models' own random initialisation (timing only)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vln_hamt_amd.reverie import synth  # noqa: E402

DEV = "cuda"
SHAPE = dict(B=8, txt_len=60, n_views=37, obj_lens=[20, 0, 7, 13, 1, 20, 4, 9], hist_steps=3)


def config(objects, prec):
    from vln_hamt_amd.modeling import HamtConfig
    kw = dict(max_action_steps=50 if objects else 100, image_feat_size=768, num_l_layers=9, num_x_layers=4, num_h_pano_layers=2,
              hist_enc_pano=True, no_lang_ca=True, fix_lang_embedding=False, fix_hist_embedding=False, fix_obs_embedding=False,
              hamt_precision=prec)
    if objects:
        kw["obj_feat_size"] = 768
    else:
        kw["act_pred_token"] = "ob"
    return HamtConfig(**kw)


def build(objects, prec):
    if objects:
        from vln_hamt_amd.reverie.vlnbert_navref import NavRefCMT as Model
    else:
        from vln_hamt_amd.models.vilmodel_cmt import NavCMT as Model
    return Model(config(objects, prec)).to(DEV)


def inputs(seed=43):
    x = synth.make_inputs(seed, SHAPE["B"], SHAPE["txt_len"], SHAPE["n_views"], SHAPE["obj_lens"], 768, 768, hist_steps=SHAPE["hist_steps"],
                          vocab_size=30522)
    x["step_ids"] = torch.arange(SHAPE["hist_steps"])          # (device tensors: the captured history step reads them)
    return {k: v.to(DEV) for k, v in x.items()}


def visual(model, objects, x, lang, hist):
    B, n = hist.shape[:2]
    kw = dict(txt_embeds=lang, txt_masks=x["txt_masks"], hist_embeds=hist, hist_masks=torch.ones(B, n, dtype=torch.bool, device=DEV),
              ob_img_feats=x["ob_img_feats"], ob_ang_feats=x["ob_ang_feats"], ob_nav_types=x["ob_nav_types"], ob_masks=x["ob_masks"])
    if objects:
        kw.update(obj_feats=x["obj_feats"], obj_angles=x["obj_angles"], obj_poses=x["obj_poses"], obj_masks=x["obj_masks"])
    return model("visual", **kw)


def history(model, x, t):
    return model("history", hist_img_feats=x["hist_img_feats"][t], hist_ang_feats=x["hist_ang_feats"][t], ob_step_ids=x["step_ids"][t:t + 1],
                 hist_pano_img_feats=x["hist_pano_img_feats"][t], hist_pano_ang_feats=x["hist_pano_ang_feats"][t])


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def bench(objects, prec, steps, warmup):
    from vln_hamt_amd import ops
    from vln_hamt_amd.graph import GraphedInference
    from vln_hamt_amd.optim import AdamW
    name = "NavRefCMT" if objects else "NavCMT"
    x = inputs()
    B = SHAPE["B"]
    model = build(objects, prec).eval()
    with torch.no_grad():
        lang = model("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
        hist = torch.stack([model("history").expand(B, -1)] + [history(model, x, t) for t in range(3)], 1).contiguous()
    out = []

    def step_eager():
        with torch.no_grad():
            visual(model, objects, x, lang, hist)
            history(model, x, 2)
    out.append(dict(model=name, case="eager", ms_per_step=timed(step_eager, steps, warmup)))
    gv = GraphedInference(lambda h: visual(model, objects, x, lang, h))
    gh = GraphedInference(lambda: history(model, x, 2))

    def step_graphed():
        gv("v", hist)
        gh("h")
    out.append(dict(model=name, case="graphed", ms_per_step=timed(step_graphed, steps, warmup)))
    del gv, gh
    model.train()
    for m in model.modules():             # timing of the training direction without dropout masks
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    opt = AdamW([{"params": [p for p in model.parameters() if p.requires_grad], "weight_decay": 0.01}], lr=1e-5, betas=(0.9, 0.98))
    act_t, ref_t = synth.targets({k: v.cpu() for k, v in x.items() if k != "step_ids"}, seed=1)
    act_t, ref_t = act_t.to(DEV), ref_t.to(DEV)

    def rollout():
        lg = model("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
        hs = [model("history").expand(B, -1)]
        loss = 0.0
        for t in range(3):
            o = visual(model, objects, x, lg, torch.stack(hs, 1))
            loss = loss + ops.cross_entropy(o[0], act_t).sum()
            if objects:
                loss = loss + ops.cross_entropy(o[1], ref_t).sum()
            hs.append(history(model, x, t))
        loss.backward()
        opt.step()
        opt.zero_grad()
    out.append(dict(model=name, case="train", ms_per_step=timed(rollout, max(3, steps // 3), max(2, warmup // 2)) / 3))
    for r in out:
        r.update(prec=prec, B=B, txt_len=SHAPE["txt_len"], views=SHAPE["n_views"], objects=(20 if objects else 0), hist_steps=3)
        r["ms_per_step"] = round(r["ms_per_step"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prec", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--only", choices=("reverie", "navcmt"), default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "reverie_bench needs a GPU"
    torch.manual_seed(0)
    for objects in (True, False):
        if a.only and (a.only == "reverie") != objects:
            continue
        for r in bench(objects, a.prec, a.steps, a.warmup):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
