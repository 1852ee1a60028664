#!/usr/bin/env python3
"""Generate tests/golden/reverie_tiny.npz by running the REFERENCE's own REVERIE model (finetune_src/reverie/vlnbert_navref.py
NavRefCMT, model_navref.py NavRefModel) on CPU in fp32.

Test infrastructure, like tools/gen_rangerlars_golden.py (needs the reference checkout, oracle.ref_shim.REF):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_reverie_golden.py

Weights: oracle.hamt_oracle.make_state_dict over the reference model's own state_dict shapes.  Inputs: vln_hamt_amd.reverie.synth
(rebuilt from the same seeds by the tests, not stored).  Cases:
  a/<lang>   tiny config (H 128, 2 heads, 64-wide image and object features), eval: language, the history cls token and 3 steps,
             visual with ragged object counts incl. a viewpoint without objects -- all six outputs;  <lang> = nolangca / ca
  b/         the same (no_lang_ca) with every obj_embeddings bias zero (the fresh-initialisation corner);
  c/         training direction, every dropout 0: a 3-step rollout, action CE + object CE per step (ignore_index -100, reduction
             sum, as the agent's criterion), ONE backward: the loss, every parameter's gradient norm, strided probes of some;
  d/<lang>   NavRefModel.forward('visual', ..., return_states=True) with the list of history embeddings and ragged hist_lens;
  e/         one full-size forward at run_reverie.sh's shape (H 768, 9 + 4 layers, 2 panorama layers, 768-wide features, B 8,
             60 tokens, 37 views, 20 objects): logits and output probes only;
  keys       the reference NavRefCMT's state_dict keys, in order.
NavRefModel is built with __new__ around the reference NavRefCMT (its __init__ would fetch bert-base-uncased's config from the hub),
as oracle/gen_goldens.py:gen_agent_models does for VLNBertCMT.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import ref_shim                                    # noqa: E402
from oracle.hamt_oracle import OracleConfig, make_state_dict   # noqa: E402
from vln_hamt_amd.reverie import synth                         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NAME = "reverie_tiny.npz"
PROBE_N = 64
SD_SEED = 17
TINY = dict(B=4, txt_len=24, n_views=9, obj_lens=[5, 0, 3, 1], seed=41)
FULL = dict(B=8, txt_len=60, n_views=37, obj_lens=[20, 0, 7, 13, 1, 20, 4, 9], seed=43)
HIST_LENS = {4: [4, 2, 3, 1], 8: [4, 2, 3, 1, 4, 4, 2, 3]}
GRAD_PROBES = ("obj_embeddings.", "ref_object.", "embeddings.token_type_embeddings.weight", "img_embeddings.nav_type_embedding.weight",
               "next_action.net.0.weight", "encoder.x_layers.0.visual_attention.att.query.weight", "img_embeddings.img_linear.weight",
               "hist_embeddings.position_embeddings.weight")


def tiny_cfg(no_lang_ca=True, **kw):
    return OracleConfig.tiny(hidden_size=128, num_attention_heads=2, intermediate_size=256, image_feat_size=64, max_action_steps=50,
                             no_lang_ca=no_lang_ca, **kw)


def full_cfg():
    return OracleConfig(hidden_size=768, num_attention_heads=12, intermediate_size=3072, vocab_size=30522, max_action_steps=50,
                        image_feat_size=768, num_l_layers=9, num_x_layers=4, num_h_pano_layers=2, no_lang_ca=True)


def obj_feat_size(cfg):
    return cfg.image_feat_size          # run_reverie.sh: --image_feat_size ${ft_dim} --obj_feat_size ${ft_dim}


def inputs(cfg, case):
    return synth.make_inputs(case["seed"], case["B"], case["txt_len"], case["n_views"], case["obj_lens"], cfg.image_feat_size,
                             obj_feat_size(cfg), hist_steps=3, vocab_size=cfg.vocab_size)


def probe(t, n=PROBE_N):
    f = t.detach().reshape(-1)
    return f[:: max(1, f.numel() // n)][:n].numpy().copy()


def import_ref():
    for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        del sys.modules[k]
    return ref_shim._import_pkg("finetune_src", "reverie", ["vlnbert_navref", "model_navref"])


def build_ref(vn, cfg, zero_obj_bias=False):
    model = vn.NavRefCMT(ref_shim.make_config(cfg, output_attentions=True, obj_feat_size=obj_feat_size(cfg)))
    sd = make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=SD_SEED)
    if zero_obj_bias:
        sd = {k: (torch.zeros_like(v) if k.startswith("obj_embeddings.") and k.endswith("bias") else v) for k, v in sd.items()}
    model.load_state_dict(sd, strict=True)
    return model


def run_visual(fwd, x, hist, hist_masks):
    return fwd("visual", txt_embeds=x["lang"], txt_masks=x["txt_masks"], hist_embeds=hist, hist_masks=hist_masks,
               ob_img_feats=x["ob_img_feats"], ob_ang_feats=x["ob_ang_feats"], ob_nav_types=x["ob_nav_types"], ob_masks=x["ob_masks"],
               obj_feats=x["obj_feats"], obj_angles=x["obj_angles"], obj_poses=x["obj_poses"], obj_masks=x["obj_masks"])


def history(fwd, x, t):
    return fwd("history", hist_img_feats=x["hist_img_feats"][t], hist_ang_feats=x["hist_ang_feats"][t], ob_step_ids=torch.tensor([t]),
               hist_pano_img_feats=x["hist_pano_img_feats"][t], hist_pano_ang_feats=x["hist_pano_ang_feats"][t])


def episode(model, x, B):
    """language, the history cls token and 3 steps, then one visual call with ragged history lengths -> the six outputs"""
    x = dict(x)
    x["lang"] = model("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
    hs = [model("history").expand(B, -1)] + [history(model, x, t) for t in range(3)]
    hist_masks = torch.arange(4)[None] < torch.tensor(HIST_LENS[B])[:, None]
    return run_visual(model, x, torch.stack(hs, 1), hist_masks)


def generate():
    vn, mn = import_ref()
    torch.manual_seed(0)
    store = {}
    # (a), (b): tiny config, eval
    for tag, no_lang_ca, zero in (("a/nolangca", True, False), ("a/ca", False, False), ("b", True, True)):
        cfg = tiny_cfg(no_lang_ca)
        model = build_ref(vn, cfg, zero).eval()
        if tag == "a/nolangca":
            store["keys"] = np.array(list(model.state_dict().keys()))
        with torch.no_grad():
            outs = episode(model, inputs(cfg, TINY), TINY["B"])
        for name, o in zip(("act_logits", "obj_logits", "txt", "hist", "ob", "obj"), outs):
            store[f"{tag}/{name}"] = o.numpy().copy()
    # (c): training direction, dropout 0
    cfg = tiny_cfg(True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pred_head_dropout_prob=0.0)
    model = build_ref(vn, cfg).train()
    x = inputs(cfg, TINY)
    act_t, ref_t = synth.targets(x, seed=5)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-100, reduction="sum")
    x["lang"] = model("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
    hs = [model("history").expand(TINY["B"], -1)]
    loss = 0.0
    for t in range(3):
        out = run_visual(model, x, torch.stack(hs, 1), torch.ones(TINY["B"], t + 1, dtype=torch.bool))
        loss = loss + ce(out[0], act_t) + ce(out[1], ref_t)
        hs.append(history(model, x, t))
    loss.backward()
    store["c/loss"] = np.array(float(loss.detach()), dtype=np.float64)
    names = [k for k, p in model.named_parameters() if p.grad is not None]
    store["c/grad_names"] = np.array(names)
    store["c/grad_norms"] = np.array([float(dict(model.named_parameters())[k].grad.double().norm()) for k in names])
    for k, p in model.named_parameters():
        if p.grad is not None and any(k.startswith(g) for g in GRAD_PROBES):
            store[f"c/probe/{k}"] = probe(p.grad)
    # (d): NavRefModel around the reference NavRefCMT
    for tag, no_lang_ca in (("d/nolangca", True), ("d/ca", False)):
        cfg = tiny_cfg(no_lang_ca)
        agent = mn.NavRefModel.__new__(mn.NavRefModel)
        torch.nn.Module.__init__(agent)
        agent.args = types.SimpleNamespace(no_lang_ca=no_lang_ca, feat_dropout=0.4)
        agent.vln_bert = build_ref(vn, cfg)
        agent.drop_env = torch.nn.Dropout(p=0.4)
        agent.eval()
        x = inputs(cfg, TINY)
        with torch.no_grad(), ref_shim.cuda_is_identity():
            lang = agent("language", txt_ids=x["txt_ids"], txt_masks=x["txt_masks"])
            hs = [agent("history").expand(TINY["B"], -1)]
            for t in range(3):
                hs.append(agent("history", hist_img_feats=x["hist_img_feats"][t], hist_ang_feats=x["hist_ang_feats"][t], ob_step=t,
                                hist_pano_img_feats=x["hist_pano_img_feats"][t], hist_pano_ang_feats=x["hist_pano_ang_feats"][t]))
            outs = agent("visual", txt_embeds=lang, txt_masks=x["txt_masks"], hist_embeds=hs, hist_lens=HIST_LENS[TINY["B"]],
                         ob_img_feats=x["ob_img_feats"], ob_ang_feats=x["ob_ang_feats"], ob_nav_types=x["ob_nav_types"],
                         ob_masks=x["ob_masks"], obj_feats=x["obj_feats"], obj_angles=x["obj_angles"], obj_poses=x["obj_poses"],
                         obj_masks=x["obj_masks"], return_states=True)
        assert sorted(outs) == ["act_logits", "obj_logits", "states"]
        for k, v in outs.items():
            store[f"{tag}/{k}"] = v.numpy().copy()
    # (e): one full-size forward
    cfg = full_cfg()
    model = build_ref(vn, cfg).eval()
    with torch.no_grad():
        outs = episode(model, inputs(cfg, FULL), FULL["B"])
    store["e/act_logits"], store["e/obj_logits"] = outs[0].numpy().copy(), outs[1].numpy().copy()
    for name, o in zip(("txt", "hist", "ob", "obj"), outs[2:]):
        store[f"e/probe/{name}"] = probe(o, 257)
    store["meta/sd_seed"] = np.array(SD_SEED)
    return store


def main():
    store = generate()
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME), **store)
    print(f"{NAME}: {len(store)} arrays, {os.path.getsize(os.path.join(OUT, NAME))} bytes")


if __name__ == "__main__":
    main()
