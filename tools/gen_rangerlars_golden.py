#!/usr/bin/env python3
"""Generate tests/golden/rangerlars_tiny.npz by running the REFERENCE's own optim.rangerlars (Ralamb + Lookahead) on CPU.

Test infrastructure, like oracle/gen_goldens.py:gen_optim (needs the reference checkout, oracle.ref_shim.REF):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_rangerlars_golden.py

Tiny pretrain model in fp32, dropout off, the reference's decay groups (weight decay 0.01), lr 5e-3 under lr_at(step, 5e-3, 2, 20),
clip 5.0, betas (0.9, 0.98); the pre-loop step() of main_r2r.py:229-230, then 17 training steps over TASKS.  With the pre-loop step
the Lookahead syncs (k = 6) fall on training steps 5 (the slow buffers of the parameters with a gradient are created), 11 and 17.
The task list covers the corners of the lazy slow-buffer creation (lookahead.py:29-39); the generator asserts each of them.

The reference's Lookahead never calls Optimizer.__init__, so under torch 2 its step() misses the hook dictionaries: they are set,
empty, on the instance (nothing else is changed).
"""
import importlib
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import ref_shim                                                   # noqa: E402
from oracle.gen_goldens import build_ref_pretrain                             # noqa: E402
from oracle.hamt_oracle import OracleConfig, lr_at, make_state_dict, pretrain_param_shapes  # noqa: E402
from vln_hamt_amd.synth import make_batch                                     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NAME = "rangerlars_tiny.npz"
TASKS = "sap mlm sap sprel sap mrc sap mlm sar sprel mlm sap mrc sap sar mrc sap".split()
SYNCS = (5, 11, 17)
PROBES = ["bert.encoder.x_layers.0.visual_attention.att.query.weight", "bert.encoder.layer.1.output.dense.bias",
          "bert.embeddings.LayerNorm.weight", "bert.img_embeddings.layer_norm.weight", "bert.hist_embeddings.cls_token",
          "mlm_head.predictions.transform.dense.weight", "next_action.net.2.weight", "next_action.net.4.bias",
          "sprel_head.net.0.weight", "image_classifier.net.0.weight", "regress_action.net.0.bias"]
NO_DECAY = ['bias', 'LayerNorm.bias', 'LayerNorm.weight']
PROBE_N = 512


def probe(t):
    """an evenly strided probe of at most PROBE_N elements of a parameter (keeps the fixture small)"""
    f = t.detach().reshape(-1)
    return f[:: max(1, f.numel() // PROBE_N)][:PROBE_N].numpy().copy()


def batch_for(step, cfg):
    return make_batch(TASKS[step - 1], 3, cfg, seed=200 + step, txt_len=20, hist_len=4, ragged=True)


def import_ref_optim():
    sys.path.insert(0, os.path.join(ref_shim.REF, "pretrain_src"))
    for k in [k for k in sys.modules if k == "optim" or k.startswith("optim.")]:
        del sys.modules[k]
    try:
        return importlib.import_module("optim.rangerlars"), importlib.import_module("optim.sched")
    finally:
        sys.path.pop(0)


def generate():
    ref_rl, ref_sched = import_ref_optim()
    torch.manual_seed(0)
    cfg = OracleConfig.tiny(hidden_size=128, num_attention_heads=2, intermediate_size=256, image_feat_size=64)
    sd = make_state_dict(pretrain_param_shapes(cfg), seed=7)
    model, _ = build_ref_pretrain(cfg, sd)
    named = list(model.named_parameters())
    names = [n for n, _ in named]
    groups = [{'params': [p for n, p in named if not any(nd in n for nd in NO_DECAY)], 'weight_decay': 0.01},
              {'params': [p for n, p in named if any(nd in n for nd in NO_DECAY)], 'weight_decay': 0.0}]
    opt = ref_rl.RangerLars(groups, lr=5e-3, betas=(0.9, 0.98))
    opt._optimizer_step_pre_hooks = OrderedDict()
    opt._optimizer_step_post_hooks = OrderedDict()

    class O:  # opts namespace for get_lr_sched
        learning_rate, warmup_steps, num_train_steps = 5e-3, 2, 20
    store = {"meta/names": np.array(names), "meta/decay_names": np.array([n for n in names if not any(nd in n for nd in NO_DECAY)]),
             "meta/tasks": np.array(TASKS), "meta/sd_seed": np.array(7), "meta/probe_n": np.array(PROBE_N)}
    slot = {id(p): i for i, (_, p) in enumerate(named)}

    def record(pre):
        steps = np.zeros(len(names), dtype=np.int64)
        wn, an, tr = (np.zeros(len(names), dtype=np.float32) for _ in range(3))
        for p, st in opt.base_optimizer.state.items():
            i = slot[id(p)]
            steps[i] = st["step"]
            wn[i], an[i], tr[i] = float(st["weight_norm"]), float(st["adam_norm"]), float(st["trust_ratio"])
        slow = np.zeros(len(names), dtype=bool)
        for p, st in opt.state.items():
            if "slow_buffer" in st:
                slow[slot[id(p)]] = True
        store[pre + "step"], store[pre + "weight_norm"], store[pre + "adam_norm"], store[pre + "trust_ratio"] = steps, wn, an, tr
        store[pre + "has_slow"] = slow
        store[pre + "lookahead_step"] = np.array([g["lookahead_step"] for g in opt.param_groups], dtype=np.int64)

    opt.zero_grad()
    opt.step()                                   # main_r2r.py:230: no gradients, the Lookahead counter advances
    record("step0/")
    active = {}
    for step in range(1, len(TASKS) + 1):
        task = TASKS[step - 1]
        loss = model(batch_for(step, cfg), task, True).mean()
        loss.backward()
        lr = ref_sched.get_lr_sched(step, O)
        assert abs(lr - lr_at(step, 5e-3, 2, 20)) < 1e-15
        for g in opt.param_groups:
            g['lr'] = lr
        gn = torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
        active[step] = np.array([p.grad is not None for _, p in named])
        opt.step()
        opt.zero_grad()
        pre = f"step{step}/"
        store[pre + "loss"] = np.float64(loss.item())
        store[pre + "grad_norm"] = np.float64(gn.item())
        store[pre + "lr"] = np.float64(lr)
        store[pre + "active"] = active[step]
        for k in PROBES:
            store[pre + "param/" + k] = probe(dict(named)[k])
        record(pre)

    # the corners of lookahead.py:29-39 this task list must reach
    a5, a11, a17 = (active[s] for s in SYNCS)
    groups_ = {"interpolate at 11 and 17": a5 & a11 & a17,
               "first slow buffer at 11 or 17": ~a5 & (a11 | a17),
               "slow buffer, then skipped at a later sync": (a5 & (~a11 | ~a17)) | (a11 & ~a17),
               "never sync": ~a5 & ~a11 & ~a17}
    for what, sel in groups_.items():
        assert sel.any(), what
        print(f"  {what}: {int(sel.sum())} parameters, e.g. {names[int(np.argmax(sel))]}")
    assert np.array_equal(store["step17/has_slow"], a5 | a11 | a17)
    return store


def main():
    store = generate()
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME), **store)
    print(f"{NAME}: {len(store)} arrays, {os.path.getsize(os.path.join(OUT, NAME))} bytes")


if __name__ == "__main__":
    main()
