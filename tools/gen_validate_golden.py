#!/usr/bin/env python3
"""Generate tests/golden/validate.npz by running the REFERENCE's own validation functions (pretrain_src/main_r2r.py: validate_mlm,
validate_sap, validate_sar, validate_sprel, compute_accuracy_for_soft_targets, validate_mrc, validate_itm) on scripted model outputs,
CPU, fp32.

Test infrastructure, like tools/gen_policy_step_golden.py (needs the reference checkout, oracle.ref_shim.REF):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_validate_golden.py

main_r2r.py cannot be imported (it pulls in the whole training script: horovod-style launchers, the tensorboard logger, the data
loaders), so the seven function definitions are cut out of the reference FILE with `ast` at generation time and compiled with torch,
F, time, a silent LOGGER and `all_gather = lambda x: [x]` -- nothing of them is restated or stored here.  The model is a stand-in that
returns the scripted outputs batch by batch.  The fixture holds the scripted scores, labels, targets and masks and the returned
numbers; the 30 522-wide MLM rows are regenerated from a seed (tests/_eval_ref.py::mlm_scripted_scores), only their labels are stored.

Three batches per task with different row counts, one of them with zero rows.  The generator asserts on its own inputs that the two
largest logits of every finite CE / KL row are bit-equal (the scripted ties) or more than 64 fp32 ulps of max(1, |lse|, max |x|) apart:
fp32 log_softmax cannot merge them, so the reference's arg-max is the mathematical one.
"""
import ast
import logging
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from oracle import ref_shim                                            # noqa: E402
from _eval_ref import MLM_C, mlm_scripted_scores, top_two_gap_ok       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "validate.npz")
NAMES = ("validate_mlm", "validate_sap", "validate_sar", "validate_sprel", "compute_accuracy_for_soft_targets", "validate_mrc", "validate_itm")
F32 = np.float32


def reference_functions():
    path = os.path.join(ref_shim.REF, "pretrain_src", "main_r2r.py")
    src = open(path).read()
    tree = ast.parse(src)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(d.name for d in defs) == sorted(NAMES), [d.name for d in defs]
    silent = logging.getLogger("gen_validate_golden.reference")
    silent.addHandler(logging.NullHandler())
    silent.propagate = False
    env = {"torch": torch, "F": F, "time": time, "LOGGER": silent, "all_gather": lambda x: [x]}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), env)
    return {n: env[n] for n in NAMES}


class Scripted:
    """model(batch, task, compute_loss=False) -> the scripted output of batch['i']"""

    def __init__(self, outputs):
        self.outputs = outputs

    def __call__(self, batch, task, compute_loss=True):
        assert compute_loss is False
        o = self.outputs[int(batch["i"])]
        return tuple(torch.from_numpy(a) for a in o) if isinstance(o, tuple) else torch.from_numpy(o)


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def script_mlm(store):
    """txt_labels [B, L] with -1 = no label; rows 7, 0, 4 of 30 522 logits (in every second row the label is the arg-max)"""
    rng = rng_of(1)
    outs, batches = [], []
    for i, (B, L, n) in enumerate(((3, 9, 7), (2, 6, 0), (2, 8, 4))):
        lab = np.full(B * L, -1, dtype=np.int64)
        lab[rng.permutation(B * L)[:n]] = rng.integers(1996, 29611, size=n)
        lab = lab.reshape(B, L)
        seed = 5000 + i
        x = mlm_scripted_scores(seed, lab[lab != -1])
        assert x.shape == (n, MLM_C) and top_two_gap_ok(x)
        store[f"mlm/{i}/txt_labels"], store[f"mlm/{i}/seed"] = lab, np.int64(seed)
        outs.append(x)
        batches.append({"i": i, "txt_labels": torch.from_numpy(lab)})
    return outs, batches


def sap_rows(rng, R, C=37):
    x = (2 * rng.standard_normal((R, C))).astype(F32)
    for r in range(R):
        x[r, rng.permutation(C - 1)[:int(rng.integers(20, 32))]] = -np.inf     # padding columns; the STOP column C - 1 stays
    return x


def script_sap(store):
    """C = 37 with -inf padding; batch 0 row 1: the label sits on the largest logit, exactly tied with a LATER column"""
    rng = rng_of(2)
    outs, batches = [], []
    for i, R in enumerate((5, 3, 0)):
        x = sap_rows(rng, R)
        lab = np.array([int(rng.choice(np.flatnonzero(np.isfinite(x[r])))) for r in range(R)], dtype=np.int64)
        if i == 0:
            fin = np.flatnonzero(np.isfinite(x[1]))
            lo, hi = int(fin[0]), int(fin[-1])
            x[1, lo] = F32(x[1, fin].max() + 1.0)
            x[1, hi] = x[1, lo]
            lab[1] = lo
            lab[3] = int(np.argmax(x[3]))                                       # an ordinary correct row
        assert top_two_gap_ok(x)
        store[f"sap/{i}/scores"], store[f"sap/{i}/labels"] = x, lab
        outs.append(x)
        batches.append({"i": i, "ob_action_viewindex": torch.from_numpy(lab)})
    return outs, batches


def script_sapnan(store):
    """the separate SAP case: an all -inf row (labelled 0, which is also its arg-max) and a label on a -inf column"""
    rng = rng_of(3)
    x = sap_rows(rng, 4)
    lab = np.array([int(np.argmax(x[r])) for r in range(4)], dtype=np.int64)
    x[1] = -np.inf
    lab[1] = 0
    lab[2] = int(np.flatnonzero(np.isinf(x[2]))[0])
    store["sapnan/0/scores"], store["sapnan/0/labels"] = x, lab
    return [x], [{"i": 0, "ob_action_viewindex": torch.from_numpy(lab)}]


def script_itm(store):
    rng = rng_of(4)
    outs, batches = [], []
    for i, R in enumerate((4, 0, 7)):
        x = (1.5 * rng.standard_normal((R, 5))).astype(F32)
        assert top_two_gap_ok(x)
        store[f"itm/{i}/scores"] = x
        outs.append((x, np.zeros(R, dtype=np.int64)))
        batches.append({"i": i})
    return outs, batches


def script_mrc(store):
    """C = 1000; batch 0: row 0 an all-zero target, row 1 a one-hot target, row 2 prediction and target arg-max agree"""
    rng = rng_of(5)
    outs, batches = [], []
    for i, (B, T, R) in enumerate(((3, 4, 6), (2, 3, 0), (2, 5, 3))):
        x = (2 * rng.standard_normal((R, 1000))).astype(F32)
        z = 2 * rng.standard_normal((R, 1000))
        t = np.exp(z - z.max(axis=1, keepdims=True)) if R else z
        t = (t / t.sum(axis=1, keepdims=True)).astype(F32) if R else z.astype(F32)
        if i == 0:
            t[0] = 0
            t[1] = 0
            t[1, 421] = 1.0
            x[2, int(np.argmax(t[2]))] = F32(x[2].max() + 2.0)
            x[1, 421] = F32(x[1].max() + 2.0)
        assert top_two_gap_ok(x)
        m = np.zeros(B * T, dtype=bool)
        m[rng.permutation(B * T)[:R]] = True
        store[f"mrc/{i}/scores"], store[f"mrc/{i}/targets"], store[f"mrc/{i}/hist_mrc_masks"] = x, t, m.reshape(B, T)
        outs.append((x, t))
        batches.append({"i": i, "hist_mrc_masks": torch.from_numpy(m.reshape(B, T))})
    return outs, batches


def _two_scales(rng, shape):
    a = rng.standard_normal(shape)
    a[..., 0] *= np.where(np.arange(shape[0]) % 2 == 0, 1e-3, 1e3).reshape((-1,) + (1,) * (len(shape) - 2)) if shape[0] else 1.0
    return a.astype(F32)


def script_sar(store):
    rng = rng_of(6)
    outs, batches = [], []
    for i, R in enumerate((5, 0, 8)):
        x, t = _two_scales(rng, (R, 3)), _two_scales(rng, (R, 3))
        store[f"sar/{i}/scores"], store[f"sar/{i}/ob_action_angles"], store[f"sar/{i}/ob_progress"] = x, t[:, :2].copy(), t[:, 2].copy()
        outs.append(x)
        batches.append({"i": i, "ob_action_angles": torch.from_numpy(t[:, :2].copy()), "ob_progress": torch.from_numpy(t[:, 2].copy())})
    return outs, batches


def script_sprel(store, tag, shapes):
    rng = rng_of(7 if tag == "sprel" else 8)
    outs, batches = [], []
    for i, shape in enumerate(shapes):
        x, t = _two_scales(rng, shape), _two_scales(rng, shape)
        store[f"{tag}/{i}/scores"], store[f"{tag}/{i}/sp_targets"] = x, t
        outs.append(x)
        batches.append({"i": i, "sp_targets": torch.from_numpy(t)})
    return outs, batches


def main():
    ref = reference_functions()
    store = {}
    plan = [("mlm", "validate_mlm", script_mlm(store)), ("sap", "validate_sap", script_sap(store)),
            ("sapnan", "validate_sap", script_sapnan(store)), ("itm", "validate_itm", script_itm(store)),
            ("mrc", "validate_mrc", script_mrc(store)), ("sar", "validate_sar", script_sar(store)),
            # SPREL: [R, 2] scores (R = 2 x 36, 0, 36: the two columns), and the model's own [B, 36, 2] (views 0 and 1 of every sample)
            ("sprel", "validate_sprel", script_sprel(store, "sprel", ((72, 2), (0, 2), (36, 2)))),
            ("sprel3d", "validate_sprel", script_sprel(store, "sprel3d", ((3, 36, 2), (0, 36, 2), (2, 36, 2))))]
    for tag, fn, (outs, batches) in plan:
        log = ref[fn](Scripted(outs), batches)
        store[f"{tag}/n_batches"] = np.int64(len(batches))
        for k, v in log.items():
            if not k.endswith("_per_s"):                         # (wall-clock throughput is not a result)
                store[f"{tag}/want/{k}"] = np.float64(v)
        print(tag, {k: v for k, v in log.items() if not k.endswith("_per_s")})
    assert np.isnan(store["sapnan/want/loss"]) or np.isinf(store["sapnan/want/loss"])
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
