#!/usr/bin/env python3
"""The proxy-task validation pass (pretrain_src/main_r2r.py:344-511) on the R2R-canon model, bf16, validation batch 64, 20 synthetic
batches per task:

  aten     the reference's statement sequence as torch ops on this project's model -- what a caller runs today: cross_entropy(sum) /
           max / == / sum with an `.item()` each, boolean indexing of the MLM labels, once per batch;
  device   vln_hamt_amd.validate.validate_* (one ops.eval_* call per batch, one read per pass).

    python tools/validate_bench.py [--out profiles/validate_mi355x.json]

Both paths alternate round by round in one process; a pass is timed with the host clock around work that ends in a device synchronise
(the aten path's last `.item()`, the device path's read, then torch.cuda.synchronize()); the median and the range over 5 rounds are
reported.  `forward+loss` times whole passes; `loss_only` replaces the model by its precomputed outputs, which leaves the loss /
accuracy side alone; `launches_per_batch` counts the device kernels of the loss-only pass with torch.profiler (in a run of its own,
after the timing).  The condition is device <= aten per task.  A host without a GPU fails: nothing here is measured on a CPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

TASKS = ("mlm", "sap", "sar", "sprel", "mrc", "itm")


# ------------------------------------------------------------------------------------------ the aten path (main_r2r.py as written)
def aten_pass(model, task, loader):
    tot = [0.0, 0.0, 0.0]
    n_correct = n = 0
    with torch.no_grad():
        for batch in loader:
            out = model(batch, task=task, compute_loss=False)
            if task in ("mlm", "sap", "itm"):
                if task == "mlm":
                    scores, labels = out, batch["txt_labels"]
                    labels = labels[labels != -1]
                elif task == "sap":
                    scores, labels = out, batch["ob_action_viewindex"]
                else:
                    scores, labels = out
                tot[0] += F.cross_entropy(scores, labels, reduction="sum").item()
                n_correct += (scores.max(dim=-1)[1] == labels).sum().item()
                n += labels.numel()
            elif task == "mrc":
                pred, tgt = out
                pred = F.log_softmax(pred, dim=-1)
                loss = F.kl_div(pred, tgt, reduction="sum")
                n_correct += (pred.max(dim=-1)[1] == tgt.max(dim=-1)[1]).sum().item()
                tot[0] += loss.item()
                n += batch["hist_mrc_masks"].sum().item()
            else:
                tg = ([batch["ob_action_angles"][:, 0], batch["ob_action_angles"][:, 1], batch["ob_progress"]] if task == "sar"
                      else [batch["sp_targets"][:, 0], batch["sp_targets"][:, 1]])
                for j, t in enumerate(tg):
                    tot[j] += F.mse_loss(out[:, j], t, reduction="sum").item()
                n += out.size(0)
    return [t / n for t in tot], n_correct / n


class Replay:
    """the model's precomputed outputs, batch by batch: the loss / accuracy side alone"""

    def __init__(self, outputs):
        self.outputs, self.i = outputs, 0

    def __call__(self, batch, task, compute_loss=True):
        out = self.outputs[self.i % len(self.outputs)]
        self.i += 1
        return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def count_launches(fn, n_batches):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    copies = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" in e.name.lower()]
    return {"kernels_per_batch": len(kernels) / n_batches, "copies_per_batch": len(copies) / n_batches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prec", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("validate_bench: no GPU; nothing is measured on a CPU")
    from vln_hamt_amd import validate as V
    from vln_hamt_amd.model.pretrain_cmt import MultiStepNavCMTPreTraining
    from vln_hamt_amd.modeling import HamtConfig
    from vln_hamt_amd.synth import make_batch, make_itm_rng
    dev = "cuda"
    cfg = HamtConfig(hamt_precision=args.prec, pretrain_tasks=set(TASKS))
    torch.manual_seed(0)
    model = MultiStepNavCMTPreTraining(cfg).to(dev).eval()
    fns = {"mlm": V.validate_mlm, "sap": V.validate_sap, "sar": V.validate_sar, "sprel": V.validate_sprel, "mrc": V.validate_mrc, "itm": V.validate_itm}
    result = {"device": torch.cuda.get_device_name(0), "prec": args.prec, "batch": args.batch, "batches_per_task": args.batches, "rounds": args.rounds,
              "unit": "ms per pass", "tasks": {}}
    for ti, task in enumerate(TASKS):
        loader = []
        for i in range(args.batches):
            b = make_batch(task, args.batch, cfg, seed=9000 + 100 * ti + i, txt_len=80, hist_len=5, ragged=True, device=dev)
            if task == "itm":
                r = make_itm_rng(b, seed=i)
                b["itm_neg_idxs"], b["itm_shuffled_pos_ids"] = r["neg_idxs"], r["shuffled_pos_ids"]
            loader.append(b)
        with torch.no_grad():
            outputs = [model(b, task=task, compute_loss=False) for b in loader]
        replay = lambda: Replay(outputs)
        cells = {"forward+loss": (lambda: aten_pass(model, task, loader), lambda: fns[task](model, loader)),
                 "loss_only": (lambda: aten_pass(replay(), task, loader), lambda: fns[task](replay(), loader))}
        row = {}
        for cell, (aten, device) in cells.items():
            aten(), device()                                        # warm-up of every shape in the window
            ts = {"aten": [], "device": []}
            for _ in range(args.rounds):
                ts["aten"].append(timed(aten)[0])
                ts["device"].append(timed(device)[0])
            row[cell] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ts.items()}
            row[cell]["device_le_aten"] = row[cell]["device"]["median"] <= row[cell]["aten"]["median"]
        (a_loss, a_acc), d = aten_pass(replay(), task, loader), fns[task](replay(), loader)
        row["agreement"] = {"aten": {"loss": a_loss, "acc": a_acc}, "device": {k: v for k, v in d.items() if not k.endswith("_per_s")}}
        row["launches_per_batch"] = {"aten": count_launches(cells["loss_only"][0], args.batches), "device": count_launches(cells["loss_only"][1], args.batches)}
        result["tasks"][task] = row
        print(task, json.dumps(row), flush=True)
    result["device_le_aten_all"] = all(result["tasks"][t][c]["device_le_aten"] for t in TASKS for c in ("forward+loss", "loss_only"))
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
