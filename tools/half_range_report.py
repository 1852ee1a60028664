#!/usr/bin/env python3
"""Which dense layers of a checkpoint reach half's limit?  Builds the pre-training model (R2R-canon config, or --tiny), optionally loads a
state_dict file, runs one synthetic batch per task under an audit.HalfRangeWatch and prints one row per dense layer that feeds a LayerNorm:

    python tools/half_range_report.py [--state-dict FILE] [--batch 8] [--tasks mlm,sap,...] [--promote] [--tiny]

`at_limit` counts output elements with |x| == 65504 -- what the clamped half store turns every overflow into (a value that merely rounds
to 65504 counts too) --, `nonfinite` inf / NaN, `max_abs` the largest finite magnitude, `calls` the audited launches.  --promote gives
the flagged layers fp32 outputs (HalfRangeWatch.promote_flagged) and runs the batches again to show what they really hold.  Exit
status 1 when a layer is flagged (after promotion: when one still is)."""
import argparse
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

TASKS = ("mlm", "sap", "sar", "sprel", "mrc", "itm")


def build_model(tiny, device):
    from vln_hamt_amd.model.pretrain_cmt import MultiStepNavCMTPreTraining
    from vln_hamt_amd.modeling import HamtConfig
    kw = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, image_feat_size=64, num_l_layers=2, num_x_layers=2,
              num_h_pano_layers=1, vocab_size=1000) if tiny else {}
    cfg = HamtConfig(hamt_precision="bf16", pretrain_tasks=set(TASKS), **kw)
    torch.manual_seed(0)
    return MultiStepNavCMTPreTraining(cfg).to(device).eval(), cfg


def run_tasks(model, cfg, tasks, bsz, device):
    from vln_hamt_amd.synth import make_batch, make_itm_rng
    with torch.no_grad():
        for i, task in enumerate(tasks):
            b = make_batch(task, bsz, cfg, seed=100 + i, txt_len=80, hist_len=5, device=device)
            if task == "itm":
                r = make_itm_rng(b, seed=i)
                b["itm_neg_idxs"], b["itm_shuffled_pos_ids"] = r["neg_idxs"], r["shuffled_pos_ids"]
            model(b, task, True)


def print_table(rows):
    w = max([len(r.name) for r in rows] + [4])
    print(f"{'site':<{w}}  {'at_limit':>9}  {'nonfinite':>9}  {'max_abs':>11}  {'calls':>6}")
    for r in rows:
        flag = "  <-- " + ("at half's limit" if r.at_limit else "non-finite") if (r.at_limit or r.nonfinite) else ""
        print(f"{r.name:<{w}}  {r.at_limit:>9}  {r.nonfinite:>9}  {r.max_abs:>11.5g}  {r.calls:>6}{flag}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--state-dict", default=None, help="a torch.save()d state_dict (or a checkpoint with one under 'state_dict' / 'model')")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tasks", default=",".join(TASKS))
    ap.add_argument("--promote", action="store_true")
    ap.add_argument("--tiny", action="store_true", help="a 128-wide two-layer model (a quick look at the tool itself)")
    args = ap.parse_args()
    from vln_hamt_amd import HalfRangeWatch
    from vln_hamt_amd._lib import HamtError
    if not torch.cuda.is_available():
        raise HamtError("half_range_report: needs a GPU (the HAMT kernels have no CPU path)")
    device = torch.device("cuda", 0)
    model, cfg = build_model(args.tiny, device)
    if args.state_dict:
        sd = torch.load(args.state_dict, map_location="cpu")
        for k in ("state_dict", "model"):
            if isinstance(sd, dict) and k in sd and isinstance(sd[k], dict):
                sd = sd[k]
        res = model.load_state_dict(sd, strict=False)
        print(f"loaded {args.state_dict}: {len(res.missing_keys)} missing, {len(res.unexpected_keys)} unexpected key(s)")
    tasks = [t for t in args.tasks.split(",") if t]
    watch = HalfRangeWatch(model)
    with watch:
        run_tasks(model, cfg, tasks, args.batch, device)
    print_table(watch.report())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bad = watch.check()
    if bad and args.promote:
        watch.promote(bad)
        watch.reset()
        with watch:
            run_tasks(model, cfg, tasks, args.batch, device)
        print(f"\nafter promoting {len(bad)} layer(s) to fp32 outputs:")
        print_table(watch.report())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bad = watch.check()
    print(f"{len(bad)} layer(s) flagged" + (": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
