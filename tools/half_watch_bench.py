#!/usr/bin/env python3
"""What audit.HalfRangeWatch costs (-> profiles/half_watch_mi355x.json):

  * the eager B = 64 training step (graph.GraphedTrainStep._eager: forward, backward, clip, AdamW) over the six tasks with the watch
    enabled and disabled, alternating in one process, median of --reps; the audit launches per step, counted from the records;
  * the audit kernel alone, by device events, over a rotation of [5120, 768] half buffers larger than the 256 MB last-level cache (every
    launch reads HBM): microseconds per launch and bytes per second.

    python tools/half_watch_bench.py [--batch 64] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

TASKS = ("mlm", "sap", "sar", "sprel", "mrc", "itm")


def kernel_rate(device, M=5120, N=768, cache_mb=256, rounds=5):
    from vln_hamt_amd import ops
    per = M * N * 2
    n_buf = (2 * cache_mb * 2 ** 20) // per + 1                      # twice the cache: a buffer is long gone when its turn comes again
    bufs = [(torch.randn(M, N, device=device) * 30).to(torch.float16) for _ in range(n_buf)]
    rec = torch.zeros(ops.RANGE_REC, dtype=torch.int64, device=device)
    for b in bufs[:4]:
        ops.range_audit(b, rec)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for b in bufs:
            ops.range_audit(b, rec)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / n_buf)               # ms per launch
    # one launch between two events, per buffer: the kernel without the back-to-back launch rate of the host
    singles = []
    for b in bufs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ops.range_audit(b, rec); e1.record(); e1.synchronize()
        singles.append(e0.elapsed_time(e1))
    # the same pass as a captured graph: the eager loop above runs at the host's launch rate (a ctypes call from Python per kernel)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        for b in bufs:
            ops.range_audit(b, rec)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    graphed = 1e9
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); e1.synchronize()
        graphed = min(graphed, e0.elapsed_time(e1) / n_buf)
    r = rec.cpu().tolist()
    assert r[0] == 0 and r[1] == 0 and r[3] == 4 + (2 * rounds + 2) * n_buf, r
    return {"shape": [M, N], "dtype": "float16", "buffers": n_buf, "rotation_mb": round(n_buf * per / 2 ** 20, 1),
            "us_per_launch_graph_replay": round(graphed * 1e3, 2), "gb_per_s_graph_replay": round(per / (graphed * 1e-3) / 1e9, 1),
            "us_per_launch_back_to_back": round(best * 1e3, 2), "gb_per_s_back_to_back": round(per / (best * 1e-3) / 1e9, 1),
            "us_single_launch_median": round(statistics.median(singles) * 1e3, 2),
            "gb_per_s_single_launch": round(per / (statistics.median(singles) * 1e-3) / 1e9, 1),
            "how": "HIP events; graph replay / back to back = one event pair around a pass over the rotation (a captured graph of it / eager "
                   "launches from Python, which run at the host's launch rate), best of %d; single = one pair per launch, median" % rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from vln_hamt_amd import HalfRangeWatch, ops
    from vln_hamt_amd.graph import GraphedTrainStep
    from vln_hamt_amd.optim import AdamW
    from vln_hamt_amd.optim.misc import NO_DECAY
    from vln_hamt_amd.synth import make_batch, make_itm_rng
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    ops.manual_seed(1234, device)
    out = {"device": torch.cuda.get_device_name(device), "kernel": kernel_rate(device)}
    print(json.dumps(out["kernel"]), flush=True)

    model, cfg = bench.build_model("bf16", device)
    named = list(model.named_parameters())
    opt = AdamW([{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
                 {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}], lr=5e-5, betas=(0.9, 0.98))
    opt.materialize()
    stepper = GraphedTrainStep(model, opt, max_grad_norm=5.0)
    batches = []
    for i, task in enumerate(TASKS):
        b = make_batch(task, args.batch, cfg, seed=1234 + 7919 * i, txt_len=bench.L_TXT, hist_len=bench.T_HIST,
                       mlm_exact=12 if task == "mlm" else None, device=device)
        if task == "itm":
            r = make_itm_rng(b, seed=i)
            b["itm_neg_idxs"], b["itm_shuffled_pos_ids"] = r["neg_idxs"], r["shuffled_pos_ids"]
        batches.append((task, b))

    def six_steps():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for task, b in batches:
            stepper._eager(b, task)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(batches)

    watch = HalfRangeWatch(model)
    for _ in range(2):                                              # warm-up, both ways
        six_steps()
        with watch:
            six_steps()
    watch.reset()
    on, off = [], []
    for _ in range(args.reps):
        off.append(six_steps())
        with watch:
            on.append(six_steps())
    rows = watch.report()
    launches = sum(r.calls for r in rows) / (args.reps * len(batches))
    flagged = [r.name for r in rows if r.at_limit or r.nonfinite]
    out["eager_step"] = {"batch": args.batch, "tasks": list(TASKS), "reps": args.reps,
                         "ms_per_step_watch_off": [round(v, 3) for v in off], "ms_per_step_watch_on": [round(v, 3) for v in on],
                         "median_off": round(statistics.median(off), 3), "median_on": round(statistics.median(on), 3),
                         "audit_launches_per_step": round(launches, 2), "sites": len(rows), "flagged": flagged,
                         "largest_max_abs": max(r.max_abs for r in rows),
                         "how": "forward + backward + clip + AdamW, eager launches, mean over one step of each of the six tasks; off / on alternate"}
    print(json.dumps(out["eager_step"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
