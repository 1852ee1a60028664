#!/usr/bin/env python3
"""View-feature extraction on synthetic panoramas, ViT-B/16, 576 views (16 viewpoints) per batch:

  (a) backbone, `forward_features(rows)`                  -- the full last block
  (b) backbone, `forward_features(rows, cls_tail=True)`   -- K / V for all tokens, everything else for the cls rows
      alternating a, b, a, b, ... in one process on the same prepared patch rows; median and range of `--rounds` rounds of
      `--reps` passes each (device-synchronised host clock), after a warm-up of both;
  (c) the whole `build_feature_file` (host reads, pinned double buffer, image prep, backbone, head, writer to an .npz) in views/s.

    python tools/extract_bench.py [--rounds 7] [--reps 4] [--viewpoints 64] [--precision bf16]

Random weights (a timing does not depend on them).  Writes profiles/extract_mi355x.json and prints it.  Condition: (b) <= (a)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402

from vln_hamt_amd.data.image_data import SyntheticPanoStore                          # noqa: E402
from vln_hamt_amd.data.image_prep import image_prep                                  # noqa: E402
from vln_hamt_amd.model.vision_transformer import vit_base_patch16_224               # noqa: E402
from vln_hamt_amd.preprocess import ViewFeatureExtractor, build_feature_file         # noqa: E402

VIEWS = 576
# FLOPs of one view (multiply-add = 2): 12 blocks of qkv + proj + fc1 + fc2 on 197 tokens and the two attention products, + the patch GEMM
H, S = 768, 197
BLOCK = 2 * S * (3 * H * H + H * H + 8 * H * H) + 2 * 2 * S * S * H
FULL = 12 * BLOCK + 2 * 196 * H * H
TAIL = 2 * S * 2 * H * H + 2 * (H * H + H * H + 8 * H * H) + 2 * 2 * S * H           # K, V for all tokens; q, proj, MLP and attention for one
PREDICTED = (BLOCK - TAIL) / FULL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--viewpoints", type=int, default=64)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_mi355x.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "extract_bench.py measures on the GPU (a CPU run has no rate to report)"
    assert a.rounds >= 5
    torch.manual_seed(0)
    model = vit_base_patch16_224(hamt_precision=a.precision, num_classes=1000).cuda().eval()
    ex = {tail: ViewFeatureExtractor(model, cls_tail=tail) for tail in (False, True)}
    store = SyntheticPanoStore(seed=3, cache=a.viewpoints + 1)
    keys = [("scan%d" % (i // 8), "vp%02d" % i) for i in range(a.viewpoints)]
    views = torch.from_numpy(np.concatenate([store.get("%s_%s" % k) for k in keys[:VIEWS // 36]], 0)).cuda()
    recs, recs_dev = ex[True]._records(VIEWS, views.shape[1], views.shape[2], views.device)
    rows = image_prep(views, recs, recs_dev, layout="patches", dtype=torch.bfloat16 if a.precision == "bf16" else torch.float32)

    def cell(tail):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(a.reps):
                model.forward_features(rows, cls_tail=tail)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    with torch.no_grad():
        fa, fb = model.forward_features(rows), model.forward_features(rows, cls_tail=True)
    diff = float((fa - fb).abs().max()) / max(1.0, float(fa.abs().max()))
    for tail in (False, True):
        cell(tail)
    ms = {False: [], True: []}
    for _ in range(a.rounds):
        for tail in (False, True):
            ms[tail].append(cell(tail))
    med = {t: statistics.median(v) for t, v in ms.items()}
    res = {"tool": "extract_bench.py", "device": torch.cuda.get_device_name(0), "precision": a.precision, "views_per_batch": VIEWS,
           "rounds": a.rounds, "reps_per_round": a.reps,
           "backbone_full_ms": {"median": med[False], "min": min(ms[False]), "max": max(ms[False])},
           "backbone_cls_tail_ms": {"median": med[True], "min": min(ms[True]), "max": max(ms[True])},
           "backbone_full_views_per_s": VIEWS / med[False] * 1e3, "backbone_cls_tail_views_per_s": VIEWS / med[True] * 1e3,
           "cls_tail_saving": 1.0 - med[True] / med[False], "flop_count_predicts": PREDICTED,
           "cls_tail_vs_full_max_rel_diff": diff}
    # (c) the whole file: every panorama generated beforehand, so that the host side is the read + gather + copy a real store costs
    for k in keys:
        store.get("%s_%s" % k)
    with tempfile.TemporaryDirectory() as tmp:
        for tail in (False, True):
            build_feature_file(store, keys[:16], os.path.join(tmp, "warm.npz"), ex[tail], out_image_logits=True, batch_size=VIEWS)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            build_feature_file(store, keys, os.path.join(tmp, "f.npz"), ex[tail], out_image_logits=True, batch_size=VIEWS)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res["build_feature_file_%s_views_per_s" % ("cls_tail" if tail else "full")] = a.viewpoints * 36 / dt
    res["build_feature_file_viewpoints"] = a.viewpoints
    res["condition_cls_tail_not_slower"] = bool(med[True] <= med[False])
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    assert res["condition_cls_tail_not_slower"], "cls_tail is slower than the full last block"


if __name__ == "__main__":
    main()
