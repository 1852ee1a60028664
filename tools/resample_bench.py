#!/usr/bin/env python3
"""The whole-view resample on one panorama of raw renders, 36 views of 480 x 640, next to the backbone that follows it:

  (i)   `image_resample`, Lanczos, to 248 x 330          -- what `build_image_store` runs
  (ii)  `image_resample`, bicubic, centre 224 x 224      -- what the extractor runs in front of the backbone (`resize="bicubic"`)
  (b)   ViT-B/16 `forward_features(rows, cls_tail=True)` on the same 36 views (patch rows prepared beforehand)
      alternating i, ii, b, i, ii, b, ... in one process; median and range of `--rounds` rounds of `--reps` launches each
      (device-synchronised host clock), after a warm-up of all three.  Effective bytes/s = the 33 MB of renders over the time.
  (c)   `build_feature_file` in views/s from raw renders (`resize="bicubic"`) and, in the same process, from stored 248 x 330 views;
  (d)   `build_image_store` in views/s (directory of .npy in a temporary directory).

    python tools/resample_bench.py [--rounds 9] [--reps 200] [--viewpoints 32] [--precision bf16]

Random weights and random bytes (a timing depends on neither).  Writes profiles/image_resample_mi355x.json and prints it."""
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
from vln_hamt_amd.data.image_resample import image_resample                          # noqa: E402
from vln_hamt_amd.data.image_transform import eval_resize_geometry                   # noqa: E402
from vln_hamt_amd.model.vision_transformer import vit_base_patch16_224               # noqa: E402
from vln_hamt_amd.preprocess import ViewFeatureExtractor, build_feature_file, build_image_store     # noqa: E402

N, H, W = 36, 480, 640


class RenderStore:
    """`get(key) -> uint8 (36, 480, 640, 3)`: random bytes, every panorama made beforehand"""

    def __init__(self, keys):
        g = np.random.Generator(np.random.PCG64(11))
        self.d = {k: g.integers(0, 256, (N, H, W, 3), dtype=np.uint8) for k in keys}

    def get(self, key):
        return self.d[key]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--viewpoints", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_resample_mi355x.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resample_bench.py measures on the GPU (a CPU run has no rate to report)"
    assert a.rounds >= 5
    torch.manual_seed(0)
    model = vit_base_patch16_224(hamt_precision=a.precision, num_classes=1000).cuda().eval()
    ex_raw, ex = ViewFeatureExtractor(model, resize="bicubic"), ViewFeatureExtractor(model)
    keys = [("scan%d" % (i // 8), "vp%02d" % i) for i in range(a.viewpoints)]
    renders = RenderStore(["%s_%s" % k for k in keys])
    src = torch.from_numpy(renders.get("%s_%s" % keys[0])).cuda()
    OH, OW, window = eval_resize_geometry(H, W)
    out_i = torch.empty((N, OH, OW, 3), dtype=torch.uint8, device="cuda")
    out_ii = torch.empty((N, 224, 224, 3), dtype=torch.uint8, device="cuda")
    recs, recs_dev = ex_raw._records(N, 224, 224, src.device, identity=True)
    rows = image_prep(image_resample(src, (OH, OW), "bicubic", window), recs, recs_dev, layout="patches",
                      dtype=torch.bfloat16 if a.precision == "bf16" else torch.float32)

    def run(what):
        if what == "lanczos_248x330":
            image_resample(src, (OH, OW), "lanczos", out=out_i)
        elif what == "bicubic_centre_224":
            image_resample(src, (OH, OW), "bicubic", window, out=out_ii)
        else:
            model.forward_features(rows, cls_tail=True)

    def cell(what):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(a.reps):
                run(what)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    names = ("lanczos_248x330", "bicubic_centre_224", "backbone_cls_tail")
    for what in names:
        cell(what)
    ms = {w: [] for w in names}
    for _ in range(a.rounds):
        for what in names:
            ms[what].append(cell(what))
    med = {w: statistics.median(v) for w, v in ms.items()}
    read = N * H * W * 3
    res = {"tool": "resample_bench.py", "device": torch.cuda.get_device_name(0), "precision": a.precision, "views": N, "render": [H, W],
           "rounds": a.rounds, "reps_per_round": a.reps, "bytes_read_per_panorama": read}
    for w in names:
        res[w + "_ms"] = {"median": med[w], "min": min(ms[w]), "max": max(ms[w])}
    for w in names[:2]:
        res[w + "_effective_GB_per_s"] = read / med[w] / 1e6
        res[w + "_over_backbone"] = med[w] / med["backbone_cls_tail"]
    res["backbone_views_per_s"] = N / med["backbone_cls_tail"] * 1e3
    # (c), (d): whole files; every panorama exists beforehand, so the host side is the gather + copy a real store costs
    stored = SyntheticPanoStore(seed=3, cache=a.viewpoints + 1)
    for k in keys:
        stored.get("%s_%s" % k)
    with tempfile.TemporaryDirectory() as tmp:
        for name, store, e in (("raw_renders", renders, ex_raw), ("stored_views", stored, ex)):
            build_feature_file(store, keys[:16], os.path.join(tmp, "warm.npz"), e, out_image_logits=True, batch_size=576)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            build_feature_file(store, keys, os.path.join(tmp, "f.npz"), e, out_image_logits=True, batch_size=576)
            torch.cuda.synchronize()
            res["build_feature_file_%s_views_per_s" % name] = a.viewpoints * N / (time.perf_counter() - t0)
        build_image_store(renders, keys[:4], os.path.join(tmp, "warm"), batch_size=72)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        build_image_store(renders, keys, os.path.join(tmp, "panos"), batch_size=72)
        torch.cuda.synchronize()
        res["build_image_store_views_per_s"] = a.viewpoints * N / (time.perf_counter() - t0)
    res["viewpoints"] = a.viewpoints
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
