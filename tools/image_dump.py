#!/usr/bin/env python3
"""Every output of `image_prep`, `image_resample` and `library_taps` on the shapes the image benchmarks use, from a given
libhamt_hip.so: the evidence for "a change to csrc/image_prep.hip, csrc/image_resample.hip or csrc/pil_resample.h moved no bit".

    python tools/image_dump.py --lib PATH/libhamt_hip.so --out a.json       # once per library, each in a fresh process
    python tools/image_dump.py --compare a.json b.json [--report FILE]     # exit status 1 unless every array is equal

(i)   `image_prep` on the 221 train-draw slots of tools/image_pipeline_bench.py's SAP sample (248 x 330): nchw, patch rows fp32 and
      bf16, for 8 dataset seeds;
(ii)  `image_resample` of 36 seeded 480 x 640 views to 248 x 330 Lanczos and to the bicubic centre window of
      `eval_resize_geometry(480, 640)`;
(iii) `library_taps` for both axes of both.
The arrays of (i) are 2.6 GB, so a dump holds dtype, shape and the SHA-256 of each array's raw bytes, not the bytes."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
SEEDS = 8


def dump(lib, out):
    import torch
    from vln_hamt_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)                # before the first load
    from image_pipeline_bench import SyntheticSapImages
    from vln_hamt_amd.data.image_prep import image_prep
    from vln_hamt_amd.data.image_resample import image_resample, library_taps
    from vln_hamt_amd.data.image_tasks import sap_image_collate
    from vln_hamt_amd.data.image_transform import eval_resize_geometry
    dev = torch.device("cuda", 0)
    arrays = {}

    def put(name, t):
        a = np.ascontiguousarray(t.detach().cpu().view(torch.uint8).numpy() if torch.is_tensor(t) else t)
        arrays[name] = [str(t.dtype), list(t.shape), hashlib.sha256(a.tobytes()).hexdigest()]

    for seed in range(SEEDS):
        pb = sap_image_collate([SyntheticSapImages(n=1, seed=seed)[0]])
        src = torch.from_numpy(pb.host_views().copy()).to(dev)
        recs = np.concatenate([pb.host_records(k) for k in ("hist_images", "hist_pano_images", "ob_images")]).copy()
        assert len(recs) == 221
        put(f"prep/seed{seed}/nchw", image_prep(src, recs))
        put(f"prep/seed{seed}/patches_fp32", image_prep(src, recs, layout="patches").rows)
        put(f"prep/seed{seed}/patches_bf16", image_prep(src, recs, layout="patches", dtype=torch.bfloat16).rows)
    H, W = 480, 640
    OH, OW, window = eval_resize_geometry(H, W)
    views = torch.from_numpy(np.random.Generator(np.random.PCG64(11)).integers(0, 256, (36, H, W, 3), dtype=np.uint8)).to(dev)
    put("resample/lanczos_248x330", image_resample(views, (OH, OW), "lanczos"))
    put("resample/bicubic_centre_224", image_resample(views, (OH, OW), "bicubic", window))
    for filt, (x0, y0, w, h) in (("lanczos", (0, 0, OW, OH)), ("bicubic", window)):
        for axis, (i, o, first, count) in (("x", (W, OW, x0, w)), ("y", (H, OH, y0, h))):
            for part, a in zip(("xmin", "xcnt", "k"), library_taps(i, o, filt, first, count)):
                put(f"taps/{filt}/{axis}/{part}", a)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(arrays, f, indent=0)
    print(f"image_dump: {len(arrays)} arrays from {_lib.LIB_PATH} -> {out}", flush=True)


def compare(a, b, report):
    with open(a) as f:
        fa = json.load(f)
    with open(b) as f:
        fb = json.load(f)
    lines = [f"array names differ: {sorted(set(fa) ^ set(fb))}"] if sorted(fa) != sorted(fb) else []
    names = sorted(set(fa) & set(fb))
    lines += [f"DIFFERS {k}: {fa[k]} vs {fb[k]}" for k in names if fa[k] != fb[k]]
    equal = sum(fa[k] == fb[k] for k in names)
    head = [f"arrays compared: {len(names)}", f"arrays equal (dtype, shape, SHA-256 of the raw bytes): {equal}",
            f"elements: {sum(int(np.prod(fa[k][1])) for k in names)}"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if report:
        with open(report, "w") as f:
            f.write(text)
    return 0 if equal == len(names) and not lines else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.report))
    dump(a.lib, a.out)
