#!/usr/bin/env python3
"""Writes tests/golden/vit_extract.npz: features and logits of the REFERENCE's own VisionTransformer (pretrain_src/model/
vision_transformer.py through oracle.ref_shim.import_vit) in eval mode -- `forward_features`, then `head`, as
preprocess/precompute_img_features_vit.py:99-100 calls them -- for the two configurations of tests/_vit_extract_ref.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_vit_extract_golden.py [--check]

Test infrastructure (needs the reference checkout, oracle.ref_shim.REF).  Outputs only: `<tag>/feats` [n, D], `<tag>/logits` [n, C];
weights and inputs are regenerated from the recipe by whoever reads the fixture.  --check compares instead of writing.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from oracle import ref_shim                    # noqa: E402
import _vit_extract_ref as R                   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vit_extract.npz")


def build():
    vt = ref_shim.import_vit()
    store = {}
    for tag, c in R.CONFIGS.items():
        ref = vt.VisionTransformer(num_classes=c["classes"], qkv_bias=True, **c["vit"])
        ref.load_state_dict({k: v.clone() for k, v in R.state_dict(tag).items()}, strict=True)
        ref.eval()
        with torch.no_grad():
            feats = ref.forward_features(torch.from_numpy(R.images(tag)))
            logits = ref.head(feats)
        store[f"{tag}/feats"], store[f"{tag}/logits"] = feats.numpy(), logits.numpy()
        print(f"  [{tag}] feats {tuple(feats.shape)} max|.| {float(feats.abs().max()):.3f}, logits {tuple(logits.shape)} max|.| {float(logits.abs().max()):.3f}")
    return store


if __name__ == "__main__":
    data = build()
    if "--check" in sys.argv:
        old = np.load(OUT)
        for k, v in data.items():
            assert np.allclose(old[k], v, rtol=0, atol=1e-6 * max(1.0, float(np.abs(v).max()))), k
        print("fixture matches its generator")
    else:
        np.savez_compressed(OUT, **data)
        print(OUT, os.path.getsize(OUT), "bytes")
