#!/usr/bin/env python3
"""Writes tests/golden/image_prep.npz: parameter records and PIL's uint8 results for a few views of `SyntheticPanoStore`.

    python tools/gen_image_prep_golden.py [--check]

The fixture pins the chain PIL == numpy host path == HIP kernel on machines without PIL: `recs` (VIEW_DTYPE bytes), `keys` / `view`
(which synthetic view each record transforms; `src` indexes the row), `out` uint8 (n, 224, 224, 3) = PIL's
`Image.fromarray(view).crop(box).resize((224, 224), Image.BICUBIC)` -> `ImageOps.mirror` -> `ImageEnhance.*` in the record's order.
The views themselves are not stored (they are regenerated from the store's seed).  --check compares instead of writing.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vln_hamt_amd.data import image_transform as T  # noqa: E402
from vln_hamt_amd.data.image_data import SyntheticPanoStore  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "image_prep.npz")
STORE_SEED = 7


def pil_apply(view, rec):
    """the reference side of every comparison: PIL's own calls"""
    from PIL import Image, ImageEnhance, ImageOps
    l, t, w, h = int(rec["left"]), int(rec["top"]), int(rec["width"]), int(rec["height"])
    im = Image.fromarray(np.ascontiguousarray(view)).crop((l, t, l + w, t + h)).resize((T.IMGSIZE, T.IMGSIZE), Image.BICUBIC)
    if int(rec["flip"]):
        im = ImageOps.mirror(im)
    for op in T.unpack_order(int(rec["order"])):
        if op == T.OP_BRIGHTNESS:
            im = ImageEnhance.Brightness(im).enhance(float(rec["brightness"]))
        elif op == T.OP_CONTRAST:
            im = ImageEnhance.Contrast(im).enhance(float(rec["contrast"]))
        elif op == T.OP_SATURATION:
            im = ImageEnhance.Color(im).enhance(float(rec["saturation"]))
    return np.asarray(im)


def cases():
    """-> (keys, view index per record, records with src = row)"""
    keys = ["scanA_vp0", "scanA_vp1", "scanB_vp0", "scanB_vp1", "scanC_vp0", "scanC_vp1"]
    view = [0, 7, 13, 22, 30, 35]
    recs = np.zeros((len(keys),), T.VIEW_DTYPE)
    recs[0] = T.draw_eval_params()
    recs[1] = T.make_record((0, 0, T.WIDTH, T.HEIGHT), True, (1, 0, 2), (1.31, 0.72, 0.66))          # whole view, contrast first
    recs[2] = T.make_record((101, 37, 83, 97), False, (2, 1, 0), (0.64, 1.38, 1.21))                 # upsampling both ways
    recs[3] = T.make_record((5, 60, 310, 120), True, (0, 2, 1), (1.4, 0.6, 1.0))                     # wide and low
    recs[4] = T.make_record((200, 3, 100, 240), False, (2, 0, 1), (0.9, 1.1, 1.39))                  # narrow and high
    recs[5] = T.make_record((33, 20, 260, 215), True, (1, 2, 0), (1.05, 1.25, 0.61))
    recs["src"] = np.arange(len(keys))
    return keys, view, recs


def views_of(keys, view):
    store = SyntheticPanoStore(STORE_SEED)
    return np.stack([store.get(k)[v] for k, v in zip(keys, view)], 0)


def build():
    keys, view, recs = cases()
    views = views_of(keys, view)
    out = np.stack([pil_apply(views[i], recs[i]) for i in range(len(recs))], 0)
    return dict(keys=np.array(keys), view=np.array(view, np.int32), recs=recs.view(np.uint8).reshape(len(recs), -1), out=out,
                store_seed=np.int32(STORE_SEED))


if __name__ == "__main__":
    data = build()
    if "--check" in sys.argv:
        old = np.load(OUT)
        for k, v in data.items():
            assert np.array_equal(old[k], v), k
        print("fixture matches its generator")
    else:
        np.savez_compressed(OUT, **data)
        print(OUT, os.path.getsize(OUT), "bytes")
