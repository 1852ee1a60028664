#!/usr/bin/env python3
"""Writes the stored panorama views (`"{scan}_{viewpoint}"` -> uint8 (36, 248, 330, 3)) from raw renders: the reference's
preprocess/build_image_lmdb.py, except

  --renders      replaces the simulator: a `PanoImageStore` path (directory of <key>.npy, .npz, LMDB) whose blocks are the 36 raw
                 renders of a viewpoint, uint8 (36, 480, 640, 3) (--render_size), RGB
  --output_dir   a directory of <key>.npy, which `PanoImageStore` reads (the reference writes an LMDB; the `lmdb` module is not part
                 of this project's environment -- `vln_hamt_amd.preprocess.build_image_store(env=...)` takes an opened one)
  --batch_size   views per resample launch, rounded up to whole panoramas
  --num_workers  host reader threads (at most 16)

    python tools/build_image_store.py --connectivity_dir connectivity --renders renders --output_dir panoimages

The resize is PIL's `resize((330, 248), Image.ANTIALIAS)` bit for bit, on the device."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vln_hamt_amd.data.image_data import PanoImageStore                                # noqa: E402
from vln_hamt_amd.preprocess import build_image_store, load_viewpoint_ids              # noqa: E402

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--connectivity_dir", default="../connectivity")
    parser.add_argument("--renders", required=True)
    parser.add_argument("--render_size", type=int, nargs=2, default=(480, 640), metavar=("H", "W"))
    parser.add_argument("--output_dir", required=True)
    parser.add_argument("--batch_size", default=72, type=int)
    parser.add_argument("--num_workers", type=int, default=8)
    args = parser.parse_args()
    scanvp_list = load_viewpoint_ids(args.connectivity_dir)
    print("Loaded %d viewpoints" % len(scanvp_list))
    renders = PanoImageStore(args.renders, height=args.render_size[0], width=args.render_size[1])
    t0 = time.time()
    n = build_image_store(renders, scanvp_list, args.output_dir, batch_size=args.batch_size, num_workers=args.num_workers)
    print("%d viewpoints (%d views) in %.1f s -> %s" % (n, 36 * n, time.time() - t0, args.output_dir))
