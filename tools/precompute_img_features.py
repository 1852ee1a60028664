#!/usr/bin/env python3
"""Writes the view-feature file (`"{scan}_{viewpoint}"` -> [36, 768 (+ 1000)]) from stored panoramas: the reference's
preprocess/precompute_img_features_vit.py with its arguments, except

  --img_db       replaces --scan_dir: a `PanoImageStore` path (directory of <key>.npy, .npz, LMDB).  There is no simulator.
  --num_workers  host reader threads (at most 16), not simulator processes
  --precision    bf16 (default) or fp32 backbone
  --no_cls_tail  run the full last block instead of the cls-only tail
  --resize       bicubic: --img_db holds raw renders (--render_size, default 480 640); timm's Resize(248) + CenterCrop(224) run on
                 the device in front of the backbone, as the reference's transform does on the host.  Without it only stored
                 248 x 330 views are accepted.

    python tools/precompute_img_features.py --checkpoint_file vit.pt --connectivity_dir connectivity --img_db panos \\
        --out_image_logits --output_file img_features/vit_fts.npz

--output_file: a directory (one .npy per key), .npz, or .hdf5 / .h5 (needs h5py)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vln_hamt_amd.data.image_data import PanoImageStore                                                # noqa: E402
from vln_hamt_amd.preprocess import build_feature_extractor, build_feature_file, load_viewpoint_ids     # noqa: E402

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--model_name", default="vit_base_patch16_224")
    parser.add_argument("--checkpoint_file", default=None)
    parser.add_argument("--connectivity_dir", default="../connectivity")
    parser.add_argument("--img_db", required=True)
    parser.add_argument("--out_image_logits", action="store_true", default=False)
    parser.add_argument("--output_file", required=True)
    parser.add_argument("--batch_size", default=64, type=int)
    parser.add_argument("--num_workers", type=int, default=8)
    parser.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    parser.add_argument("--no_cls_tail", action="store_true", default=False)
    parser.add_argument("--resize", default=None, choices=("bicubic",))
    parser.add_argument("--render_size", type=int, nargs=2, default=(480, 640), metavar=("H", "W"))
    args = parser.parse_args()
    scanvp_list = load_viewpoint_ids(args.connectivity_dir)
    print("Loaded %d viewpoints" % len(scanvp_list))
    extractor = build_feature_extractor(args.model_name, args.checkpoint_file, hamt_precision=args.precision, cls_tail=not args.no_cls_tail,
                                        resize=args.resize)
    img_db = PanoImageStore(args.img_db, height=args.render_size[0], width=args.render_size[1]) if args.resize else args.img_db
    t0 = time.time()
    n = build_feature_file(img_db, scanvp_list, args.output_file, extractor, out_image_logits=args.out_image_logits,
                           batch_size=args.batch_size, num_workers=args.num_workers)
    print("%d viewpoints (%d views) in %.1f s -> %s" % (n, 36 * n, time.time() - t0, args.output_file))
