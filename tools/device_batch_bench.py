#!/usr/bin/env python3
"""Row N4 measurement: the host pipeline (MultiStepNavData.get_input -> *_collate -> PackedBatch.to_device) against the device-resident one
(index-only dataset -> *_index_collate -> IndexedBatch.to_device over a PretrainStore), on synthetic trajectories at bench.py's SAP shape:
B = 64, 768-d features, 1000 soft labels in the store, 80 tokens, 5 history steps with panoramas, 37 observation slots.

One process, one GPU; the two pipelines alternate inside every timed window; all of it fails without a GPU.  Reports
  (a) host __getitem__ + collate per batch on ONE thread, both pipelines (host clock);
  (b) device time of PackedBatch.to_device from pinned memory, H2D copy included (device events);
  (c) device time of IndexedBatch.to_device, likewise;
  (d) bytes crossing PCIe per batch, both ways;
  (e) the store's HBM footprint;
and checks first that the two device batches are equal, key for key, at the size it times.
usage: device_batch_bench.py [--batch 64] [--reps 30] [--windows 5] [--task sap] [--out profiles/device_batches_mi355x.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

F, P, A, L, T = 768, 1000, 4, 80, 5


def synth_dataset(root, scans=4, vps=48, trajs=96, seed=0):
    """a dataset directory in the formats data/r2r_data.py reads: ring graphs with chords, random features, paths of T + 1 viewpoints"""
    rng = np.random.default_rng(seed)
    feats = os.path.join(root, "fts")
    os.makedirs(feats)
    cands, lines = {}, []
    with open(os.path.join(root, "scans.txt"), "w") as f:
        f.write("\n".join(f"s{s}" for s in range(scans)) + "\n")
    for s in range(scans):
        nbrs = {v: sorted({(v + 1) % vps, (v - 1) % vps, (v + 7) % vps, (v - 7) % vps}) for v in range(vps)}
        xyz = rng.standard_normal((vps, 3)) * 3
        nodes = []
        for v in range(vps):
            pose = [0.0] * 16
            pose[3], pose[7], pose[11] = (float(x) for x in xyz[v])
            nodes.append({"image_id": f"v{v:03d}", "pose": pose, "included": True, "unobstructed": [u in nbrs[v] for u in range(vps)]})
            np.save(os.path.join(feats, f"s{s}_v{v:03d}.npy"), rng.standard_normal((36, F + P)).astype(np.float32))
            views = rng.choice(36, len(nbrs[v]), replace=False)
            cands[f"s{s}_v{v:03d}"] = {f"v{u:03d}": [int(views[k]), 2.0, float(rng.uniform(-0.2, 0.2)), float(rng.uniform(-0.2, 0.2))]
                                       for k, u in enumerate(nbrs[v])}
        with open(os.path.join(root, f"s{s}_connectivity.json"), "w") as f:
            json.dump(nodes, f)
        for j in range(trajs // scans):
            path = [int(rng.integers(vps))]
            while len(path) < T + 1:
                path.append(int(rng.choice([u for u in nbrs[path[-1]] if u not in path[-2:]])))
            names = [f"v{v:03d}" for v in path]
            act = [cands[f"s{s}_{names[t]}"][names[t + 1]][0] for t in range(T)] + [-1]
            lines.append({"scan": f"s{s}", "path": names, "path_viewindex": [int(x) for x in rng.integers(0, 36, T + 1)], "action_viewindex": act,
                          "rel_act_angles": rng.uniform(-1.5, 1.5, (T + 1, 2)).tolist(), "instr_ids": [f"s{s}_{j}_0"],
                          "instr_encodings": [[101] + [int(x) for x in rng.integers(1996, 29000, L - 2)] + [102]]})
    with open(os.path.join(root, "traj.jsonl"), "w") as f:
        f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    with open(os.path.join(root, "cands.json"), "w") as f:
        json.dump(cands, f)
    return dict(traj_files=[os.path.join(root, "traj.jsonl")], img_ft_file=feats, scanvp_cands_file=os.path.join(root, "cands.json"),
                connectivity_dir=root, image_feat_size=F, image_prob_size=P, angle_feat_size=A, max_txt_len=L, max_act_len=100, in_memory=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30, help="batches per pipeline and window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--task", default="sap", choices=["sap", "sar", "sprel"])
    ap.add_argument("--out", default=None, help="write the result as JSON here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_batch_bench: needs a GPU (nothing here is measured on a CPU)")
    from vln_hamt_amd import data as D
    dev = torch.device("cuda", 0)
    torch.set_num_threads(1)                          # (a) is per host thread
    B, task = args.batch, args.task
    tok = types.SimpleNamespace(cls_token_id=101, sep_token_id=102, mask_token_id=103, pad_token_id=0)
    with tempfile.TemporaryDirectory() as root:
        db = D.MultiStepNavData(**synth_dataset(root))
        t0 = time.perf_counter()
        store = D.PretrainStore(db, dev)
        build_s = time.perf_counter() - t0
        host_cls = {"sap": D.SapDataset, "sar": D.SarDataset, "sprel": D.SprelDataset}[task]
        host_ds, index_ds = host_cls(db, tok, 0.3, 0.43), D.INDEX_DATASETS[task](db, tok, 0.3, 0.43)
        full = [i for i, (_, _, t) in enumerate(db.traj_step_refer) if t == T]          # bench.py's shape: every sample at full length
        rng = np.random.default_rng(1)
        draws = [[int(x) for x in rng.choice(full, B)] for _ in range(args.reps)]

        def host_batch(ds, collate, idxs, seed):
            random.seed(seed)
            np.random.seed(seed)
            return collate([ds[i] for i in idxs])

        pipes = {"packed": (host_ds, D.COLLATE[task]), "indexed": (index_ds, D.INDEX_COLLATE[task])}
        # ---- equal batches at the size that is timed
        got = {k: host_batch(ds, c, draws[0], 5).pin_memory().to_device(dev) for k, (ds, c) in pipes.items()}
        for k, v in got["packed"].items():
            w = got["indexed"][k]
            assert (v is None and w is None) or (v.dtype == w.dtype and torch.equal(v, w)), k
        assert set(got["packed"]) == set(got["indexed"]) and store.check() == 0
        padded = sum(v.numel() * v.element_size() for v in got["packed"].values() if torch.is_tensor(v))
        # ---- (a) host time, (b) / (c) device time: alternating, several windows
        host_ms = {k: [] for k in pipes}
        dev_us = {k: [] for k in pipes}
        nbytes = {}
        for w in range(args.windows + 1):             # (window 0 warms every shape up and is dropped)
            for r, idxs in enumerate(draws):
                for k, (ds, c) in pipes.items():
                    t0 = time.perf_counter()
                    pb = host_batch(ds, c, idxs, 100 + r)
                    dt = time.perf_counter() - t0
                    pb = pb.pin_memory()
                    nbytes[k] = pb.nbytes
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = pb.to_device(dev)
                    e1.record()
                    e1.synchronize()
                    if w:
                        host_ms[k].append(dt * 1e3)
                        dev_us[k].append(e0.elapsed_time(e1) * 1e3)
                    del out
        med = lambda xs: round(statistics.median(xs), 3)
        spread = lambda xs: [round(float(np.percentile(xs, q)), 3) for q in (10, 90)]
        res = {"what": f"{task} batches, B={B}, F={F}, P={P}, A={A}, L={L}, T={T} with panoramas, 37 observation slots; synthetic trajectories",
               "gpu": torch.cuda.get_device_name(0), "batches_timed_per_pipeline": len(host_ms["packed"]),
               "host_ms_per_batch_one_thread": {k: {"median": med(v), "p10_p90": spread(v)} for k, v in host_ms.items()},
               "to_device_us_by_events": {k: {"median": med(v), "p10_p90": spread(v)} for k, v in dev_us.items()},
               "h2d_bytes_per_batch": nbytes, "d2h_bytes_per_batch": {k: 0 for k in pipes}, "padded_batch_bytes": padded,
               "store_hbm_bytes": store.nbytes, "store_rows": {"viewpoints": store.NV, "steps": store.NS}, "store_build_s": round(build_s, 3),
               "batches_equal": True, "anomalies": store.check()}
        res["indexed_to_device_not_slower"] = res["to_device_us_by_events"]["indexed"]["median"] <= res["to_device_us_by_events"]["packed"]["median"]
        res["indexed_host_faster"] = res["host_ms_per_batch_one_thread"]["indexed"]["median"] < res["host_ms_per_batch_one_thread"]["packed"]["median"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not (res["indexed_to_device_not_slower"] and res["indexed_host_faster"]):
        raise SystemExit("device_batch_bench: a condition failed (see the two booleans above)")


if __name__ == "__main__":
    main()
