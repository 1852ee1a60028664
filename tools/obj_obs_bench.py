#!/usr/bin/env python3
"""REVERIE's object block of a rollout step: the device path (agent.ObjEpisodes.observe, one launch) against the host path it replaces
(per-episode numpy in the statement order of reverie/env.py::_get_obs :181-215 and reverie/agent.py::_object_variable :125-139, then
the uploads), on one box.  The protocol is tools/obs_bench.py's.

    python tools/obj_obs_bench.py [--out profiles/obj_gather_mi355x.json]

Cells: B = 8 and B = 64, Fo = 2048, A = 4, max_objects = 20, a synthetic store of --viewpoints viewpoints with 1 to 20 objects each.
Every timed call stands the episodes on fresh random viewpoints (pre-drawn on the device).  Both paths alternate round by round in one
process and end in a device synchronise; the median over the rounds is reported with the spread.  Before anything is timed the two paths
are compared bit for bit on the cell's own shapes.  `gather` is `observe()` timed with device events over back-to-back eager calls (so
never below the host's launch rate), and `gather_bytes_per_s` the bytes the gather has to move (every output element written once, every
live row read once) over it; `gather_in_graph` is the same call captured 50 times (50 sets of viewpoints) in one graph and replayed: the
launch as a captured rollout step pays for it.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

VIEWS = 36


def make_database(NV, Fo, max_objects, seed=0):
    """-> (graphs stand-in, the object database in the reference's dict form)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nodes = ["v%05d" % i for i in range(NV)]
    db = {}
    for i, vp in enumerate(nodes):
        n = int(rng.integers(1, max_objects + 1))
        boxes = np.concatenate([rng.integers(0, 400, (n, 2)), rng.integers(8, 200, (n, 2))], 1)
        db["scan_" + vp] = {"obj_ids": [str(x) for x in rng.integers(0, 1000, n)], "fts": rng.standard_normal((n, Fo), dtype=np.float32),
                            "bboxes": boxes.astype(np.int64), "viewindexs": rng.integers(0, VIEWS, n)}
    graphs = types.SimpleNamespace(scans=["scan"], nodes={"scan": nodes}, scan_n_host=np.array([NV], np.int32))
    return graphs, db


def host_step(db, keys, ang36, cur, view, dev, Fo, A, max_objects):
    """what the reference does on the host per step, then the uploads; -> the device tensors"""
    cands = []
    for row, vw in zip(cur, view):                                                               # reverie/env.py:188-204
        e = db[keys[row]]
        directional = ang36[vw]
        obj_ang = np.vstack([directional[v] for v in e["viewindexs"]])
        b = e["bboxes"]
        x1, y1, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        pos = np.stack([x1 / 640, y1 / 480, (x1 + w) / 640, (y1 + h) / 480, w * h / (640 * 480)], 0).transpose()
        fts = np.concatenate([e["fts"], obj_ang], 1)
        cands.append((pos[:max_objects], fts[:max_objects], e["obj_ids"][:max_objects]))
    lens = [max(len(c[2]), 1) for c in cands]                                                    # reverie/agent.py:126-139
    feats = np.zeros((len(cands), max(lens), Fo + A), np.float32)
    poses = np.zeros((len(cands), max(lens), 5), np.float32)
    for i, (pos, fts, ids) in enumerate(cands):
        if len(fts) > 0:
            feats[i, :lens[i]] = fts
            poses[i, :lens[i]] = pos
    up = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
    return up(feats[..., -A:]), up(feats[..., :-A]), up(poses), up(np.array(lens, np.int32))


def _median(xs):
    return {"us": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def bench(dev, NV, rounds, iters, Fo=2048, A=4, max_objects=20):
    from vln_hamt_amd.agent import ObjEpisodes, ObjStore, build_obj_tables
    graphs, db = make_database(NV, Fo, max_objects)
    keys = ["scan_" + vp for vp in graphs.nodes["scan"]]
    tab = build_obj_tables(graphs, db, Fo, max_objects)
    ang36 = np.random.Generator(np.random.PCG64(1)).standard_normal((VIEWS, VIEWS, A), dtype=np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    obs_store = types.SimpleNamespace(device=torch.device("cuda", torch.cuda.current_device()), NV=NV, A=A, ang36=up(ang36),
                                      vp_base=torch.zeros(1, dtype=torch.int64, device=dev), scan_n=torch.tensor([NV], dtype=torch.int32, device=dev), graphs=None)
    store = ObjStore.from_tensors(obs_store, *(up(tab[k]) for k in ("obj_off", "obj_feat", "obj_view", "obj_pos", "obj_id")))
    cnt = np.diff(tab["obj_off"])
    res = {}
    for B in (8, 64):
        rng = np.random.Generator(np.random.PCG64(B))
        curs, views = rng.integers(0, NV, (iters, B)).astype(np.int32), rng.integers(0, VIEWS, (iters, B)).astype(np.int32)
        curs_d, views_d = torch.from_numpy(curs).to(dev), torch.from_numpy(views).to(dev)
        nav = types.SimpleNamespace(scan=torch.zeros(B, dtype=torch.int32, device=dev), cur=curs_d[0], B=B)
        obs = types.SimpleNamespace(store=obs_store, nav=nav, B=B, view=views_d[0])
        ep = ObjEpisodes(store, obs)

        # ---- the two paths build the same tensors
        for i in range(3):
            nav.cur, obs.view = curs_d[i], views_d[i]
            o = ep.observe()
            ang, fts, pos, lens = host_step(db, keys, ang36, curs[i], views[i], dev, Fo, A, max_objects)
            L = fts.shape[1]
            assert torch.equal(o.obj_feats[:, :L], fts) and torch.equal(o.obj_angles[:, :L], ang) and torch.equal(o.obj_poses[:, :L], pos)
            assert torch.equal(o.obj_lens.clamp(min=1), lens) and not o.obj_feats[:, L:].any() and int(ep.anomalies.item()) == 0
        live = cnt[curs.ravel()].sum() / iters
        bytes_moved = 4 * B * ep.Ow * (Fo + A + 5) + 4 * live * (Fo + A + 5) + B * ep.Ow * 5 + live * 8      # written + read + mask, ids, views

        def device_path():
            for i in range(iters):
                nav.cur, obs.view = curs_d[i], views_d[i]
                ep.observe()
            torch.cuda.synchronize()

        def host_path():
            for i in range(iters):
                host_step(db, keys, ang36, curs[i], views[i], dev, Fo, A, max_objects)
            torch.cuda.synchronize()

        def gather_events():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(iters):
                nav.cur, obs.view = curs_d[i], views_d[i]
                ep.observe()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / iters

        device_path(), host_path(), gather_events()                                              # warm-up of every shape
        n_graph = min(iters, 50)                                                                 # the same calls inside one captured graph
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                for i in range(n_graph):
                    nav.cur, obs.view = curs_d[i], views_d[i]
                    ep.observe()
        torch.cuda.current_stream().wait_stream(side)

        def gather_graphed():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            graph.replay()
            s.record()
            for _ in range(4):
                graph.replay()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / (4 * n_graph)
        gather_graphed()
        samples = {"device": [], "host": [], "gather": [], "graphed": []}
        for _ in range(rounds):
            for k, f in (("host", host_path), ("device", device_path)):                         # alternating, same process
                t0 = time.perf_counter()
                f()
                samples[k].append((time.perf_counter() - t0) / iters * 1e6)
            samples["gather"].append(gather_events())
            samples["graphed"].append(gather_graphed())
        r = {"device_observe": _median(samples["device"]), "host_stack_upload": _median(samples["host"]), "gather": _median(samples["gather"]),
             "gather_in_graph": _median(samples["graphed"])}
        r["host_over_device"] = round(r["host_stack_upload"]["us"] / r["device_observe"]["us"], 2)
        r["device_faster"] = r["device_observe"]["us"] < r["host_stack_upload"]["us"]
        r["gather_bytes"], r["gather_bytes_per_s"] = int(bytes_moved), round(bytes_moved / (r["gather"]["us"] * 1e-6), 0)
        r["gather_in_graph_bytes_per_s"] = round(bytes_moved / (r["gather_in_graph"]["us"] * 1e-6), 0)
        r["host_upload_bytes"] = int(4 * B * max_objects * (Fo + A + 5) + 4 * B)                  # (at the widest batch: one viewpoint with 20 objects)
        r["width"], r["mean_objects"], r["calls_per_sample"] = ep.Ow, round(float(live) / B, 2), iters
        res[f"B{B}"] = r
        print(f"[obj] B {B:2d}: host {r['host_stack_upload']['us']:9.1f} us/step ({r['host_stack_upload']['min']:.1f}-{r['host_stack_upload']['max']:.1f})   "
              f"device observe {r['device_observe']['us']:7.1f} us/step ({r['device_observe']['min']:.1f}-{r['device_observe']['max']:.1f})   "
              f"gather by events {r['gather']['us']:.1f} us = {r['gather_bytes_per_s'] / 1e9:.1f} GB/s over {bytes_moved / 1e6:.2f} MB   "
              f"inside a graph {r['gather_in_graph']['us']:.1f} us = {r['gather_in_graph_bytes_per_s'] / 1e9:.1f} GB/s", flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--viewpoints", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("obj_obs_bench: needs a GPU (no CPU fallback)")
    dev = torch.device("cuda")
    res = {"workload": "REVERIE's object block of a rollout step (features, view angles, boxes, mask, count, ids; Fo 2048, A 4, max_objects 20): "
                       "agent.ObjEpisodes.observe vs per-episode numpy stacking and uploads",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "viewpoints": a.viewpoints, "per_step": bench(dev, a.viewpoints, a.rounds, a.iters)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
