#!/usr/bin/env python3
"""The observations of a rollout step: the device path (agent.ObsEpisodes: `observe` + `turn`, two launches) against the host path it
replaces (per-episode numpy stacking in the statement order of env.py::make_candidate / _get_obs and agent_cmt.py's
_cand_pano_feature_variable / _history_variable, then the uploads), on one box.

    python tools/obs_bench.py [--out profiles/obs_gather_mi355x.json]

Cells: B = 8 and B = 64, F = 768, A = 4, panorama layout with the history outputs, a synthetic store of --viewpoints viewpoints with 1 to
12 candidates each.  Every timed call stands the episodes on fresh random viewpoints (pre-drawn on the device: rows of the store that
the last call did not touch).  Both paths alternate round by round in one process and end in a device synchronise; the median over the
rounds is reported with the spread.  Before anything is timed the two paths are compared bit for bit on the cell's own shapes.
`gather` is `observe()` alone, timed with device events over back-to-back eager calls (so never below the host's launch rate), and
`gather_bytes_per_s` the bytes the gather has to move (every output element written once, every live row read once) over it;
`gather_in_graph` is the same call captured 50 times (50 sets of viewpoints) in one graph and replayed: the launch as a captured
rollout step pays for it.
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


def make_tables(NV, F, A, C, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    cnt = rng.integers(1, 13, NV).astype(np.int32)
    point, node = np.full((NV, C), -1, np.int32), np.full((NV, C), -1, np.int32)
    for r in range(NV):
        point[r, :cnt[r]], node[r, :cnt[r]] = rng.integers(0, VIEWS, cnt[r]), rng.integers(0, NV, cnt[r])
    return {"feat": rng.standard_normal((NV, VIEWS, F), dtype=np.float32), "ang36": rng.standard_normal((VIEWS, VIEWS, A), dtype=np.float32),
            "cand_cnt": cnt, "cand_point": point, "cand_node": node, "cand_ang": rng.standard_normal((NV, C, 12, A), dtype=np.float32),
            "vp_base": np.zeros(1, np.int64), "scan_n": np.array([NV], np.int32)}


def host_step(tab, cur, view, dev, F, A):
    """what the reference does on the host per step, then the uploads; -> the device tensors and the candidates' views"""
    obs = []
    for row, vw in zip(cur, view):
        feature = np.concatenate((tab["feat"][row], tab["ang36"][vw]), -1)                       # env.py:282
        cands = [{"pointId": int(tab["cand_point"][row, c]),
                  "feature": np.concatenate((tab["feat"][row, tab["cand_point"][row, c]], tab["cand_ang"][row, c, vw % 12]), -1)}     # :239-252
                 for c in range(tab["cand_cnt"][row])]
        obs.append({"feature": feature, "candidate": cands, "viewIndex": vw})
    ob_lens, imgs, angs, navs = [], [], [], []
    for ob in obs:                                                                               # agent_cmt.py:111-135
        ci, ca, nt = [], [], []
        taken = np.zeros(VIEWS, bool)
        for cc in ob["candidate"]:
            ci.append(cc["feature"][:F])
            ca.append(cc["feature"][F:])
            taken[cc["pointId"]] = True
            nt.append(1)
        ci.append(np.zeros(F, np.float32))
        ca.append(np.zeros(A, np.float32))
        nt.append(2)
        rest = ob["feature"][~taken]
        imgs.append(np.concatenate([np.vstack(ci), rest[:, :F]], 0))
        angs.append(np.concatenate([np.vstack(ca), rest[:, F:]], 0))
        nt.extend([0] * (VIEWS - int(taken.sum())))
        ob_lens.append(len(nt))
        navs.append(nt)
    L = max(ob_lens)
    for i in range(len(obs)):                                                                    # :138-145
        pad = L - ob_lens[i]
        imgs[i] = np.concatenate([imgs[i], np.zeros((pad, F), np.float32)], 0)
        angs[i] = np.concatenate([angs[i], np.zeros((pad, A), np.float32)], 0)
        navs[i] = np.array(navs[i] + [0] * pad)
    h_img = np.zeros((len(obs), F), np.float32)                                                  # :173-190
    h_pimg, h_pang = np.zeros((len(obs), VIEWS, F), np.float32), np.zeros((len(obs), VIEWS, A), np.float32)
    for i, ob in enumerate(obs):
        h_img[i] = ob["feature"][ob["viewIndex"], :F]
        h_pimg[i], h_pang[i] = ob["feature"][:, :F], ob["feature"][:, F:]
    up = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
    out = (up(np.stack(imgs, 0)), up(np.stack(angs, 0)), up(np.stack(navs, 0)), up(np.array(ob_lens, np.int32)), up(h_img), up(h_pimg), up(h_pang))
    return out, [[cc["pointId"] for cc in ob["candidate"]] for ob in obs]


def host_turn(points, env_action, view):
    return [p[a] if a >= 0 else v for p, a, v in zip(points, env_action, view)]


def _median(xs):
    return {"us": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def bench(dev, NV, rounds, iters, F=768, A=4, C=12):
    from vln_hamt_amd.agent import ObsEpisodes, ObsStore
    tab = make_tables(NV, F, A, C)
    store = ObsStore.from_tensors(*(torch.from_numpy(tab[k]).to(dev) for k in ("feat", "ang36", "cand_cnt", "cand_point", "cand_node", "cand_ang", "vp_base", "scan_n")))
    res = {}
    for B in (8, 64):
        rng = np.random.Generator(np.random.PCG64(B))
        curs, views = rng.integers(0, NV, (iters, B)).astype(np.int32), rng.integers(0, VIEWS, (iters, B)).astype(np.int32)
        acts = np.array([[int(rng.integers(-1, tab["cand_cnt"][r])) for r in row] for row in curs], np.int32)
        curs_d, views_d, acts_d = (torch.from_numpy(a).to(dev) for a in (curs, views, acts))
        nav = types.SimpleNamespace(scan=torch.zeros(B, dtype=torch.int32, device=dev), cur=curs_d[0], B=B, T_max=1)
        ep = ObsEpisodes(store, nav)

        # ---- the two paths build the same tensors
        for i in range(3):
            nav.cur = curs_d[i]
            ep.view.copy_(views_d[i])
            o = ep.observe()
            (img, ang, navt, lens, h_img, h_pimg, h_pang), points = host_step(tab, curs[i], views[i], dev, F, A)
            L = img.shape[1]
            assert torch.equal(o.ob_img[:, :L], img) and torch.equal(o.ob_ang[:, :L], ang) and torch.equal(o.ob_nav[:, :L], navt) and torch.equal(o.ob_len, lens)
            assert not o.ob_img[:, L:].any() and torch.equal(o.hist_img, h_img) and torch.equal(o.hist_pano_img, h_pimg) and torch.equal(o.hist_pano_ang, h_pang)
            ep.turn(acts_d[i])
            assert ep.view.cpu().tolist() == host_turn(points, acts[i].tolist(), views[i].tolist())
        ob_rows = sum(int(tab["cand_cnt"][r]) + VIEWS - len(set(tab["cand_point"][r, :tab["cand_cnt"][r]].tolist())) for r in curs.ravel()) / iters
        hist = B * (F + VIEWS * (F + A))
        bytes_moved = 4 * (B * ep.W * (F + A) + hist) + 4 * (ob_rows * (F + A) + hist) + B * ep.W * 17          # written + read + the per-slot integers

        def device_path():
            for i in range(iters):
                nav.cur = curs_d[i]
                ep.observe()
                ep.turn(acts_d[i])
            torch.cuda.synchronize()

        def host_path():
            view = views[0].tolist()
            for i in range(iters):
                _, points = host_step(tab, curs[i], view, dev, F, A)
                view = host_turn(points, acts[i].tolist(), view)
            torch.cuda.synchronize()

        def gather_events():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(iters):
                nav.cur = curs_d[i]
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
                    nav.cur = curs_d[i]
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
        r = {"device_observe_turn": _median(samples["device"]), "host_stack_upload": _median(samples["host"]), "gather": _median(samples["gather"]),
             "gather_in_graph": _median(samples["graphed"])}
        r["host_over_device"] = round(r["host_stack_upload"]["us"] / r["device_observe_turn"]["us"], 2)
        r["device_faster"] = r["device_observe_turn"]["us"] < r["host_stack_upload"]["us"]
        r["gather_bytes"], r["gather_bytes_per_s"] = int(bytes_moved), round(bytes_moved / (r["gather"]["us"] * 1e-6), 0)
        r["gather_in_graph_bytes_per_s"] = round(bytes_moved / (r["gather_in_graph"]["us"] * 1e-6), 0)
        r["width"], r["calls_per_sample"] = ep.W, iters
        res[f"B{B}"] = r
        print(f"[obs] B {B:2d}: host {r['host_stack_upload']['us']:9.1f} us/step ({r['host_stack_upload']['min']:.1f}-{r['host_stack_upload']['max']:.1f})   "
              f"device observe + turn {r['device_observe_turn']['us']:7.1f} us/step ({r['device_observe_turn']['min']:.1f}-{r['device_observe_turn']['max']:.1f})   "
              f"gather alone {r['gather']['us']:.1f} us = {r['gather_bytes_per_s'] / 1e9:.1f} GB/s over {bytes_moved / 1e6:.2f} MB   "
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
        raise SystemExit("obs_bench: needs a GPU (no CPU fallback)")
    dev = torch.device("cuda")
    res = {"workload": "observations of a rollout step (candidates, STOP, remaining views, history views; F 768, A 4, panorama layout): "
                       "agent.ObsEpisodes observe + turn vs per-episode numpy stacking and uploads",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "viewpoints": a.viewpoints, "per_step": bench(dev, a.viewpoints, a.rounds, a.iters)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
