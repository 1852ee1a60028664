#!/usr/bin/env python3
"""What a rollout step and an evaluation pass read from the navigation graph: the agent's host loops (teacher look-up, back-track mask,
reward shaping with a full DTW per episode per step, the metrics; dict-of-dict distances, as the reference keeps them) against the
device path (ops.nav_observe + ops.nav_advance per step, ops.nav_eval per pass).

    python tools/nav_reward_bench.py [--out profiles/nav_reward_mi355x.json]

  host    Python loops over the batch: the teacher's slot, the visited-set mask, cal_dtw over the whole path walked so far, the
          reward rules, then the uploads the model needs (target, mask; the rewards once per rollout) -- the statement sequence of
          agent_cmt.py:199-211, :342-349, :407-445 and env.py::_eval_item.  Checked against tests/golden/nav_reward.npz (the
          reference's own statements) before anything is timed.
  device  NavEpisodes + the two launches per step; NavGraphs.eval_items (pack, upload, one launch, download) and the launch alone.
Per-step cells: B in {8, 64}; ground truth 7 / 14 steps (R2R) and 40 / 39 steps (R4R-like), whole rollouts on the 70-node test graph,
time per step.  Eval cells: N = 2 349 at R2R shapes, N = 45 000 at 40 x 40 (the host is timed on the first --host-items of them and
scaled; the JSON says so).  Both paths alternate round by round in one process; the median over the rounds is reported with the spread.
The graphed inference step (tools/policy_step_bench.py's, config-5 shape) is measured with and without the two extra launches.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

GOLDEN = os.path.join(ROOT, "tests", "golden")
CONNECTIVITY = [os.path.join(GOLDEN, "r2r_tiny"), os.path.join(GOLDEN, "nav_tiny")]
IGNORE = -100


# ------------------------------------------------------------------------------------------------ the host path
def host_dtw(D, pred, ref):
    m = np.inf * np.ones((len(pred) + 1, len(ref) + 1))
    m[0][0] = 0
    for i in range(1, len(pred) + 1):
        for j in range(1, len(ref) + 1):
            m[i][j] = D[pred[i - 1]][ref[j - 1]] + min(m[i - 1][j], m[i][j - 1], m[i - 1][j - 1])
    return m[len(pred)][len(ref)]


def host_ndtw(D, pred, ref):
    return np.exp(-host_dtw(D, pred, ref) / (3.0 * len(ref)))


def host_teacher_vp(nxt, here, gt, t, mode):
    if mode == "shortest":
        return nxt[here][gt[-1]]
    if mode == "path_step":
        return gt[t + 1] if t < len(gt) - 1 else here
    if here in gt:
        i = gt.index(here)
        return here if i == len(gt) - 1 else gt[i + 1]
    return None


class HostEpisodes:
    """the agent's host state of one rollout: where every episode stands, its path, visited set, last_dist / last_ndtw"""

    def __init__(self, D, nxt, starts, gts):
        self.D, self.nxt, self.B, self.gt = D, nxt, len(starts), gts
        self.here, self.path, self.visited = list(starts), [[s] for s in starts], [set() for _ in starts]
        self.last_dist, self.last_ndtw = np.zeros(self.B, np.float32), np.zeros(self.B, np.float32)
        self.failed = 0
        for i in range(self.B):
            self.last_dist[i] = D[i][starts[i]][gts[i][-1]]
            self.last_ndtw[i] = host_ndtw(D[i], self.path[i], gts[i])

    def observe(self, t, cands, ended, mode, V):
        a = np.zeros(self.B, np.int64)
        bt = np.zeros((self.B, V), bool)
        for i in range(self.B):
            if ended[i]:
                a[i] = IGNORE
            else:
                tv = host_teacher_vp(self.nxt[i], self.here[i], self.gt[i], t, mode)
                for k, c in enumerate(cands[i]):
                    if c == tv:
                        a[i] = k
                        break
                else:
                    if tv == self.here[i]:
                        a[i] = len(cands[i])
                    else:
                        a[i], self.failed = IGNORE, self.failed + 1
            self.visited[i].add(self.here[i])
            for k, c in enumerate(cands[i]):
                if c in self.visited[i]:
                    bt[i][k] = True
        return a, bt

    def advance(self, cands, cpu_a_t, ended):
        B = self.B
        dist, ndtw, reward = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        for i in range(B):
            if cpu_a_t[i] != -1:
                self.here[i] = cands[i][cpu_a_t[i]]
                self.path[i].append(self.here[i])
            dist[i] = self.D[i][self.here[i]][self.gt[i][-1]]
            ndtw[i] = host_ndtw(self.D[i], self.path[i], self.gt[i])
            if ended[i]:
                reward[i] = 0.0
            elif cpu_a_t[i] == -1:
                reward[i] = 2.0 + ndtw[i] * 2.0 if dist[i] < 3.0 else -2.0
            else:
                reward[i] = -(dist[i] - self.last_dist[i])
                shaped = ndtw[i] - self.last_ndtw[i]
                reward[i] = (1.0 if reward[i] > 0.0 else -1.0 if reward[i] < 0.0 else 0.0) + shaped
                if self.last_dist[i] <= 1.0 and dist[i] - self.last_dist[i] > 0.0:
                    reward[i] -= (1.0 - self.last_dist[i]) * 2.0
        self.last_dist[:], self.last_ndtw[:] = dist, ndtw
        return reward, dist, ndtw


def host_eval_item(D, path, gt):
    goal = gt[-1]
    near = path[0]
    for v in path:
        if D[v][goal] < D[near][goal]:
            near = v
    s = {"nav_error": D[path[-1]][goal], "oracle_error": D[near][goal], "trajectory_steps": len(path) - 1,
         "trajectory_lengths": np.sum([D[a][b] for a, b in zip(path[:-1], path[1:])])}
    glen = np.sum([D[a][b] for a, b in zip(gt[:-1], gt[1:])])
    s["success"] = float(s["nav_error"] < 3.0)
    s["spl"] = s["success"] * glen / max(s["trajectory_lengths"], glen, 0.01)
    s["oracle_success"] = float(s["oracle_error"] < 3.0)
    s["DTW"] = host_dtw(D, path, gt)
    s["nDTW"] = np.exp(-s["DTW"] / (3.0 * len(gt)))
    s["SDTW"] = s["success"] * s["nDTW"]
    cover = np.mean([np.exp(-np.min([D[u][v] for v in path]) / 3.0) for u in gt])
    expected = cover * glen
    with np.errstate(invalid="ignore"):
        s["CLS"] = cover * (expected / (expected + np.abs(expected - s["trajectory_lengths"])))
    return s


def dict_tables(graphs):
    """per scan: ({a: {b: metres}}, {a: {b: next hop}}) over node ids -- the dict-of-dict form the agent's host loops index"""
    out = []
    for s in graphs.scans:
        d, nx_ = graphs.dist_host[s], graphs.nxt_host[s]
        n = len(d)
        out.append(({a: {b: float(d[a, b]) for b in range(n)} for a in range(n)}, {a: {b: int(nx_[a, b]) for b in range(n)} for a in range(n)}))
    return out


def check_host_path_against_golden(graphs):
    z = np.load(os.path.join(GOLDEN, "nav_reward.npz"))
    tabs = dict_tables(graphs)
    g = lambda k: z["roll/" + k]
    T, B, V = g("cand").shape
    gts = [g("gt")[b, :g("gt_len")[b]].tolist() for b in range(B)]
    for mode in ("path_step", "path_index", "shortest"):
        ep = HostEpisodes([tabs[s][0] for s in g("scan")], [tabs[s][1] for s in g("scan")], g("start").tolist(), gts)
        for t in range(T):
            cands = [g("cand")[t, b, :g("cand_len")[t, b] - 1].tolist() for b in range(B)]
            a, bt = ep.observe(t, cands, g("ended")[t], mode, V)
            r, dist, ndtw = ep.advance(cands, g("env_action")[t], g("ended")[t])
            assert np.array_equal(a, g(f"target/{mode}")[t]) and np.array_equal(bt, g("bt_mask")[t].astype(bool)), (mode, t)
            assert np.array_equal(dist, g("dist")[t]) and np.abs(ndtw - g("ndtw")[t]).max() <= 2.4e-7 and np.abs(r - g("reward")[t]).max() <= 1e-6, (mode, t)
        assert ep.failed == int(g(f"assert/{mode}").sum())
    e = lambda k: z["eval/" + k]
    cols = ("nav_error", "oracle_error", "trajectory_steps", "trajectory_lengths", "success", "spl", "oracle_success", "DTW", "nDTW", "SDTW", "CLS")
    for i in range(len(e("scan"))):
        s = host_eval_item(tabs[e("scan")[i]][0], e("path")[i, :e("path_len")[i]].tolist(), e("gt")[i, :e("gt_len")[i]].tolist())
        got, want = np.array([s[c] for c in cols], np.float64), e("metrics")[i]
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got, want, rtol=1e-12, atol=0, equal_nan=True), (i, got, want)
    print("[nav bench] the host path reproduces tests/golden/nav_reward.npz", flush=True)


# ------------------------------------------------------------------------------------------------ scripted work
def walk(rng, nbrs, start, n):
    p = [start]
    while len(p) < n:
        nb = nbrs[p[-1]]
        fresh = [v for v in nb if v not in p]
        pool = fresh if fresh and rng.random() > 0.2 else nb
        p.append(pool[int(rng.integers(len(pool)))])
    return p


def make_rollout(graphs, B, G, T, V, seed=0):
    """B episodes on scanC: a ground truth of G nodes, a scripted walk of T moves near it; per step the candidates (neighbours, shuffled)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nx_ = graphs.nxt_host["scanC"]
    n = len(nx_)
    nbrs = [[y for y in range(n) if y != x and nx_[x, y] == y] for x in range(n)]
    gts = [walk(rng, nbrs, int(rng.integers(n)), G) for _ in range(B)]
    here = [gt[0] for gt in gts]
    steps = []
    for t in range(T):
        cands, act = [], []
        for b in range(B):
            nb = [nbrs[here[b]][j] for j in rng.permutation(len(nbrs[here[b]]))]
            want = gts[b][t + 1] if t + 1 < G and rng.random() > 0.25 and gts[b][t + 1] in nb else nb[int(rng.integers(len(nb)))]
            cands.append(nb)
            act.append(nb.index(want))
            here[b] = want
        cn = np.full((B, V), -1, np.int32)
        for b, nb in enumerate(cands):
            cn[b, :len(nb)] = nb
        steps.append((cands, np.array(act, np.int32), cn, np.array([len(c) + 1 for c in cands], np.int32)))
    return gts, steps


def _reps(f, window=0.2):
    """how often to call `f` so that one timed sample lasts about `window` seconds (f ends in a device synchronise)"""
    f()
    t0 = time.perf_counter()
    f()
    return max(1, int(window / max(time.perf_counter() - t0, 1e-6)))


def _sample(f, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return (time.perf_counter() - t0) / reps


def _median(xs):
    return {"us": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def bench_steps(graphs, dev, rounds):
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import NavEpisodes
    tabs = dict_tables(graphs)
    s = graphs.scans.index("scanC")
    name = lambda v: graphs.viewpoint("scanC", v)
    res, V = {}, 9
    for B in (8, 64):
        for G, T, tag in ((7, 14, "r2r_gt7_path15"), (40, 39, "r4r_gt40_path40")):
            gts, steps = make_rollout(graphs, B, G, T, V, seed=B + G)
            nav = NavEpisodes(graphs, T, B, max_gt=64)
            ended_d = torch.zeros(B, dtype=torch.uint8, device=dev)
            mask_d = torch.ones(B, dtype=torch.float32, device=dev)
            reward_d = torch.zeros(T, B, dtype=torch.float32, device=dev)
            dev_steps = [(torch.from_numpy(cn).to(dev), torch.from_numpy(cl).to(dev), torch.from_numpy(act).to(dev)) for _, act, cn, cl in steps]
            ended = np.zeros(B, bool)

            def host_rollout():
                ep = HostEpisodes([tabs[s][0]] * B, [tabs[s][1]] * B, [g_[0] for g_ in gts], gts)
                rewards = []
                for t, (cands, act, _, _) in enumerate(steps):
                    a, bt = ep.observe(t, cands, ended, "path_step", V)
                    torch.from_numpy(a).to(dev, non_blocking=True)
                    torch.from_numpy(bt).to(dev, non_blocking=True)
                    rewards.append(ep.advance(cands, act, ended)[0])
                torch.from_numpy(np.stack(rewards)).to(dev, non_blocking=True)
                torch.cuda.synchronize()

            def device_rollout():
                nav.reset(["scanC"] * B, [name(g_[0]) for g_ in gts], [[name(v) for v in g_] for g_ in gts])
                for t, (cn, cl, act) in enumerate(dev_steps):
                    ops.nav_observe(nav, t, cn, cl, ended_d, mode="path_step")
                    ops.nav_advance(nav, cn, act, mask_d, reward_d[t])
                torch.cuda.synchronize()
            reps = {"host": _reps(host_rollout), "device": _reps(device_rollout)}
            samples = {"host": [], "device": []}
            for _ in range(rounds):
                for k, f in (("host", host_rollout), ("device", device_rollout)):          # alternating, same process
                    samples[k].append(_sample(f, reps[k]) / T * 1e6)
            # the two paths computed the same rewards
            ep = HostEpisodes([tabs[s][0]] * B, [tabs[s][1]] * B, [g_[0] for g_ in gts], gts)
            want = np.stack([ep.advance(c, a, ended)[0] for c, a, _, _ in steps])
            err = float(np.abs(reward_d.cpu().numpy() - want).max())
            assert err <= 1e-6, err
            r = {k: _median(v) for k, v in samples.items()}
            r["device_not_slower"] = r["device"]["us"] <= r["host"]["us"]
            r["max_reward_difference"], r["rollouts_per_sample"] = err, reps
            res[f"B{B}_{tag}"] = r
            print(f"[nav step] B {B:2d} {tag}: host {r['host']['us']:9.1f} us/step ({r['host']['min']:.1f}-{r['host']['max']:.1f})   "
                  f"device {r['device']['us']:7.1f} us/step ({r['device']['min']:.1f}-{r['device']['max']:.1f}; reset included)", flush=True)
    return res


def bench_eval(graphs, dev, rounds, host_items):
    from vln_hamt_amd import ops
    tabs = dict_tables(graphs)
    s = graphs.scans.index("scanC")
    nx_ = graphs.nxt_host["scanC"]
    n = len(nx_)
    nbrs = [[y for y in range(n) if y != x and nx_[x, y] == y] for x in range(n)]
    name = lambda v: graphs.viewpoint("scanC", v)
    res = {}
    for N, P, G, tag in ((2349, 7, 6, "r2r_val_2349"), (45000, 40, 40, "r4r_like_45000_40x40")):
        rng = np.random.Generator(np.random.PCG64(N))
        base = [(walk(rng, nbrs, st, P), walk(rng, nbrs, st, G)) for st in (int(rng.integers(n)) for _ in range(min(N, 3000)))]
        items = [base[i % len(base)] for i in range(N)]
        n_host = min(N, host_items)
        paths, gts = [[name(v) for v in p] for p, _ in items], [[name(v) for v in g_] for _, g_ in items]
        sc, pa, pl = graphs.pack(["scanC"] * N, paths)
        _, ga, gl = graphs.pack(["scanC"] * N, gts)
        packed = [torch.from_numpy(a).to(dev) for a in (sc, pa, pl, ga, gl)]

        def host():
            return [host_eval_item(tabs[s][0], p, g_) for p, g_ in items[:n_host]]

        def device_from_names():
            return graphs.eval_items(["scanC"] * N, paths, gts).cpu()

        def device_launch():
            out = ops.nav_eval(graphs, *packed)
            torch.cuda.synchronize()
            return out
        want = host()
        got = device_from_names().numpy()
        ref = np.array([[w[c] for c in ops.NAV_EVAL_COLS] for w in want], np.float64)
        assert np.allclose(got[:n_host], ref, rtol=1e-12, atol=0, equal_nan=True)
        fns = {"host": host, "device_from_names": device_from_names, "device_launch": device_launch}
        reps = {k: _reps(f) for k, f in fns.items()}
        samples = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                samples[k].append(_sample(f, reps[k]) * 1e3 * (N / n_host if k == "host" else 1.0))
        r = {k: {"ms": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in samples.items()}
        r["host_items_timed"], r["host_scaled_by"], r["calls_per_sample"] = n_host, round(N / n_host, 3), reps
        r["device_not_slower"] = r["device_from_names"]["ms"] <= r["host"]["ms"]
        res[tag] = r
        print(f"[nav eval] {tag}: host {r['host']['ms']:.1f} ms (timed on {n_host} items, scaled)   device from names {r['device_from_names']['ms']:.2f} ms   "
              f"launch alone {r['device_launch']['ms']:.3f} ms", flush=True)
    return res


def bench_graphed(graphs, dev, rounds, iters, n_hist=10, B=8, L=160, feat=512, V=37, A=4):
    """tools/policy_step_bench.py's graphed inference step (visual -> RolloutRecorder.step(sync=False) -> history in ONE graph, then the copy
    of the environment action) without and with `nav=`: the cost of the two extra launches inside the graph."""
    from policy_step_bench import _live, _time
    from vln_hamt_amd.agent import NavEpisodes, RolloutRecorder
    from vln_hamt_amd.graph import GraphedInference
    from vln_hamt_amd.modeling import HamtConfig
    from vln_hamt_amd.models.vilmodel_cmt import NavCMT
    cfg = HamtConfig(hamt_precision="bf16", image_feat_size=feat, hist_enc_pano=True, num_h_pano_layers=2, no_lang_ca=True, act_pred_token="ob_txt",
                     fix_lang_embedding=False, fix_hist_embedding=False, fix_obs_embedding=False, update_lang_bert=True, vocab_size=250002 // 8 * 8)
    torch.manual_seed(0)
    model = NavCMT(cfg).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    r = lambda *sh: torch.randn(*sh, generator=g).to(dev)
    txt_ids = torch.randint(5, 30000, (B, L), generator=g).to(dev)
    txt_masks = torch.ones(B, L, dtype=torch.bool, device=dev)
    hist, hm = r(B, n_hist, 768), torch.ones(B, n_hist, dtype=torch.bool, device=dev)
    oi, oa, himg, pimg, pang = r(B, V, feat), r(B, V, A), r(B, feat), r(B, 36, feat), r(B, 36, A)
    navt = torch.zeros(B, V, dtype=torch.long, device=dev); navt[:, :6] = 1; navt[:, V - 1] = 2
    ob_masks = torch.ones(B, V, dtype=torch.bool, device=dev)
    sid = torch.tensor([n_hist - 1], device=dev)
    cl = torch.full((B,), V, dtype=torch.int32, device=dev)
    gts, steps = make_rollout(graphs, B, 7, 1, V, seed=3)
    cn = steps[0][2].copy()
    for b in range(B):                                                  # every slot a real neighbour: whatever the model chooses is a move
        k = int(steps[0][3][b]) - 1
        cn[b] = [cn[b, j % k] for j in range(V)]
    cn = torch.from_numpy(cn).to(dev)
    name = lambda v: graphs.viewpoint("scanC", v)
    out = {}
    with torch.no_grad():
        lang = model("language", txt_ids=txt_ids, txt_masks=txt_masks)
        visual = lambda h_, m_, i_, a_: model("visual", txt_embeds=lang, hist_embeds=h_, txt_masks=txt_masks, hist_masks=m_, ob_img_feats=i_,
                                               ob_ang_feats=a_, ob_nav_types=navt, ob_masks=ob_masks)[0]
        history = lambda i_, a_, p_, pa_: model("history", hist_img_feats=i_, hist_ang_feats=a_, ob_step_ids=sid, hist_pano_img_feats=p_, hist_pano_ang_feats=pa_)
        for fb in ("argmax", "sample"):
            recs = {"policy_step_only": RolloutRecorder(1, B, dev), "with_nav_observe_advance": RolloutRecorder(1, B, dev)}
            nav = NavEpisodes(graphs, 1, B, max_gt=64)
            reset_nav = lambda: nav.reset(["scanC"] * B, [name(g_[0]) for g_ in gts], [[name(v) for v in g_] for g_ in gts])
            reset_nav()

            def whole(h_, m_, i_, a_, hi_, p_, pa_, rec=recs["policy_step_only"], fb=fb):
                logit = visual(h_, m_, i_, a_)
                _, env, prev = rec.step(0, logit, cand_lens=cl, ob_ang_feats=a_, feedback=fb, sync=False)
                return env, history(hi_, prev, p_, pa_)

            def whole_nav(h_, m_, i_, a_, hi_, p_, pa_, rec=recs["with_nav_observe_advance"], fb=fb):
                logit = visual(h_, m_, i_, a_)
                _, env, prev = rec.step(0, logit, cand_lens=cl, ob_ang_feats=a_, feedback=fb, sync=False, nav=nav, cand_nodes=cn)
                return env, history(hi_, prev, p_, pa_)
            gws = {"policy_step_only": GraphedInference(whole, state=(recs["policy_step_only"].ended, recs["policy_step_only"].hist_len)),
                   "with_nav_observe_advance": GraphedInference(whole_nav, state=(recs["with_nav_observe_advance"].ended,
                                                                                  recs["with_nav_observe_advance"].hist_len, *nav.state_tensors()))}

            def step(k):
                env, h = gws[k]("w", hist, hm, oi, oa, himg, pimg, pang)
                return recs[k].to_host(env), h
            for k in gws:
                for _ in range(5):
                    step(k)
            samples = {k: [] for k in gws}
            for _ in range(rounds):
                for k in gws:
                    _live(recs[k])
                    reset_nav()                                         # (a one-step path buffer: every timed block starts from a fresh rollout)
                    torch.cuda.synchronize()
                    samples[k].append(_time(lambda k=k: step(k), iters))
            out[fb] = {k: {"us_per_step": round(statistics.median(x), 1), "min": round(min(x), 1), "max": round(max(x), 1)} for k, x in samples.items()}
            out[fb]["extra_us"] = round(out[fb]["with_nav_observe_advance"]["us_per_step"] - out[fb]["policy_step_only"]["us_per_step"], 1)
            print(f"[graphed step] B {B} {fb:7s}: " + "   ".join(f"{k} {v['us_per_step']:.1f} us ({v['min']:.1f}-{v['max']:.1f})"
                                                                  for k, v in out[fb].items() if isinstance(v, dict)), flush=True)
            del gws
    out["shape"] = {"B": B, "txt_len": L, "hist_tokens": n_hist, "views": V, "image_feat": feat}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--host-items", type=int, default=400)
    ap.add_argument("--no-graphed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nav_reward_bench: needs a GPU (no CPU fallback)")
    from vln_hamt_amd.agent import NavGraphs
    dev = torch.device("cuda")
    graphs = NavGraphs(CONNECTIVITY, device=dev)
    check_host_path_against_golden(graphs)
    res = {"workload": "navigation-graph side of a rollout step (teacher slot, back-track mask, reward shaping) and the evaluation metrics: "
                       "host Python loops over dict-of-dict distances vs ops.nav_observe + ops.nav_advance / ops.nav_eval",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "per_step": bench_steps(graphs, dev, a.rounds),
           "eval": bench_eval(graphs, dev, max(3, a.rounds // 2), a.host_items)}
    if not a.no_graphed:
        res["graphed_inference_step"] = bench_graphed(graphs, dev, max(3, a.rounds // 2), a.iters)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
