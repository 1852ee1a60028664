#!/usr/bin/env python3
"""What CVDN's / REVERIE's goal-set rollouts and R2R-Back's return trips read from the navigation graph around a step, and their
evaluation passes: the agents' host loops (dict-of-dict distances, as the reference keeps them) against the device path.

    python tools/nav_tasks_bench.py [--out profiles/nav_tasks_mi355x.json]

  host    (a) Python loops over the batch -- the teacher's slot and the visited-set mask (tools/nav_reward_bench.py's), then per task
          the statement sequence of cvdn/env.py:81-87 + cvdn/agent.py:174-203 (minimum over the goal set, the constant rewards) or of
          agent_r2rback.py:192-198 + :227-276 (mid-stop, two distances, cal_dtw over the path walked so far, `ended` / `first_ended`),
          and the uploads the model needs; cvdn / reverie / R2RBackBatch `_eval_item` per trajectory.  Checked against
          tests/golden/nav_tasks.npz (the reference's own statements) before anything is timed.
  device  (b) GoalSetEpisodes / ReturnEpisodes: one upload per rollout, ops.nav_observe + ops.nav_advance_goals / nav_advance_back per step;
          NavGraphs.eval_goal_items / ops.nav_eval_back per pass, from viewpoint names (pack, upload, one launch, download).
Cells: B in {8, 64} for both kinds of rollout (ground truth 7, 14 steps, on the 70-node test graph; time per step); one evaluation pass
per flavour at R2R-val size (N = 2 349).  Both paths alternate block by block in one process; the median over the rounds is reported
with the spread.  The condition is (b) <= (a) in every cell.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from nav_reward_bench import CONNECTIVITY, GOLDEN, IGNORE, HostEpisodes, _median, _reps, _sample, dict_tables, host_dtw, host_ndtw, make_rollout, walk


# ------------------------------------------------------------------------------------------------ the host paths
class HostGoalEpisodes(HostEpisodes):
    """cvdn/env.py:81-87 and cvdn/agent.py:52-55, :174-203 (= reverie/agent.py:337-366); `goals[i]` None = no end_panos"""

    def __init__(self, D, nxt, starts, gts, goals):
        self.D, self.nxt, self.B, self.gt, self.goals = D, nxt, len(starts), gts, goals
        self.here, self.path, self.visited = list(starts), [[s] for s in starts], [set() for _ in starts]
        self.last_dist, self.failed = np.zeros(self.B, np.float32), 0
        for i in range(self.B):
            self.last_dist[i] = self.distance(i)

    def distance(self, i):
        if self.goals[i] is None:
            return 0
        min_dist = np.inf
        for end_pano in self.goals[i]:
            min_dist = min(min_dist, self.D[i][self.here[i]][end_pano])
        return min_dist

    def advance(self, cands, cpu_a_t, ended):
        dist, reward = np.zeros(self.B, np.float32), np.zeros(self.B, np.float32)
        for i in range(self.B):
            if cpu_a_t[i] != -1:
                self.here[i] = cands[i][cpu_a_t[i]]
                self.path[i].append(self.here[i])
            dist[i] = self.distance(i)
            if ended[i]:
                reward[i] = 0.0
            elif cpu_a_t[i] == -1:
                reward[i] = 2.0 if dist[i] == 0.0 else -2.0
            else:
                reward[i] = -(dist[i] - self.last_dist[i])
                reward[i] = 1.0 if reward[i] > 0.0 else -1.0 if reward[i] < 0.0 else 0
        self.last_dist[:] = dist
        return reward, dist


class HostBackEpisodes(HostEpisodes):
    """agent_r2rback.py:104-113, :192-198, :227-276; `ended` and `first_ended` are the agent's own"""

    def __init__(self, D, nxt, starts, gts, mids):
        super().__init__(D, nxt, starts, gts)
        self.mids = mids
        self.midstop = [None] * self.B
        self.ended, self.first_ended = np.array([False] * self.B), np.array([False] * self.B)
        for i in range(self.B):
            self.last_dist[i] = D[i][starts[i]][mids[i]]

    def advance(self, cands, a_t, cand_len, train_rl=True):
        B = self.B
        cpu_a_t = np.array(a_t)
        for i, next_id in enumerate(cpu_a_t):
            if next_id == cand_len[i] - 1 or next_id == IGNORE or self.ended[i]:
                cpu_a_t[i] = -1
                if not self.first_ended[i]:
                    self.midstop[i] = self.here[i]
        dist, ndtw, reward, mask = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32), np.ones(B, np.float32)
        for i in range(B):
            if cpu_a_t[i] != -1:
                self.here[i] = cands[i][cpu_a_t[i]]
                self.path[i].append(self.here[i])
        if train_rl:
            for i in range(B):
                dist[i] = self.D[i][self.here[i]][self.gt[i][-1] if self.first_ended[i] else self.mids[i]]
                ndtw[i] = host_ndtw(self.D[i], self.path[i], self.gt[i])
                if self.ended[i]:
                    reward[i], mask[i] = 0.0, 0.0
                elif cpu_a_t[i] == -1:
                    if dist[i] < 3.0:
                        reward[i] = 2.0 + ndtw[i] * 2.0
                    else:
                        reward[i] = -2.0
                        self.ended[i] = True
                else:
                    reward[i] = -(dist[i] - self.last_dist[i])
                    shaped = ndtw[i] - self.last_ndtw[i]
                    reward[i] = (1.0 if reward[i] > 0.0 else -1.0 if reward[i] < 0.0 else 0.0) + shaped
                    if self.last_dist[i] <= 1.0 and dist[i] - self.last_dist[i] > 0.0:
                        reward[i] -= (1.0 - self.last_dist[i]) * 2.0
            self.last_ndtw[:] = ndtw
            self.last_dist[:] = dist
            for i in range(B):
                if not self.first_ended[i] and cpu_a_t[i] == -1:
                    self.last_dist[i] = self.D[i][self.here[i]][self.gt[i][-1]]
        self.ended[:] = np.logical_or(self.ended, self.first_ended * (cpu_a_t == -1))
        self.first_ended[:] = np.logical_or(self.first_ended, cpu_a_t == -1)
        return reward, dist, ndtw, mask, cpu_a_t


def host_eval_goals(D, path, goals, gt=None):
    goals = set(goals)
    s = {"trajectory_steps": len(path) - 1, "trajectory_lengths": np.sum([D[a][b] for a, b in zip(path[:-1], path[1:])])}
    glen = np.min([D[path[0]][e] for e in goals]) if gt is None else np.sum([D[a][b] for a, b in zip(gt[:-1], gt[1:])])
    s["success"] = float(path[-1] in goals)
    s["oracle_success"] = float(any(x in goals for x in path))
    s["spl"] = s["success"] * glen / max(s["trajectory_lengths"], glen, 0.01)
    s["gp"] = glen - np.min([D[path[-1]][e] for e in goals])
    s["spl_ratio"] = glen / max(s["trajectory_lengths"], glen, 0.01)
    return s


def host_eval_back(D, path, gt, midstop, gt_midstop):
    s = {"nav_error": D[path[-1]][gt[-1]], "trajectory_steps": len(path) - 1,
         "trajectory_lengths": np.sum([D[a][b] for a, b in zip(path[:-1], path[1:])])}
    glen = np.sum([D[a][b] for a, b in zip(gt[:-1], gt[1:])])
    s["success"] = int(midstop is not None and D[midstop][gt_midstop] <= 3.0 and D[path[-1]][gt[-1]] <= 3.0)
    s["spl"] = s["success"] * glen / max(s["trajectory_lengths"], glen, 0.01)
    s["DTW"] = host_dtw(D, path, gt)
    s["nDTW"] = np.exp(-s["DTW"] / (3.0 * len(gt)))
    s["SDTW"] = s["success"] * s["nDTW"]
    cover = np.mean([np.exp(-np.min([D[u][v] for v in path]) / 3.0) for u in gt])
    expected = cover * glen
    with np.errstate(invalid="ignore"):
        s["CLS"] = cover * (expected / (expected + np.abs(expected - s["trajectory_lengths"])))
    return s


def check_host_paths_against_golden(graphs):
    from vln_hamt_amd import ops
    z = np.load(os.path.join(GOLDEN, "nav_tasks.npz"))
    tabs = dict_tables(graphs)
    g = lambda k: z["goals/" + k]
    T, B, V = g("cand").shape
    cut = lambda a, n: [row[:k].tolist() for row, k in zip(a, n)]
    per = lambda scan, j: [tabs[s][j] for s in scan]
    goals = [e if e else None for e in cut(g("goals"), g("goal_len"))]
    for mode in ("path_step", "path_index", "shortest"):
        ep = HostGoalEpisodes(per(g("scan"), 0), per(g("scan"), 1), g("start").tolist(), cut(g("gt"), g("gt_len")), goals)
        assert np.array_equal(ep.last_dist, g("init_last_dist"))
        for t in range(T):
            cands = cut(g("cand")[t], g("cand_len")[t] - 1)
            a, bt = ep.observe(t, cands, g("ended")[t], mode, V)
            r, dist = ep.advance(cands, g("env_action")[t], g("ended")[t])
            assert np.array_equal(a, g(f"target/{mode}")[t]) and np.array_equal(bt, g("bt_mask")[t].astype(bool)), (mode, t)
            assert np.array_equal(dist, g("dist")[t]) and np.array_equal(r, g("reward")[t]), (mode, t)
    for prefix in ("back", "back_eval"):
        g = lambda k: z[prefix + "/" + k]
        T, B, V = g("cand").shape
        ep = HostBackEpisodes(per(g("scan"), 0), per(g("scan"), 1), g("start").tolist(), cut(g("gt"), g("gt_len")), g("midstop").tolist())
        for t in range(T):
            cands = cut(g("cand")[t], g("cand_len")[t] - 1)
            ep.observe(t, cands, ep.ended, "path_step", V)
            r, dist, ndtw, mask, env = ep.advance(cands, g("a_t")[t], g("cand_len")[t], train_rl=prefix == "back")
            assert np.array_equal(env, g("env_action")[t]) and np.array_equal(ep.ended, g("ended_after")[t]), (prefix, t)
            assert np.array_equal(ep.first_ended, g("first_ended_after")[t]), (prefix, t)
            assert [-1 if m is None else m for m in ep.midstop] == g("midstop_at")[t].tolist(), (prefix, t)
            if prefix == "back":
                assert np.array_equal(dist, g("dist")[t]) and np.array_equal(ep.last_dist, g("last_dist")[t]), t
                assert np.abs(ndtw - g("ndtw")[t]).max() <= 2.4e-7 and np.abs(r - g("reward")[t]).max() <= 1e-6, t
    close = lambda got, want: np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    for flavour, cols in (("cvdn", ops.NAV_GOALS_EVAL_COLS[:6]), ("reverie", ops.NAV_GOALS_EVAL_COLS[:5]), ("backm", ops.NAV_BACK_EVAL_COLS)):
        e = lambda k: z[flavour + "/" + k]
        for i in range(len(e("scan"))):
            D, path = tabs[e("scan")[i]][0], e("path")[i, :e("path_len")[i]].tolist()
            if flavour == "backm":
                mid = None if e("midstop")[i] < 0 else int(e("midstop")[i])
                s = host_eval_back(D, path, e("gt")[i, :e("gt_len")[i]].tolist(), mid, int(e("gt_midstop")[i]))
            else:
                s = host_eval_goals(D, path, e("goals")[i, :e("goal_len")[i]].tolist(), e("gt")[i, :e("gt_len")[i]].tolist() if flavour == "reverie" else None)
            assert close(np.array([s[c] for c in cols], np.float64), e("metrics")[i, :len(cols)]), (flavour, i)
    print("[nav tasks bench] the host paths reproduce tests/golden/nav_tasks.npz", flush=True)


# ------------------------------------------------------------------------------------------------ the cells
def bench_rollouts(graphs, dev, rounds):
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import GoalSetEpisodes, ReturnEpisodes
    tabs = dict_tables(graphs)
    s = graphs.scans.index("scanC")
    name = lambda v: graphs.viewpoint("scanC", v)
    res, V, G, T = {}, 9, 7, 14
    for B in (8, 64):
        gts, steps = make_rollout(graphs, B, G, T, V, seed=B + G)
        rng = np.random.Generator(np.random.PCG64(B))
        goal_sets = [[int(v) for v in rng.integers(70, size=(1, 3, 12, 40)[b % 4])] for b in range(B)]        # REVERIE: tens of viewpoints
        mids = [gt[G // 2] for gt in gts]
        scans, starts, gt_names = ["scanC"] * B, [name(g_[0]) for g_ in gts], [[name(v) for v in g_] for g_ in gts]
        goal_names, mid_names = [[name(v) for v in e] for e in goal_sets], [name(v) for v in mids]
        # return trips: everyone stops at step 4 (the mid-stop: hit or missed) and again at the last step
        a_back = [np.where(np.full(B, t in (4, T - 1)), cl - 1, act).astype(np.int64) for t, (_, act, _, cl) in enumerate(steps)]
        dev_steps = [(torch.from_numpy(cn).to(dev), torch.from_numpy(cl).to(dev), torch.from_numpy(act).to(dev)) for _, act, cn, cl in steps]
        ended0 = np.zeros(B, bool)
        ended_d, mask_d = torch.zeros(B, dtype=torch.uint8, device=dev), torch.ones(B, dtype=torch.float32, device=dev)
        reward_d = torch.zeros(T, B, dtype=torch.float32, device=dev)
        nav_g, nav_b = GoalSetEpisodes(graphs, T, B, max_gt=64, max_goals=64), ReturnEpisodes(graphs, T, B, max_gt=64)
        D, nxt = [tabs[s][0]] * B, [tabs[s][1]] * B

        def host_goals():
            ep = HostGoalEpisodes(D, nxt, [g_[0] for g_ in gts], gts, goal_sets)
            rewards = []
            for t, (cands, act, _, _) in enumerate(steps):
                a, bt = ep.observe(t, cands, ended0, "path_step", V)
                torch.from_numpy(a).to(dev, non_blocking=True)
                torch.from_numpy(bt).to(dev, non_blocking=True)
                rewards.append(ep.advance(cands, act, ended0)[0])
            torch.from_numpy(np.stack(rewards)).to(dev, non_blocking=True)
            torch.cuda.synchronize()
            return np.stack(rewards)

        def device_goals():
            nav_g.reset(scans, starts, gt_names, goal_names)
            for t, (cn, cl, act) in enumerate(dev_steps):
                ops.nav_observe(nav_g, t, cn, cl, ended_d, mode="path_step")
                ops.nav_advance_goals(nav_g, cn, act, mask_d, reward_d[t])
            torch.cuda.synchronize()

        def host_back():
            ep = HostBackEpisodes(D, nxt, [g_[0] for g_ in gts], gts, mids)
            rewards, masks = [], []
            for t, (cands, _, _, cl) in enumerate(steps):
                a, bt = ep.observe(t, cands, ep.ended, "path_step", V)
                torch.from_numpy(a).to(dev, non_blocking=True)
                torch.from_numpy(bt).to(dev, non_blocking=True)
                r, _, _, m, _ = ep.advance(cands, a_back[t], cl)
                rewards.append(r)
                masks.append(m)
            torch.from_numpy(np.stack(rewards)).to(dev, non_blocking=True)
            torch.cuda.synchronize()
            return np.stack(rewards), np.stack(masks), ep

        # what the policy step hands the return-trip launch, step by step (it is not part of either path): env action, mask, ended |= stop
        ep = HostBackEpisodes(D, nxt, [g_[0] for g_ in gts], gts, mids)
        back_steps = []
        for t, (cands, _, cn, cl) in enumerate(steps):
            before = ep.ended.copy()
            env = ep.advance(cands, a_back[t], cl)[4]
            back_steps.append((dev_steps[t][0], dev_steps[t][1], torch.from_numpy(env.astype(np.int32)).to(dev),
                               torch.from_numpy((~before).astype(np.float32)).to(dev), torch.from_numpy((before | (env < 0)).astype(np.uint8)).to(dev),
                               torch.from_numpy(before.astype(np.uint8)).to(dev)))
        ended_b = torch.zeros(B, dtype=torch.uint8, device=dev)

        def device_back():
            nav_b.reset(scans, starts, gt_names, mid_names)
            for t, (cn, cl, env, mask, after_policy, before) in enumerate(back_steps):
                ops.nav_observe(nav_b, t, cn, cl, before, mode="path_step")
                ended_b.copy_(after_policy)
                ops.nav_advance_back(nav_b, cn, env, mask, reward_d[t], ended_b, end_on_miss=True)
            torch.cuda.synchronize()
        for tag, host, device in (("goal_set", host_goals, device_goals), ("return_trip", host_back, device_back)):
            reps = {"host": _reps(host), "device": _reps(device)}
            samples = {"host": [], "device": []}
            for _ in range(rounds):
                for k, f in (("host", host), ("device", device)):          # alternating, same process
                    samples[k].append(_sample(f, reps[k]) / T * 1e6)
            want = host()
            want = want if tag == "goal_set" else want[0]
            device()
            err = float(np.abs(reward_d.cpu().numpy() - want).max())
            assert err <= (0.0 if tag == "goal_set" else 1e-6), (tag, err)
            if tag == "return_trip":
                assert np.array_equal(ended_b.cpu().numpy().astype(bool), ep.ended) and ep.ended.any()
            r = {k: _median(v) for k, v in samples.items()}
            r["device_not_slower"] = r["device"]["us"] <= r["host"]["us"]
            r["max_reward_difference"], r["rollouts_per_sample"] = err, reps
            res[f"B{B}_{tag}"] = r
            print(f"[nav tasks step] B {B:2d} {tag:11s}: host {r['host']['us']:9.1f} us/step ({r['host']['min']:.1f}-{r['host']['max']:.1f})   "
                  f"device {r['device']['us']:7.1f} us/step ({r['device']['min']:.1f}-{r['device']['max']:.1f}; reset included)", flush=True)
    return res


def bench_eval(graphs, dev, rounds, N=2349, P=7, G=6):
    from vln_hamt_amd import ops
    tabs = dict_tables(graphs)
    s = graphs.scans.index("scanC")
    nx_ = graphs.nxt_host["scanC"]
    n = len(nx_)
    nbrs = [[y for y in range(n) if y != x and nx_[x, y] == y] for x in range(n)]
    name = lambda v: graphs.viewpoint("scanC", v)
    rng = np.random.Generator(np.random.PCG64(N))
    items = []
    for _ in range(N):
        st = int(rng.integers(n))
        gt = walk(rng, nbrs, st, G)
        p = walk(rng, nbrs, st, P)
        goals = sorted({gt[-1], *(int(v) for v in rng.integers(n, size=int(rng.integers(1, 30))))})
        items.append((p, gt, goals, None if rng.random() < 0.1 else p[int(rng.integers(P))], gt[G // 2]))
    scans = ["scanC"] * N
    names = lambda k: [[name(v) for v in it[k]] for it in items]
    paths, gts, goal_names = names(0), names(1), names(2)
    preds = [{"instr_id": str(i), "trajectory": [(v,) for v in p], "midstop": None if it[3] is None else name(it[3])} for i, (p, it) in enumerate(zip(paths, items))]
    gt_trajs, gt_mid = {str(i): ("scanC", g_) for i, g_ in enumerate(gts)}, {str(i): name(it[4]) for i, it in enumerate(items)}
    D = tabs[s][0]
    cells = {
        "cvdn": (lambda: [host_eval_goals(D, p, e) for p, _, e, _, _ in items], lambda: graphs.eval_goal_items(scans, paths, goal_names).cpu(),
                 ops.NAV_GOALS_EVAL_COLS),
        "reverie": (lambda: [host_eval_goals(D, p, e, g_) for p, g_, e, _, _ in items], lambda: graphs.eval_goal_items(scans, paths, goal_names, gts).cpu(),
                    ops.NAV_GOALS_EVAL_COLS),
        "r2r_back": (lambda: [host_eval_back(D, p, g_, m, gm) for p, g_, _, m, gm in items],
                     lambda: np.stack([np.asarray(graphs.eval_metrics_back(preds, gt_trajs, gt_mid)[1][c], np.float64) for c in ops.NAV_BACK_EVAL_COLS], 1),
                     ops.NAV_BACK_EVAL_COLS),
    }
    res = {}
    for tag, (host, device, cols) in cells.items():
        ref = np.array([[w[c] for c in cols] for w in host()], np.float64)
        assert np.allclose(np.asarray(device()), ref, rtol=1e-12, atol=0, equal_nan=True), tag
        fns = {"host": host, "device_from_names": device}
        reps = {k: _reps(f) for k, f in fns.items()}
        samples = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                samples[k].append(_sample(f, reps[k]) * 1e3)
        r = {k: {"ms": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in samples.items()}
        r["calls_per_sample"], r["device_not_slower"] = reps, r["device_from_names"]["ms"] <= r["host"]["ms"]
        res[f"{tag}_val_{N}"] = r
        print(f"[nav tasks eval] {tag} N {N}: host {r['host']['ms']:.1f} ms ({r['host']['min']:.1f}-{r['host']['max']:.1f})   "
              f"device from names {r['device_from_names']['ms']:.2f} ms ({r['device_from_names']['min']:.2f}-{r['device_from_names']['max']:.2f})", flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nav_tasks_bench: needs a GPU (no CPU fallback)")
    from vln_hamt_amd.agent import NavGraphs
    dev = torch.device("cuda")
    graphs = NavGraphs(CONNECTIVITY, device=dev)
    check_host_paths_against_golden(graphs)
    res = {"workload": "navigation-graph side of CVDN / REVERIE goal-set rollouts and R2R-Back return trips (teacher slot, back-track mask, "
                       "distance and reward, mid-stop book-keeping) and their evaluation metrics: host Python loops over dict-of-dict "
                       "distances vs ops.nav_observe + ops.nav_advance_goals / nav_advance_back and ops.nav_eval_goals / nav_eval_back",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "per_step": bench_rollouts(graphs, dev, a.rounds),
           "eval": bench_eval(graphs, dev, max(3, a.rounds // 2))}
    res["device_not_slower_in_every_cell"] = all(c["device_not_slower"] for part in ("per_step", "eval") for c in res[part].values())
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
