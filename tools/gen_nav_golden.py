#!/usr/bin/env python3
"""Generate tests/golden/nav_reward.npz (and, once, the synthetic 70-node graph tests/golden/nav_tiny/) by running the REFERENCE's own
statements around a rollout step and its evaluation on scripted rollouts, CPU.

Test infrastructure, like tools/gen_policy_step_golden.py (needs the reference checkout, oracle.ref_shim.REF, and networkx):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_nav_golden.py

Nothing of the reference is restated: every piece below is cut out of its FILE at generation time (located by its first and last
statement, not by line number) and compiled --
  eval_utils.py   `cal_dtw`, `cal_cls` (as functions: the module imports MatterSim);
  data_utils.py   `load_nav_graphs` (networkx graphs; nx.all_pairs_dijkstra_* give distances and paths, as env.py:142-147);
  env.py          `ERROR_MARGIN`, `_shortest_path_action`, `_teacher_path_action`, `_get_nearest`, `_eval_item`, `eval_metrics`;
  agent_cmt.py    `_teacher_action`; the back-track block (`if self.args.no_cand_backtrack:` ... `bt_masks[ob_id][c_id] = True`);
                  the init block (`last_dist = np.zeros(` ... `last_ndtw[i] = cal_dtw(`); the reward block (`if train_rl:` ...
                  `last_ndtw[:] = ndtw_score`).
What is scripted: the simulator.  In the Matterport graph a move is deterministic, so the stand-in is three lines: the candidates of
a viewpoint are its neighbours (shuffled per step), and the chosen candidate's viewpoint is where the episode stands next, appended
to `traj` as make_equiv_action does.  B = 6 episodes over all three scans, T = 7, each following a plan of 'gt' / 'closer' / 'away' /
'back' / 'stop' moves chosen so that every branch of the reward block is taken (checked at the end); the teacher is asked in all
three modes of `_teacher_path_action` at every step, and where `_teacher_action`'s assert fires the golden records that instead of
a slot.  The eval part scores 42 scripted trajectories through `eval_metrics`.

Node ids in the golden are positions in the scan's connectivity file among the nodes that have an edge.
"""
import json
import os
import sys
import textwrap
import types
import warnings

import networkx as nx
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import ref_shim                                            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "nav_reward.npz")
TINY = os.path.join(ROOT, "tests", "golden", "r2r_tiny")
NAV_TINY = os.path.join(ROOT, "tests", "golden", "nav_tiny")
SCANS = (("scanA", TINY), ("scanB", TINY), ("scanC", NAV_TINY))
B, T = 6, 7
IGNORE = -100
MODES = ("path_step", "path_index", "shortest")


# ------------------------------------------------------------------------------------------------ the synthetic graph (data)
def write_synthetic_graph(n=70, seed=5):
    """70 nodes at seeded positions in a 12 m x 12 m x 1 m box, each linked to its 3 nearest neighbours (symmetrised; components, if
    any, joined at their closest pair), plus one excluded node -- in the connectivity-file format of the Matterport scans."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xyz = rng.random((n, 3)) * np.array([12.0, 12.0, 1.0])
    d = np.linalg.norm(xyz[:, None] - xyz[None], axis=2)
    link = np.zeros((n, n), bool)
    for i in range(n):
        for j in np.argsort(d[i])[1:4]:
            link[i, j] = link[j, i] = True
    while True:
        comp = list(nx.connected_components(nx.from_numpy_array(link)))
        if len(comp) == 1:
            break
        a = sorted(comp[0])
        rest = sorted(set(range(n)) - comp[0])
        i, j = np.unravel_index(np.argmin(d[np.ix_(a, rest)]), (len(a), len(rest)))
        link[a[i], rest[j]] = link[rest[j], a[i]] = True
    nodes = []
    for i in range(n + 1):
        pose = [0.0] * 16
        if i < n:
            pose[3], pose[7], pose[11] = (float(v) for v in xyz[i])
        nodes.append({"image_id": f"c{i:02d}" if i < n else "excluded", "pose": pose, "included": i < n,
                      "unobstructed": [bool(i < n and j < n and link[i, j]) for j in range(n + 1)]})
    os.makedirs(NAV_TINY, exist_ok=True)
    with open(os.path.join(NAV_TINY, "scanC_connectivity.json"), "w") as f:
        json.dump(nodes, f)
    with open(os.path.join(NAV_TINY, "scans.txt"), "w") as f:
        f.write("scanC\n")


# ------------------------------------------------------------------------------------------------ the reference's statements
def _block(lines, first, last, start=0):
    lo = next(i for i, ln in enumerate(lines) if i >= start and ln.strip().startswith(first))
    hi = next(i for i, ln in enumerate(lines) if i >= lo and ln.strip().startswith(last))
    return textwrap.dedent("\n".join(lines[lo:hi + 1])), (lo + 1, hi + 1)


def reference_pieces():
    """-> (namespace of the reference's functions, compiled blocks of agent_cmt.py's rollout, spans)"""
    src = lambda *p: open(os.path.join(ref_shim.REF, "finetune_src", "r2r", *p)).read().split("\n")
    spans, fn = {}, {"np": np, "nx": nx, "os": os, "json": json, "torch": torch}
    fn["defaultdict"] = __import__("collections").defaultdict

    def define(lines, path, first, last, start=0):
        text, span = _block(lines, first, last, start)
        exec(compile(text, f"{path}:{span[0]}-{span[1]}", "exec"), fn)
        spans[first.split("(")[0].replace("def ", "")] = span

    ev, du, env, ag = src("eval_utils.py"), src("data_utils.py"), src("env.py"), src("agent_cmt.py")
    define(ev, "eval_utils.py", "def cal_dtw(", "}")
    define(ev, "eval_utils.py", "def cal_cls(", "return coverage * score")
    define(du, "data_utils.py", "def load_nav_graphs(", "return graphs")
    define(env, "env.py", "ERROR_MARGIN =", "ERROR_MARGIN =")
    at = next(i for i, ln in enumerate(env) if ln.startswith("class R2RBatch"))
    for first, last in (("def _shortest_path_action(", "return nextViewpointId"), ("def _teacher_path_action(", "return teacher_vp"),
                        ("def _get_nearest(", "return near_id"), ("def _eval_item(", "return scores"), ("def eval_metrics(", "return avg_metrics, metrics")):
        define(env, "env.py", first, last, at)
    define(ag, "agent_cmt.py", "def _teacher_action(", "return torch.from_numpy(a).cuda()")
    loop = next(i for i, ln in enumerate(ag) if ln.strip() == "for t in range(self.args.max_action_len):")
    blocks = {}
    for key, first, last, start in (("init", "last_dist = np.zeros(batch_size, np.float32)", "last_ndtw[i] = cal_dtw(", 0),
                                    ("backtrack", "if self.args.no_cand_backtrack:", "bt_masks[ob_id][c_id] = True", loop),
                                    ("reward", "if train_rl:", "last_ndtw[:] = ndtw_score", loop)):
        text, spans[key] = _block(ag, first, last, start)
        blocks[key] = compile(text, f"agent_cmt.py:{spans[key][0]}-{spans[key][1]}", "exec")
    assert "raise NameError" in _block(ag, "if train_rl:", "last_ndtw[:] = ndtw_score", loop)[0], "agent_cmt.py changed"
    return fn, blocks, spans


class World:
    """the reference's graphs, distances and paths (env.py:139-147) behind the attributes its methods read"""

    def __init__(self, fn):
        self.fn = fn
        self.graphs, self.shortest_paths, self.shortest_distances, self.order = {}, {}, {}, {}
        for scan, d in SCANS:
            G = fn["load_nav_graphs"](d, [scan])[scan]
            self.graphs[scan] = G
            self.shortest_paths[scan] = dict(nx.all_pairs_dijkstra_path(G))
            self.shortest_distances[scan] = dict(nx.all_pairs_dijkstra_path_length(G))
            with open(os.path.join(d, f"{scan}_connectivity.json")) as f:
                self.order[scan] = [nd["image_id"] for nd in json.load(f) if nd["image_id"] in G]
        self.ix = {s: {v: i for i, v in enumerate(o)} for s, o in self.order.items()}
        for name in ("_shortest_path_action", "_teacher_path_action", "_get_nearest", "_eval_item", "eval_metrics"):
            setattr(self, name, types.MethodType(fn[name], self))

    def dist(self, scan, a, b):
        return self.shortest_distances[scan][a][b]


# ------------------------------------------------------------------------------------------------ the scripted rollouts
def episodes(w):
    """(scan, ground-truth path, plan) per episode.  The plans are chosen for the corners the test asserts; main() checks them."""
    C = w.shortest_paths["scanC"]
    far = max(w.order["scanC"], key=lambda v: w.dist("scanC", "c00", v))
    walk = C["c00"][far] + C[far]["c35"][1:] + C["c35"]["c10"][1:] + C["c10"][far][1:]          # a long ground truth with revisits
    walk = (walk + C[walk[-1]]["c00"][1:] + C["c00"]["c60"][1:] + C["c60"]["c20"][1:] + C["c20"]["c50"][1:])
    assert len(walk) >= 66, len(walk)
    walk = walk[:66]                                                     # crosses 64 lanes
    # an edge of at most 1 m whose far end has a neighbour further from the goal: the miss-the-target penalty
    G = w.graphs["scanC"]
    goal3, start3 = min(((a, b_) for a, b_ in G.edges if G[a][b_]["weight"] <= 1.0 and G.degree[b_] > 1), key=lambda e: G[e[0]][e[1]]["weight"])
    far3 = max(w.order["scanC"], key=lambda v: w.dist("scanC", v, goal3))
    return [
        ("scanA", ["a00", "a01", "a02", "a03"], ["gt", "gt", "gt", "stop"]),                    # a correct stop, then steps after the end
        ("scanB", ["b00", "b02", "b03"], ["gt", "away", "stop"]),                               # a wrong stop
        ("scanC", walk, ["gt"] * T),                                                            # never ends
        ("scanC", C[far3][goal3] + [start3], ["away", "back", "away", "closer", "closer", "stop"]),     # starts <= 1 m from its goal... (see main)
        ("scanA", ["a00", "a02", "a06"], ["off", "back", "gt", "away", "closer", "closer", "stop"]),    # leaves the path (path_index: no teacher)
        ("scanC", ["c07"], ["away", "back", "stop"]),                                           # a one-node ground truth: t >= gt_len - 1 from the start
    ], (goal3, start3)


def choose(w, scan, here, prev, goal, gt, t, move, visited):
    """the viewpoint a plan's move leads to (None = stop)"""
    nb = sorted(w.graphs[scan][here])
    d = lambda v: w.dist(scan, v, goal)
    if move == "stop":
        return None
    if move == "gt":
        return gt[gt.index(here) + 1] if t is None else gt[t + 1]
    if move == "back":
        return prev
    if move == "closer":
        return min(nb, key=d)
    if move == "away":
        return max(nb, key=d)
    if move == "off":
        return next(v for v in nb if v not in gt)
    raise ValueError(move)


def rollout(w, fn, blocks):
    eps, (goal3, start3) = episodes(w)
    eps[3] = ("scanC", eps[3][1][:-1], eps[3][2])                      # episode 3: ground truth ends at goal3 ...
    starts = [e[1][0] for e in eps]
    starts[3] = start3                                                 # ... and the episode starts next to it, off the ground truth's start
    rng = np.random.Generator(np.random.PCG64(17))
    here, prev = list(starts), [None] * B
    traj = [{"path": [(v, 0.0, 0.0)]} for v in starts]
    ended = np.array([False] * B)
    visited = [set() for _ in range(B)]
    me = types.SimpleNamespace(args=types.SimpleNamespace(ignoreid=IGNORE, no_cand_backtrack=True),
                               env=types.SimpleNamespace(shortest_distances=w.shortest_distances))
    teacher_action = types.MethodType(fn["_teacher_action"], me)

    def observe(t, mode):
        obs = []
        for i, (scan, gt, _) in enumerate(eps):
            state = types.SimpleNamespace(scanId=scan, location=types.SimpleNamespace(viewpointId=here[i]))
            teacher = w._teacher_path_action(state, gt, t=t if mode == "path_step" else None, shortest_teacher=mode == "shortest")
            obs.append({"scan": scan, "viewpoint": here[i], "candidate": cands[i], "teacher": teacher, "gt_path": gt,
                        "distance": w.dist(scan, here[i], gt[-1])})
        return obs

    def shuffled_candidates():
        out = []
        for i, (scan, _, _) in enumerate(eps):
            nb = sorted(w.graphs[scan][here[i]])
            out.append([{"viewpointId": nb[j]} for j in rng.permutation(len(nb))])
        return out

    cands = shuffled_candidates()
    ns = {"np": np, "torch": torch, "self": me, "cal_dtw": fn["cal_dtw"], "batch_size": B, "obs": observe(0, "path_step"), "traj": traj,
          "train_rl": True, "ended": ended, "visited": visited}
    exec(blocks["init"], ns)
    rec = {k: [] for k in ("cand", "cand_len", "a_t", "env_action", "ended", "bt_mask", "dist", "ndtw", "reward", "mask", "cur", "moved")}
    rec.update({f"target/{m}": [] for m in MODES})
    rec.update({f"assert/{m}": [] for m in MODES})
    init = {"last_dist": ns["last_dist"].copy(), "last_ndtw": ns["last_ndtw"].copy()}
    for t in range(T):
        for mode in MODES:
            obs = observe(t, mode)
            tgt, fired = np.zeros(B, np.int64), np.zeros(B, bool)
            for i in range(B):                                          # per episode: an assert of one must not hide the others' answers
                try:
                    with ref_shim.cuda_is_identity():
                        tgt[i] = int(teacher_action([obs[i]], [ended[i]])[0])
                except AssertionError:
                    tgt[i], fired[i] = IGNORE, True
            rec[f"target/{mode}"].append(tgt)
            rec[f"assert/{mode}"].append(fired)
        ns.update(obs=observe(t, "path_step"), ob_nav_types=torch.zeros(B, VMAX))
        exec(blocks["backtrack"], ns)
        rec["bt_mask"].append(ns["bt_masks"].numpy().astype(np.uint8))
        rec["cur"].append([w.ix[eps[i][0]][here[i]] for i in range(B)])
        cn = np.full((B, VMAX), -1, np.int32)
        a_t, cpu_a_t = np.zeros(B, np.int64), np.zeros(B, np.int64)
        for i, (scan, gt, plan) in enumerate(eps):
            cn[i, :len(cands[i])] = [w.ix[scan][c["viewpointId"]] for c in cands[i]]
            nxt_vp = None if ended[i] or t >= len(plan) else choose(w, scan, here[i], prev[i], gt[-1], gt, t if i == 2 else None, plan[t], visited[i])
            a_t[i] = len(cands[i]) if nxt_vp is None else [c["viewpointId"] for c in cands[i]].index(nxt_vp)
            cpu_a_t[i] = -1 if nxt_vp is None else a_t[i]               # (:372-375)
        rec["cand"].append(cn)
        rec["cand_len"].append(np.array([len(c) + 1 for c in cands], np.int32))
        rec["a_t"].append(a_t)
        rec["env_action"].append(cpu_a_t.astype(np.int32))
        rec["ended"].append(ended.copy())
        moved = np.zeros(B, bool)
        for i, a in enumerate(cpu_a_t):                                 # the stand-in for make_equiv_action + the simulator
            if a != -1:
                prev[i], here[i] = here[i], cands[i][a]["viewpointId"]
                traj[i]["path"].append((here[i], 0.0, 0.0))
                moved[i] = True
        rec["moved"].append(moved)
        cands = shuffled_candidates()
        ns.update(obs=observe(t + 1, "path_step"), cpu_a_t=cpu_a_t, rewards=[], masks=[])
        exec(blocks["reward"], ns)
        before = rec["dist"][-1] if rec["dist"] else init["last_dist"]
        for i in range(B):                                              # no scripted move leaves the fp32 distance unchanged (the reference raised otherwise)
            assert not moved[i] or ns["dist"][i] != before[i], (t, i)
        rec["dist"].append(ns["dist"].copy())
        rec["ndtw"].append(ns["ndtw_score"].copy())
        rec["reward"].append(ns["rewards"][0].copy())
        rec["mask"].append(ns["masks"][0].copy())
        ended[:] = np.logical_or(ended, cpu_a_t == -1)                  # (:447)
    out = {f"roll/{k}": np.stack([np.asarray(x) for x in v]) for k, v in rec.items()}
    out["roll/init_last_dist"], out["roll/init_last_ndtw"] = init["last_dist"], init["last_ndtw"]
    out["roll/scan"] = np.array([[s for s, _ in SCANS].index(e[0]) for e in eps], np.int32)
    out["roll/start"] = np.array([w.ix[e[0]][v] for e, v in zip(eps, starts)], np.int32)
    gl = np.array([len(e[1]) for e in eps], np.int32)
    gt = np.full((B, gl.max()), -1, np.int32)
    for i, e in enumerate(eps):
        gt[i, :gl[i]] = [w.ix[e[0]][v] for v in e[1]]
    out["roll/gt"], out["roll/gt_len"] = gt, gl
    pl = np.array([len(tr["path"]) for tr in traj], np.int32)
    path = np.full((B, T + 1), -1, np.int32)
    for i, tr in enumerate(traj):
        path[i, :pl[i]] = [w.ix[eps[i][0]][v[0]] for v in tr["path"]]
    out["roll/path"], out["roll/path_len"], out["roll/final_ended"] = path, pl, ended.copy()
    return out


VMAX = 0


# ------------------------------------------------------------------------------------------------ the scored trajectories
def eval_cases(w):
    rng = np.random.Generator(np.random.PCG64(29))

    def walk(scan, start, n, revisit=0.3):
        p = [start]
        while len(p) < n:
            nb = sorted(w.graphs[scan][p[-1]])
            fresh = [v for v in nb if v not in p]
            p.append(str(rng.choice(fresh if fresh and rng.random() > revisit else nb)))
        return p

    cases = [("scanC", ["c11"], ["c11"])]                                                       # the NaN corner: CLS = 0 / 0
    cases.append(("scanC", ["c11"], walk("scanC", "c11", 5)))                                   # a one-node path against a real ground truth
    cases.append(("scanA", ["a00", "a01", "a02", "a03"], ["a00", "a01", "a02", "a03"]))         # the ground truth itself
    cases.append(("scanA", ["a00", "a01"], ["a00", "a01", "a02", "a03"]))                       # shorter than the ground truth
    cases.append(("scanA", ["a00", "a01", "a04", "a03", "a02", "a03"], ["a00", "a01", "a02", "a03"]))     # longer, success
    cases.append(("scanB", ["b00", "b01", "b00", "b02", "b00"], ["b00", "b02", "b03"]))         # revisits, ends at the start
    for pn in (1, 2, 63, 64, 65, 130):
        for gn in (2, 64, 65, 130):
            start = w.order["scanC"][int(rng.integers(70))]
            cases.append(("scanC", walk("scanC", start, pn), walk("scanC", start, gn, revisit=0.1)))
    for _ in range(12):
        scan = ("scanA", "scanB", "scanC")[int(rng.integers(3))]
        start = w.order[scan][int(rng.integers(len(w.order[scan])))]
        gt = walk(scan, start, int(rng.integers(2, 9)), revisit=0.0)
        n = int(rng.integers(1, 12))
        cases.append((scan, (gt[:n] if rng.random() < 0.5 else walk(scan, start, n)), gt))
    return cases


def evaluate(w, cases):
    w.gt_trajs = {f"i{k}": (scan, gt) for k, (scan, _, gt) in enumerate(cases)}
    preds = [{"instr_id": f"i{k}", "trajectory": [(v, 0.0, 0.0) for v in p]} for k, (_, p, _) in enumerate(cases)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # (the NaN corner divides 0 by 0)
        avg, metrics = w.eval_metrics(preds)
    cols = ("nav_error", "oracle_error", "trajectory_steps", "trajectory_lengths", "success", "spl", "oracle_success", "DTW", "nDTW", "SDTW", "CLS")
    assert list(metrics)[:11] == list(cols), list(metrics)             # the column order is _eval_item's own key order
    N = len(cases)
    pl, gl = np.array([len(c[1]) for c in cases], np.int32), np.array([len(c[2]) for c in cases], np.int32)
    path, gt = np.full((N, pl.max()), -1, np.int32), np.full((N, gl.max()), -1, np.int32)
    for k, (scan, p, g) in enumerate(cases):
        path[k, :pl[k]] = [w.ix[scan][v] for v in p]
        gt[k, :gl[k]] = [w.ix[scan][v] for v in g]
    return {"eval/scan": np.array([[s for s, _ in SCANS].index(c[0]) for c in cases], np.int32), "eval/path": path.astype(np.int16),
            "eval/path_len": pl, "eval/gt": gt.astype(np.int16), "eval/gt_len": gl,
            "eval/metrics": np.stack([np.asarray(metrics[c], np.float64) for c in cols], 1),
            "eval/avg_keys": np.array(list(avg)), "eval/avg": np.array([avg[k] for k in avg], np.float64)}


def main():
    global VMAX
    if not os.path.exists(os.path.join(NAV_TINY, "scanC_connectivity.json")):
        write_synthetic_graph()
    fn, blocks, spans = reference_pieces()
    w = World(fn)
    VMAX = max(max(dict(G.degree).values()) for G in w.graphs.values()) + 1
    store = {"meta/ignoreid": np.array(IGNORE), "meta/scans": np.array([s for s, _ in SCANS])}
    for k, v in spans.items():
        store["meta/span/" + k] = np.asarray(v)
    gap = np.inf
    for scan, _ in SCANS:
        order, n = w.order[scan], len(w.order[scan])
        store[f"graph/{scan}/nodes"] = np.array(order)
        store[f"graph/{scan}/dist"] = np.array([[w.dist(scan, a, b_) for b_ in order] for a in order], np.float64)
        store[f"graph/{scan}/next"] = np.array([[w.ix[scan][w.shortest_paths[scan][a][b_][1]] if a != b_ else i for b_ in order]
                                                for i, a in enumerate(order)], np.int16)
        G = w.graphs[scan]
        for a in order:                                                 # how close the runner-up neighbour comes to the shortest path's first hop
            for b_ in order:
                via = sorted(G[a][k]["weight"] + w.dist(scan, k, b_) for k in G[a])
                if a != b_ and len(via) > 1:
                    gap = min(gap, via[1] - via[0])
    store["meta/next_hop_gap"] = np.float64(gap)
    roll = rollout(w, fn, blocks)
    store.update(roll)
    cases = eval_cases(w)
    store.update(evaluate(w, cases))

    # ---- the corners are really there
    r, m, env, d = roll["roll/reward"], roll["roll/mask"], roll["roll/env_action"], roll["roll/dist"]
    last = np.concatenate([roll["roll/init_last_dist"][None], d[:-1]])
    live = m == 1
    assert (live & (env == -1) & (d < 3.0)).any(), "no correct stop"
    assert (live & (env == -1) & (d >= 3.0) & (r == -2.0)).any(), "no wrong stop"
    assert (live & (env >= 0) & (d < last)).any() and (live & (env >= 0) & (d > last)).any(), "no move closer / away"
    assert (live & (env >= 0) & (last <= 1.0) & (d > last)).any(), "no miss-the-target penalty"
    assert (~live).any() and (r[~live] == 0).all(), "no steps after the end"
    assert not roll["roll/final_ended"].all() and roll["roll/final_ended"].sum() >= 4
    assert roll["roll/bt_mask"].sum() >= 6 and len(set(roll["roll/cand_len"].flatten().tolist())) > 3
    for mode in MODES:
        assert roll[f"roll/assert/{mode}"].any() or mode == "shortest", mode
    assert not roll["roll/assert/shortest"].any()                       # the shortest-path teacher always has an answer
    assert roll["roll/gt_len"].max() > 64 and roll["roll/gt_len"].min() == 1
    np.savez_compressed(OUT, **store)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(store)} arrays, {os.path.getsize(OUT)} bytes; {len(cases)} eval cases; V {VMAX}; "
          f"next-hop gap {gap:.3e}; spans {spans}")
    print("reward\n", np.round(r, 3), "\nenv\n", env, "\ndist\n", np.round(d, 2))
    for mode in MODES:
        print(mode, "\n", roll[f"roll/target/{mode}"])
    assert os.path.getsize(OUT) < 200 * 1024


if __name__ == "__main__":
    main()
