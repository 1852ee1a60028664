#!/usr/bin/env python3
"""Generate tests/golden/nav_tasks.npz by running the REFERENCE's own statements of its CVDN, REVERIE and R2R-Back agents and
environments around a rollout step and their evaluation on scripted rollouts, CPU.

Test infrastructure, like tools/gen_nav_golden.py, whose helpers, graphs (tests/golden/r2r_tiny, nav_tiny: unmodified) and R2R pieces
(`_teacher_action` over `_teacher_path_action`, the back-track block, `cal_dtw`, `cal_cls`) it shares:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_nav_tasks_golden.py

Nothing of the reference is restated: every piece is cut out of its FILE at generation time (located by its first and last statement)
and compiled --
  cvdn/agent.py           the init block (`last_dist = np.zeros(` ... `last_dist[i] = ob['distance']`) and the reward block
                          (`if train_rl:` ... `last_dist[:] = dist`);
  cvdn/env.py             the `min_dist` block of `_get_obs`, `_eval_item`, `eval_metrics`;
  r2r/agent_r2rback.py    the init block, the env-action and mid-stop block (`cpu_a_t = a_t.cpu().numpy()` ...
                          `traj[i]['midstop'] = obs[i]['viewpoint']`), the reward block through `first_ended[:] = ...`;
  r2r/env.py              `R2RBackBatch._eval_item`, `eval_metrics`;
  reverie/env.py          `ReverieNavRefBatch._eval_item`, `eval_metrics`.
What is scripted: the simulator (candidates = the neighbours, shuffled per step; the chosen candidate's viewpoint is where the episode
stands next) and each episode's list of moves, chosen so that every corner tests/test_nav_tasks.py asserts is taken (checked at the end).

Two rollouts of B = 6: `goals/` (T = 7, CVDN's blocks; the teacher asked in all three modes) and `back/` (T = 8, R2R-Back's blocks with
train_rl) plus `back_eval/` -- the same scripts with train_rl off, where the reference computes no reward and a missed mid-stop does
not end the episode.  Evaluation: `cvdn/`, `reverie/`, `backm/` with about 30 trajectories each.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import ref_shim                                            # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_nav_golden", os.path.join(ROOT, "tools", "gen_nav_golden.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

OUT = os.path.join(ROOT, "tests", "golden", "nav_tasks.npz")
SCANS, MODES, IGNORE = base.SCANS, base.MODES, base.IGNORE
B = 6
STOP, SKIP = "<stop>", "<ignored>"                                      # a move that is the STOP slot / the ignore id


# ------------------------------------------------------------------------------------------------ the reference's statements
def task_pieces(fn):
    """-> (compiled blocks, spans); the functions go into `fn` under task-prefixed names"""
    src = lambda *p: open(os.path.join(ref_shim.REF, "finetune_src", *p)).read().split("\n")
    blocks, spans = {}, {}

    def block(key, lines, path, first, last, start=0):
        text, spans[key] = base._block(lines, first, last, start)
        blocks[key] = compile(text, f"{path}:{spans[key][0]}-{spans[key][1]}", "exec")
        return text

    def define(prefix, lines, path, first, last, start):
        text, span = base._block(lines, first, last, start)
        ns = dict(fn)
        exec(compile(text, f"{path}:{span[0]}-{span[1]}", "exec"), ns)
        name = first.split("(")[0].replace("def ", "")
        fn[prefix + name], spans[prefix + name] = ns[name], span

    ca, ce = src("cvdn", "agent.py"), src("cvdn", "env.py")
    loop = next(i for i, ln in enumerate(ca) if ln.strip() == "for t in range(self.args.max_action_len):")
    block("goals_init", ca, "cvdn/agent.py", "last_dist = np.zeros(batch_size, np.float32)", "last_dist[i] = ob['distance']")
    text = block("goals_reward", ca, "cvdn/agent.py", "if train_rl:", "last_dist[:] = dist", loop)
    assert "dist[i] == 0." in text and "reward[i] = 0" in text and "ndtw" not in text, "cvdn/agent.py changed"
    at = next(i for i, ln in enumerate(ce) if ln.strip().startswith("def _get_obs("))
    block("goals_dist", ce, "cvdn/env.py", "if 'end_panos' in item:", "obs[-1]['distance'] = min_dist", at)
    define("cvdn:", ce, "cvdn/env.py", "def _eval_item(", "return scores", 0)
    define("cvdn:", ce, "cvdn/env.py", "def eval_metrics(", "return avg_metrics, metrics", 0)

    ba, env = src("r2r", "agent_r2rback.py"), src("r2r", "env.py")
    loop = next(i for i, ln in enumerate(ba) if ln.strip() == "for t in range(self.args.max_action_len):")
    block("back_init", ba, "agent_r2rback.py", "last_dist = np.zeros(batch_size, np.float32)", "last_ndtw[i] = cal_dtw(")
    block("back_action", ba, "agent_r2rback.py", "cpu_a_t = a_t.cpu().numpy()", "traj[i]['midstop'] = obs[i]['viewpoint']", loop)
    text = block("back_reward", ba, "agent_r2rback.py", "if train_rl:", "first_ended[:] = np.logical_or(first_ended", loop)
    assert "raise NameError" in text and "ob['distance'][1]" in text and "ended[i] = True" in text, "agent_r2rback.py changed"
    at = next(i for i, ln in enumerate(env) if ln.startswith("class R2RBackBatch"))
    define("back:", env, "env.py", "def _eval_item(", "return scores", at)
    define("back:", env, "env.py", "def eval_metrics(", "return avg_metrics, metrics", at)

    re_ = src("reverie", "env.py")
    at = next(i for i, ln in enumerate(re_) if ln.startswith("class ReverieNavRefBatch"))
    define("reverie:", re_, "reverie/env.py", "def _eval_item(", "return scores", at)
    define("reverie:", re_, "reverie/env.py", "def eval_metrics(", "return avg_metrics, metrics", at)
    return blocks, spans


# ------------------------------------------------------------------------------------------------ the scripted simulator
class Sim:
    """B episodes: where each stands, the candidates of the step (the neighbours, shuffled), the trajectory"""

    def __init__(self, w, scans, starts, seed):
        self.w, self.scans, self.here = w, list(scans), list(starts)
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.traj = [{"instr_id": f"r{i}", "path": [(v, 0.0, 0.0)], "midstop": None} for i, v in enumerate(starts)]
        self.shuffle()

    def shuffle(self):
        self.cands = []
        for scan, v in zip(self.scans, self.here):
            nb = sorted(self.w.graphs[scan][v])
            self.cands.append([{"viewpointId": nb[j]} for j in self.rng.permutation(len(nb))])

    def slots(self, moves):
        """a_t of the scripted moves (a viewpoint, STOP or SKIP) against this step's candidates"""
        a = np.zeros(len(moves), np.int64)
        for i, m in enumerate(moves):
            names = [c["viewpointId"] for c in self.cands[i]]
            a[i] = IGNORE if m == SKIP else len(names) if m == STOP else names.index(m)
        return a

    def act(self, cpu_a_t):
        """make_equiv_action + the simulator"""
        for i, a in enumerate(cpu_a_t):
            if a != -1:
                self.here[i] = self.cands[i][a]["viewpointId"]
                self.traj[i]["path"].append((self.here[i], 0.0, 0.0))
        self.shuffle()

    def cand_nodes(self, vmax):
        cn = np.full((len(self.here), vmax), -1, np.int32)
        for i, (scan, cs) in enumerate(zip(self.scans, self.cands)):
            cn[i, :len(cs)] = [self.w.ix[scan][c["viewpointId"]] for c in cs]
        return cn, np.array([len(c) + 1 for c in self.cands], np.int32)


def teacher_and_mask(w, fn, r2r_blocks, sim, gts, t, ended, visited, modes, vmax, rec):
    """what the agents ask before the policy step: `_teacher_action` in every mode of `modes`, and the back-track block"""
    me = types.SimpleNamespace(args=types.SimpleNamespace(ignoreid=IGNORE, no_cand_backtrack=True))
    teacher_action = types.MethodType(fn["_teacher_action"], me)
    n = len(gts)

    def observe(mode):
        obs = []
        for i in range(n):
            state = types.SimpleNamespace(scanId=sim.scans[i], location=types.SimpleNamespace(viewpointId=sim.here[i]))
            teacher = w._teacher_path_action(state, gts[i], t=t if mode == "path_step" else None, shortest_teacher=mode == "shortest")
            obs.append({"scan": sim.scans[i], "viewpoint": sim.here[i], "candidate": sim.cands[i], "teacher": teacher, "gt_path": gts[i]})
        return obs
    for mode in modes:
        obs = observe(mode)
        tgt, fired = np.zeros(n, np.int64), np.zeros(n, bool)
        for i in range(n):
            try:
                with ref_shim.cuda_is_identity():
                    tgt[i] = int(teacher_action([obs[i]], [ended[i]])[0])
            except AssertionError:
                tgt[i], fired[i] = IGNORE, True
        rec[f"target/{mode}"].append(tgt)
        rec[f"assert/{mode}"].append(fired)
    ns = {"np": np, "torch": torch, "self": me, "obs": observe("path_step"), "visited": visited, "ob_nav_types": torch.zeros(n, vmax)}
    with ref_shim.cuda_is_identity():
        exec(r2r_blocks["backtrack"], ns)
    rec["bt_mask"].append(ns["bt_masks"].numpy().astype(np.uint8))


def pack(w, scans, lists, dtype=np.int16):
    ln = np.array([len(p) for p in lists], np.int32)
    out = np.full((len(lists), max(1, int(ln.max(initial=1)))), -1, dtype)
    for i, (s, p) in enumerate(zip(scans, lists)):
        out[i, :ln[i]] = [w.ix[s][v] for v in p]
    return out, ln


def finish(w, sim, rec, eps_scan, starts, gts, prefix):
    out = {f"{prefix}/{k}": np.stack([np.asarray(x) for x in v]) for k, v in rec.items() if v}
    out[f"{prefix}/scan"] = np.array([[s for s, _ in SCANS].index(s_) for s_ in eps_scan], np.int32)
    out[f"{prefix}/start"] = np.array([w.ix[s][v] for s, v in zip(eps_scan, starts)], np.int32)
    out[f"{prefix}/gt"], out[f"{prefix}/gt_len"] = pack(w, eps_scan, gts)
    out[f"{prefix}/path"], out[f"{prefix}/path_len"] = pack(w, eps_scan, [[x[0] for x in tr["path"]] for tr in sim.traj])
    return out


# ------------------------------------------------------------------------------------------------ goal sets (CVDN's blocks)
def goal_episodes(w):
    """(scan, start, ground-truth path for the teacher, goal list or None, moves)"""
    C, order = w.shortest_paths["scanC"], w.order["scanC"]
    d = lambda a, b_: w.dist("scanC", a, b_)
    # 65 entries: 64 over the 13 nodes farthest from c01, then c01 alone at index 64 -- the one a walk of four moves ends on
    far = sorted(order, key=lambda v: -d("c01", v))[:13]
    many = [far[k % 13] for k in range(64)] + ["c01"]
    walk = next(C[v]["c01"] for v in order if len(C[v]["c01"]) == 5)
    assert all(min(d(x, v) for v in far) > d(x, "c01") for x in walk[1:])
    return [
        ("scanA", "a00", ["a00", "a02", "a03"], ["a03"], ["a02", "a03", STOP]),                        # a stop on the goal, then rows after the end
        ("scanA", "a00", ["a00", "a02"], ["a02", "a05", "a02"], ["a01", STOP]),                         # a duplicate; a stop 0.6 m from a goal: -2
        ("scanC", walk[0], walk, many, walk[1:] + [STOP]),                                              # 65 goals: the last one decides
        ("scanC", "c07", ["c07"], None, [sorted(w.graphs["scanC"]["c07"])[0], "c07", STOP]),            # no goals: distance 0 throughout
        ("scanB", "b00", ["b00", "b02", "b03"], ["b01", "b03", "b04"], ["b02", "b04", "b03", "b04", "b01", "b00", "b01"]),   # never stops
        ("scanA", "a04", ["a04", "a03", "a02"], ["a02", "a01"], ["a03", "a02", "a01", "a00", SKIP]),    # goal to goal: distance unchanged at 0
    ]


def goal_rollout(w, fn, r2r_blocks, blocks, vmax, T=7):
    eps = goal_episodes(w)
    scans, starts, gts, goal_sets = [e[0] for e in eps], [e[1] for e in eps], [e[2] for e in eps], [e[3] for e in eps]
    sim = Sim(w, scans, starts, seed=23)
    me = types.SimpleNamespace(shortest_distances=w.shortest_distances)

    def observe():
        obs = []
        for i in range(B):
            item = {} if goal_sets[i] is None else {"end_panos": goal_sets[i]}
            obs.append({"viewpoint": sim.here[i]})
            exec(blocks["goals_dist"], {"np": np, "self": me, "item": item, "scan": scans[i], "viewpoint": sim.here[i], "obs": obs})
        return obs
    ended, visited = np.array([False] * B), [set() for _ in range(B)]
    ns = {"np": np, "batch_size": B, "obs": observe(), "train_rl": True, "ended": ended}
    exec(blocks["goals_init"], ns)
    keys = ("cand", "cand_len", "a_t", "env_action", "ended", "bt_mask", "dist", "reward", "mask", "cur")
    rec = {k: [] for k in keys + tuple(f"{p}/{m}" for p in ("target", "assert") for m in MODES)}
    init = ns["last_dist"].copy()
    for t in range(T):
        teacher_and_mask(w, fn, r2r_blocks, sim, gts, t, ended, visited, MODES, vmax, rec)
        rec["cur"].append([w.ix[scans[i]][sim.here[i]] for i in range(B)])
        a_t = sim.slots([STOP if ended[i] or t >= len(eps[i][4]) else eps[i][4][t] for i in range(B)])
        cl = np.array([len(c) + 1 for c in sim.cands])
        cpu_a_t = np.where((a_t == cl - 1) | (a_t == IGNORE) | ended, -1, a_t)                          # (cvdn/agent.py:138-141)
        cn, cand_len = sim.cand_nodes(vmax)
        for k, v in (("cand", cn), ("cand_len", cand_len), ("a_t", a_t), ("env_action", cpu_a_t.astype(np.int32)), ("ended", ended.copy())):
            rec[k].append(v)
        sim.act(cpu_a_t)
        ns.update(obs=observe(), cpu_a_t=cpu_a_t, rewards=[], masks=[])
        exec(blocks["goals_reward"], ns)
        rec["dist"].append(ns["dist"].copy())
        rec["reward"].append(ns["rewards"][0].copy())
        rec["mask"].append(ns["masks"][0].copy())
        ended[:] = np.logical_or(ended, cpu_a_t == -1)                                                  # (:205)
    out = finish(w, sim, rec, scans, starts, gts, "goals")
    out["goals/init_last_dist"], out["goals/final_ended"] = init, ended.copy()
    out["goals/goals"], out["goals/goal_len"] = pack(w, scans, [g or [] for g in goal_sets])
    return out


# ------------------------------------------------------------------------------------------------ return trips (R2R-Back's blocks)
def back_episodes(w):
    """(scan, ground-truth path with its mid-stop twice in a row, mid-stop, moves)"""
    C, order, G = w.shortest_paths["scanC"], w.order["scanC"], w.graphs["scanC"]
    d = lambda a, b_: w.dist("scanC", a, b_)
    out_leg = next(C[v]["c35"] for v in order if len(C[v]["c35"]) == 3)
    home = C["c35"]["c10"]
    long_gt = (C["c00"]["c29"] + C["c29"]["c50"][1:])
    long_gt = long_gt + [long_gt[-1]]
    for via in ("c00", "c60", "c20", "c41", "c05", "c33", "c12", "c66"):
        long_gt = long_gt + C[long_gt[-1]][via][1:]
    assert len(long_gt) >= 66, len(long_gt)
    mid_at = long_gt.index("c50")
    long_gt = long_gt[:66]
    assert mid_at > 8 and long_gt[mid_at + 1] == "c50"
    # scanC: a mid-stop with a neighbour less than 3 m away (a hit that is not exact), the way home leaving through another node
    mid5 = out_leg[-1]
    near5 = min((v for v in G[mid5] if v not in out_leg and v != home[1]), key=lambda v: d(v, mid5))
    assert 0 < d(near5, mid5) < 3.0 and d(home[1], home[-1]) >= 3.0, (d(near5, mid5), d(home[1], home[-1]))
    return [
        ("scanA", ["a00", "a02", "a03", "a03", "a02", "a00"], "a03", ["a02", "a03", STOP, "a02", "a00", STOP]),          # both stops hit
        ("scanB", ["b00", "b02", "b02", "b00"], "b02", ["b01", STOP, "b00", STOP]),                                     # the mid-stop missed
        ("scanC", long_gt, "c50", long_gt[1:9]),                                                                       # never stops
        ("scanA", ["a00", "a01", "a04", "a04", "a05", "a06"], "a04", ["a01", "a04", STOP, "a05", "a06", STOP]),          # closer to the END after the stop
        ("scanB", ["b00", "b02", "b03", "b03", "b04", "b01"], "b03", ["b02", "b03", SKIP, "b04", STOP]),                 # an ignored action as the stop; the end missed
        ("scanC", out_leg + [mid5] + home[1:], mid5, out_leg[1:] + [near5, STOP, mid5, home[1], STOP]),                 # a near hit, then a wrong end
    ]


def back_rollout(w, fn, r2r_blocks, blocks, vmax, train_rl, T=8):
    eps = back_episodes(w)
    scans, gts, mids = [e[0] for e in eps], [e[1] for e in eps], [e[2] for e in eps]
    starts = [g[0] for g in gts]
    sim = Sim(w, scans, starts, seed=31)
    me = types.SimpleNamespace(args=types.SimpleNamespace(ignoreid=IGNORE), env=types.SimpleNamespace(shortest_distances=w.shortest_distances))

    def observe():
        return [{"scan": scans[i], "viewpoint": sim.here[i], "gt_path": gts[i],
                 "distance": (w.dist(scans[i], sim.here[i], mids[i]), w.dist(scans[i], sim.here[i], gts[i][-1]))} for i in range(B)]   # (env.py:435-438)
    ended, first_ended, visited = np.array([False] * B), np.array([False] * B), [set() for _ in range(B)]
    traj, step_of = sim.traj, [0] * B                                    # (step_of: how far each script has come)
    ns = {"np": np, "self": me, "cal_dtw": fn["cal_dtw"], "batch_size": B, "obs": observe(), "traj": traj, "train_rl": train_rl,
          "ended": ended, "first_ended": first_ended}
    exec(blocks["back_init"], ns)
    keys = ("cand", "cand_len", "a_t", "env_action", "ended", "first_ended", "bt_mask", "dist", "last_dist", "ndtw", "reward", "mask", "cur",
            "ended_after", "first_ended_after", "midstop_at", "target/path_step", "assert/path_step")
    rec = {k: [] for k in keys}
    init = {"last_dist": ns["last_dist"].copy(), "last_ndtw": ns["last_ndtw"].copy()}
    for t in range(T):
        teacher_and_mask(w, fn, r2r_blocks, sim, gts, t, ended, visited, ("path_step",), vmax, rec)
        rec["cur"].append([w.ix[scans[i]][sim.here[i]] for i in range(B)])
        moves = []
        for i in range(B):
            moves.append(STOP if ended[i] or step_of[i] >= len(eps[i][3]) else eps[i][3][step_of[i]])
            step_of[i] += 0 if ended[i] else 1
        a_t = sim.slots(moves)
        cn, cand_len = sim.cand_nodes(vmax)
        ns.update(a_t=torch.from_numpy(a_t.copy()), ob_cand_lens=cand_len.tolist(), obs=observe())
        exec(blocks["back_action"], ns)
        cpu_a_t = ns["cpu_a_t"]
        for k, v in (("cand", cn), ("cand_len", cand_len), ("a_t", a_t), ("env_action", cpu_a_t.astype(np.int32)), ("ended", ended.copy()),
                     ("first_ended", first_ended.copy())):
            rec[k].append(v)
        sim.act(cpu_a_t)
        ns.update(obs=observe(), rewards=[], masks=[])
        exec(blocks["back_reward"], ns)
        if train_rl:
            rec["dist"].append(ns["dist"].copy())
            rec["last_dist"].append(ns["last_dist"].copy())
            rec["ndtw"].append(ns["ndtw_score"].copy())
            rec["reward"].append(ns["rewards"][0].copy())
            rec["mask"].append(ns["masks"][0].copy())
        rec["ended_after"].append(ended.copy())
        rec["first_ended_after"].append(first_ended.copy())
        rec["midstop_at"].append([-1 if tr["midstop"] is None else w.ix[s][tr["midstop"]] for s, tr in zip(scans, traj)])
    prefix = "back" if train_rl else "back_eval"
    out = finish(w, sim, rec, scans, starts, gts, prefix)
    out[f"{prefix}/midstop"] = np.array([w.ix[s][m] for s, m in zip(scans, mids)], np.int32)
    if train_rl:
        out["back/init_last_dist"], out["back/init_last_ndtw"] = init["last_dist"], init["last_ndtw"]
    return out


# ------------------------------------------------------------------------------------------------ the scored trajectories
def eval_all(w, fn):
    rng = np.random.Generator(np.random.PCG64(37))
    order = w.order

    def walk(scan, start, n, revisit=0.3):
        p = [start]
        while len(p) < n:
            nb = sorted(w.graphs[scan][p[-1]])
            fresh = [v for v in nb if v not in p]
            p.append(str(rng.choice(fresh if fresh and rng.random() > revisit else nb)))
        return p
    pick = lambda scan, k: [str(v) for v in rng.choice(order[scan], size=k, replace=False)]
    out = {}
    scan_id = lambda ss: np.array([[s for s, _ in SCANS].index(s) for s in ss], np.int32)

    # ---- CVDN: (scan, path, end_panos)
    cases = [("scanA", ["a00", "a02", "a03"], ["a03"]), ("scanA", ["a00", "a02", "a03"], ["a05"]),                     # at the goal; gp > 0 without success
             ("scanA", ["a02", "a03", "a04"], ["a02", "a06"]),                                                       # starts inside the set: gt_lengths 0, gp < 0
             ("scanA", ["a00"], ["a00"]), ("scanB", ["b00", "b02", "b00", "b01"], ["b03", "b02", "b03"]),              # a duplicate; oracle success only
             ("scanB", ["b00", "b01"], ["b03"])]
    for pn in (1, 2, 64, 65, 130):
        for en in (1, 3, 65):
            start = pick("scanC", 1)[0]
            cases.append(("scanC", walk("scanC", start, pn), pick("scanC", en)))
    for _ in range(9):
        scan = ("scanA", "scanB", "scanC")[int(rng.integers(3))]
        p = walk(scan, pick(scan, 1)[0], int(rng.integers(1, 9)))
        cases.append((scan, p, [p[-1]] + pick(scan, 2) if rng.random() < 0.4 else pick(scan, int(rng.integers(1, 4)))))
    me = types.SimpleNamespace(shortest_distances=w.shortest_distances, gt_trajs={f"i{k}": (s, e) for k, (s, _, e) in enumerate(cases)})
    me._eval_item = types.MethodType(fn["cvdn:_eval_item"], me)
    preds = [{"instr_id": f"i{k}", "trajectory": [(v, 0.0, 0.0) for v in p]} for k, (_, p, _) in enumerate(cases)]
    avg, metrics = fn["cvdn:eval_metrics"](me, preds)
    cols = ("trajectory_steps", "trajectory_lengths", "success", "oracle_success", "spl", "gp")
    assert list(metrics) == list(cols) + ["instr_id"], list(metrics)
    ss = [c[0] for c in cases]
    out["cvdn/scan"] = scan_id(ss)
    out["cvdn/path"], out["cvdn/path_len"] = pack(w, ss, [c[1] for c in cases])
    out["cvdn/goals"], out["cvdn/goal_len"] = pack(w, ss, [c[2] for c in cases])
    out["cvdn/metrics"] = np.stack([np.asarray(metrics[c], np.float64) for c in cols], 1)
    out["cvdn/avg_keys"], out["cvdn/avg"] = np.array(list(avg)), np.array([avg[k] for k in avg], np.float64)
    n_cvdn = len(cases)

    # ---- REVERIE: (scan, path, gt_path, the viewpoints the object is visible from, predicted object, the object)
    cases = [("scanA", ["a00", "a02", "a03"], ["a00", "a02", "a03"], ["a03", "a04"], 7, 7),
             ("scanA", ["a00", "a01", "a02", "a03"], ["a00", "a02", "a03"], ["a03", "a03"], 7, 8),                     # a detour; the wrong object
             ("scanA", ["a00", "a02", "a03", "a04"], ["a00", "a02", "a03"], ["a03"], 2, 2),                           # walked past: oracle only, rgs without success
             ("scanB", ["b00"], ["b00", "b02"], ["b02"], None, 3), ("scanB", ["b00", "b02"], ["b00"], ["b02"], 3, 3)]
    for pn in (1, 2, 64, 65, 130):
        for en in (1, 3, 65):
            start = pick("scanC", 1)[0]
            goals = pick("scanC", en)
            gt = w.shortest_paths["scanC"][start][goals[0]] if rng.random() < 0.6 else walk("scanC", start, int(rng.integers(2, 70)), revisit=0.1)
            cases.append(("scanC", walk("scanC", start, pn), gt, goals, int(rng.integers(3)), int(rng.integers(3))))
    for _ in range(9):
        scan = ("scanA", "scanB", "scanC")[int(rng.integers(3))]
        gt = walk(scan, pick(scan, 1)[0], int(rng.integers(2, 7)), revisit=0.0)
        p = gt if rng.random() < 0.4 else walk(scan, gt[0], int(rng.integers(1, 9)))
        cases.append((scan, p, gt, [gt[-1]] + pick(scan, int(rng.integers(0, 3))), int(rng.integers(2)), int(rng.integers(2))))
    me = types.SimpleNamespace(shortest_distances=w.shortest_distances,
                               obj2viewpoint={f"{s}_{k}": e for k, (s, _, _, e, _, _) in enumerate(cases)},
                               gt_trajs={f"i{k}": (s, g, k) for k, (s, _, g, _, _, _) in enumerate(cases)})
    # (object ids: case k's object is named k, so that its key in obj2viewpoint is its own; the prediction is k when the case says "same")
    me._eval_item = types.MethodType(fn["reverie:_eval_item"], me)
    preds = [{"instr_id": f"i{k}", "trajectory": [(v, 0.0, 0.0) for v in p], "predObjId": (k if po == go else None if po is None else -1 - po)}
             for k, (_, p, _, _, po, go) in enumerate(cases)]
    avg, metrics = fn["reverie:eval_metrics"](me, preds)
    cols = ("trajectory_steps", "trajectory_lengths", "success", "oracle_success", "spl", "rgs", "rgspl")
    assert list(metrics) == list(cols) + ["instr_id"], list(metrics)
    ss = [c[0] for c in cases]
    out["reverie/scan"] = scan_id(ss)
    out["reverie/path"], out["reverie/path_len"] = pack(w, ss, [c[1] for c in cases])
    out["reverie/gt"], out["reverie/gt_len"] = pack(w, ss, [c[2] for c in cases])
    out["reverie/goals"], out["reverie/goal_len"] = pack(w, ss, [c[3] for c in cases])
    out["reverie/pred_obj"] = np.array([-99 if p["predObjId"] is None else p["predObjId"] for p in preds], np.int32)     # (-99: None)
    out["reverie/metrics"] = np.stack([np.asarray(metrics[c], np.float64) for c in cols], 1)
    out["reverie/avg_keys"], out["reverie/avg"] = np.array(list(avg)), np.array([avg[k] for k in avg], np.float64)
    n_rev = len(cases)

    # ---- R2R-Back: (scan, path, gt_path, midstop or None, gt_midstop)
    cases = [("scanA", ["a00", "a02", "a03", "a02", "a00"], ["a00", "a02", "a03", "a03", "a02", "a00"], "a03", "a03"),   # both conditions hold
             ("scanA", ["a00", "a02", "a03", "a02", "a01"], ["a00", "a02", "a03", "a03", "a02", "a00"], "a03", "a03"),   # the end 5.9 m off
             ("scanA", ["a00", "a02", "a03", "a02", "a00"], ["a00", "a02", "a03", "a03", "a02", "a00"], "a02", "a03"),   # the mid-stop 8.9 m off
             ("scanA", ["a00", "a02", "a03", "a02", "a00"], ["a00", "a02", "a03", "a03", "a02", "a00"], None, "a03"),    # no mid-stop
             ("scanA", ["a00", "a01", "a02", "a01"], ["a00", "a02", "a02", "a01", "a02"], "a01", "a02"),                 # both within 0.6 m
             ("scanC", ["c11"], ["c11"], "c11", "c11")]                                                                # the NaN corner: CLS = 0 / 0
    for pn in (1, 2, 64, 65, 130):
        for gn in (2, 65, 130):
            start = pick("scanC", 1)[0]
            p, gt = walk("scanC", start, pn), walk("scanC", start, gn, revisit=0.1)
            gmid = gt[len(gt) // 2]
            mid = None if rng.random() < 0.2 else gmid if rng.random() < 0.5 else p[int(rng.integers(len(p)))]
            cases.append(("scanC", p, gt, mid, gmid))
    for _ in range(9):
        scan = ("scanA", "scanB", "scanC")[int(rng.integers(3))]
        gt = walk(scan, pick(scan, 1)[0], int(rng.integers(3, 9)), revisit=0.0)
        p = gt if rng.random() < 0.5 else walk(scan, gt[0], int(rng.integers(1, 11)))
        cases.append((scan, p, gt, (p[len(p) // 2] if rng.random() < 0.8 else None), gt[len(gt) // 2]))
    me = types.SimpleNamespace(shortest_distances=w.shortest_distances, gt_trajs={f"i{k}": (s, g) for k, (s, _, g, _, _) in enumerate(cases)},
                               gt_midstops={f"i{k}": c[4] for k, c in enumerate(cases)})
    me._eval_item = types.MethodType(fn["back:_eval_item"], me)
    preds = [{"instr_id": f"i{k}", "trajectory": [(v, 0.0, 0.0) for v in p], "midstop": m} for k, (_, p, _, m, _) in enumerate(cases)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # (the NaN corner divides 0 by 0)
        avg, metrics = fn["back:eval_metrics"](me, preds)
    cols = ("nav_error", "trajectory_steps", "trajectory_lengths", "success", "spl", "DTW", "nDTW", "SDTW", "CLS")
    assert list(metrics) == list(cols) + ["instr_id"], list(metrics)
    ss = [c[0] for c in cases]
    out["backm/scan"] = scan_id(ss)
    out["backm/path"], out["backm/path_len"] = pack(w, ss, [c[1] for c in cases])
    out["backm/gt"], out["backm/gt_len"] = pack(w, ss, [c[2] for c in cases])
    out["backm/midstop"] = np.array([-1 if c[3] is None else w.ix[c[0]][c[3]] for c in cases], np.int32)
    out["backm/gt_midstop"] = np.array([w.ix[c[0]][c[4]] for c in cases], np.int32)
    out["backm/metrics"] = np.stack([np.asarray(metrics[c], np.float64) for c in cols], 1)
    out["backm/avg_keys"], out["backm/avg"] = np.array(list(avg)), np.array([avg[k] for k in avg], np.float64)
    return out, (n_cvdn, n_rev, len(cases))


def main():
    fn, r2r_blocks, r2r_spans = base.reference_pieces()
    blocks, spans = task_pieces(fn)
    w = base.World(fn)
    vmax = max(max(dict(G.degree).values()) for G in w.graphs.values()) + 1
    store = {"meta/ignoreid": np.array(IGNORE), "meta/scans": np.array([s for s, _ in SCANS])}
    for k, v in spans.items():
        store["meta/span/" + k] = np.asarray(v)
    gr = goal_rollout(w, fn, r2r_blocks, blocks, vmax)
    bk = back_rollout(w, fn, r2r_blocks, blocks, vmax, train_rl=True)
    be = back_rollout(w, fn, r2r_blocks, blocks, vmax, train_rl=False)
    ev, counts = eval_all(w, fn)
    for part in (gr, bk, be, ev):
        store.update(part)
    check_corners(store)
    np.savez_compressed(OUT, **store)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(store)} arrays, {os.path.getsize(OUT)} bytes; eval cases {counts}; V {vmax}; spans {spans}")
    print("goals reward\n", gr["goals/reward"], "\nenv\n", gr["goals/env_action"], "\ndist\n", np.round(gr["goals/dist"], 2))
    print("back reward\n", np.round(bk["back/reward"], 3), "\nenv\n", bk["back/env_action"], "\ndist\n", np.round(bk["back/dist"], 2),
          "\nended after\n", bk["back/ended_after"].astype(int), "\nwithout train_rl\n", be["back_eval/ended_after"].astype(int))
    assert os.path.getsize(OUT) < 200 * 1024


def check_corners(store):
    """the corners the tests assert are really there (tests/test_nav_tasks.py holds the same list)"""
    g = lambda k: store["goals/" + k]
    r, m, env, d = g("reward"), g("mask"), g("env_action"), g("dist")
    last = np.concatenate([g("init_last_dist")[None], d[:-1]])
    live = m == 1
    assert sorted(set(g("goal_len").tolist())) == [0, 1, 2, 3, 65] or sorted(set(g("goal_len").tolist())) == [0, 1, 3, 65], g("goal_len")
    assert (live & (env == -1) & (d == 0) & (r == 2)).any() and (live & (env == -1) & (d > 0) & (d < 3) & (r == -2)).any()
    assert (live & (env >= 0) & (d < last) & (r == 1)).any() and (live & (env >= 0) & (d > last) & (r == -1)).any()
    assert (live & (env >= 0) & (d == last) & (r == 0)).any()
    assert (~live).any() and (r[~live] == 0).all()
    b = lambda k: store["back/" + k]
    assert (b("midstop_at")[-1] == -1).any() and (b("a_t") == IGNORE).any()
    assert not b("ended_after")[-1].all() and not np.array_equal(b("ended_after"), store["back_eval/ended_after"])


if __name__ == "__main__":
    main()
