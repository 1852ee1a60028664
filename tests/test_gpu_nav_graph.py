"""-m gpu: the navigation graphs on the device (csrc/nav.hip -> ops.nav_observe / nav_advance / nav_eval -> agent.NavGraphs / NavEpisodes ->
RolloutRecorder.step(nav=...)) against the reference's own statements (tests/golden/nav_reward.npz) and the numpy restatement
(tests/_nav_ref.py).

Bounds (the CPU test's): integers, masks and the fp32 distance exact; ndtw 2.4e-7 (two fp32 ulps at 1); reward 1e-6 (|reward| <= 4, one
rounding of an fp64 result); metrics 1e-12 relative with NaNs in the same places."""
import json
import os
import types

import numpy as np
import pytest
import torch

from _nav_ref import (COLS, CONNECTIVITY, MODES, TOL_NDTW, TOL_REWARD, EpisodesRef, close_metrics, eval_ref, golden_tables, host_tables,
                      neighbours, random_walk)
from _util import load_npz
from test_nav_graph import golden_rollout

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


def graphs():
    from vln_hamt_amd.agent import NavGraphs
    if "graphs" not in _CACHE:
        _CACHE["graphs"] = NavGraphs(CONNECTIVITY, device=DEV)
    return _CACHE["graphs"]


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _golden_episodes(store, T, max_gt=128, poison=False):
    from vln_hamt_amd.agent import NavEpisodes
    g, G = (lambda k: store["roll/" + k]), graphs()
    scans = [G.scans[s] for s in g("scan")]
    nav = NavEpisodes(G, T, len(scans), max_gt=max_gt)
    if poison:
        nav.arena.fill_(0xFF)
    gts = [[G.viewpoint(sc, v) for v in gt[:n]] for sc, gt, n in zip(scans, g("gt"), g("gt_len"))]
    return nav.reset(scans, [G.viewpoint(sc, v) for sc, v in zip(scans, g("start"))], gts)


def _logits(store, seed=3):
    g = lambda k: store["roll/" + k]
    T, B, V = g("cand").shape
    x = np.random.Generator(np.random.PCG64(seed)).standard_normal((T, B, V)).astype(np.float32)
    x[np.arange(V)[None, None] >= g("cand_len")[..., None]] = -np.inf
    return x


def _run_golden(store, mode, poison=False, check=True):
    """the golden's scripted rollout through RolloutRecorder.step(nav=...); returns every result as host arrays"""
    from vln_hamt_amd.agent import RolloutRecorder
    g = lambda k: store["roll/" + k]
    T, B, V = g("cand").shape
    rec = RolloutRecorder(T, B, DEV, ignoreid=int(store["meta/ignoreid"]))
    if poison:
        for buf in (rec.ml, rec.logp, rec.ent, rec.mask, rec.reward):
            buf.fill_(float("nan"))
    rec.reset(B)
    nav = _golden_episodes(store, T, poison=poison)
    logits = d(_logits(store)).requires_grad_(True)
    res = {"init_last_dist": nav.last_dist.cpu().numpy(), "init_last_ndtw": nav.last_ndtw.cpu().numpy()}

    def step(t, cand, cand_len, ended, a_t):
        assert np.array_equal(rec.ended.cpu().numpy().astype(bool), ended) and np.array_equal(nav.cur.cpu().numpy(), g("cur")[t])
        _, env, _ = rec.step(t, logits[t], cand_lens=d(cand_len), feedback="sample", forced_action=d(a_t), nav=nav, cand_nodes=d(cand),
                             teacher_mode=mode)
        assert np.array_equal(env, g("env_action")[t]), (t, env)
        out = (rec.target.cpu().numpy(), rec.bt_mask.cpu().numpy(), rec.reward[t].cpu().numpy(), nav.last_dist.cpu().numpy(), nav.last_ndtw.cpu().numpy())
        for k, v in zip(("target", "bt_mask", "reward", "dist", "ndtw"), out):
            res[f"{k}{t}"] = v
        return out
    if check:
        golden_rollout(store, mode, step)
    else:
        for t in range(T):
            step(t, g("cand")[t], g("cand_len")[t], g("ended")[t], g("a_t")[t])
    res.update(path=nav.path.cpu().numpy(), path_len=nav.path_len.cpu().numpy(), anomalies=nav.anomalies.cpu().numpy(), cur=nav.cur.cpu().numpy(),
               dtw_row=nav.dtw_row.cpu().numpy(), mask=rec.mask.cpu().numpy())
    return res, rec, nav, logits


@pytest.mark.parametrize("mode", MODES)
def test_golden_rollout_through_the_recorder(mode):
    """The golden's B = 6, T = 7 rollout (three scans in one batch, a 66-node ground truth) through NavEpisodes and
    RolloutRecorder.step(nav=...): target, back-track mask, distance, nDTW and reward of every step against the reference's own
    statements; the walked paths; the anomaly counter = the places the reference's assert fired."""
    store = load_npz("nav_reward.npz")
    g = lambda k: store["roll/" + k]
    res, rec, nav, _ = _run_golden(store, mode)
    assert np.array_equal(res["init_last_dist"], g("init_last_dist")) and float(np.abs(res["init_last_ndtw"] - g("init_last_ndtw")).max()) <= TOL_NDTW
    assert res["anomalies"].tolist() == [int(g(f"assert/{mode}").sum()), 0]
    assert np.array_equal(res["path_len"], g("path_len")) and np.array_equal(res["mask"], g("mask"))
    for b, n in enumerate(g("path_len")):
        assert np.array_equal(res["path"][b, :n], g("path")[b, :n])


def test_poisoned_state_changes_nothing(monkeypatch):
    """Every state buffer of NavEpisodes pre-filled with 0xFF, the recorder's arrays with NaN, before `reset`, and every torch.empty of
    the ops poisoned: bit-identical targets, masks, rewards and state."""
    from test_gpu_policy_step import _poisoned_empty
    store = load_npz("nav_reward.npz")
    want = _run_golden(store, "path_index", check=False)[0]
    monkeypatch.setattr(torch, "empty", _poisoned_empty(torch.empty))
    got = _run_golden(store, "path_index", poison=True, check=False)[0]
    monkeypatch.undo()
    assert set(want) == set(got)
    for k, w in want.items():
        assert np.array_equal(w, got[k]) and not np.isnan(got[k]).any(), k


def _four_node_dir(tmp_path):
    """goal g at the origin, p and q both exactly 1 m from it and linked to each other, r behind q: the move p -> q leaves the distance unchanged"""
    xyz = {"g": (0, 0, 0), "p": (1, 0, 0), "q": (0, 1, 0), "r": (0, 2, 0)}
    links = {("g", "p"), ("g", "q"), ("p", "q"), ("q", "r")}
    names = list(xyz)
    nodes = []
    for a in names:
        pose = [0.0] * 16
        pose[3], pose[7], pose[11] = (float(v) for v in xyz[a])
        nodes.append({"image_id": a, "pose": pose, "included": True, "unobstructed": [(a, b) in links or (b, a) in links for b in names]})
    (tmp_path / "scanD_connectivity.json").write_text(json.dumps(nodes))
    (tmp_path / "scans.txt").write_text("scanD\n")
    return str(tmp_path)


def test_zero_move_anomaly(tmp_path):
    """A move between two nodes equidistant from the goal (the reference raises NameError): reward = ndtw - last_ndtw, anomalies[1] = 1"""
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import NavEpisodes, NavGraphs
    G = NavGraphs([CONNECTIVITY[0], _four_node_dir(tmp_path)], device=DEV)
    tables = host_tables(G)
    s = G.scans.index("scanD")
    ix = lambda v: G.node_id("scanD", v)
    nav = NavEpisodes(G, 3, 2, max_gt=4).reset(["scanD", "scanD"], ["p", "r"], [["p", "g"], ["r", "q", "g"]])
    ref = EpisodesRef(tables, [s, s], [ix("p"), ix("r")], [[ix("p"), ix("g")], [ix("r"), ix("q"), ix("g")]], [2, 3])
    cand = np.array([[ix("g"), ix("q"), -1], [ix("q"), -1, -1]], np.int32)
    env, mask = np.array([1, 0], np.int32), np.ones(2, np.float32)
    reward = ops.nav_advance(nav, d(cand), d(env), d(mask), torch.full((2,), float("nan"), device=DEV)).cpu().numpy()
    want, dist, ndtw = ref.advance(cand, env, mask)
    assert nav.anomalies.cpu().tolist() == [0, 1] == ref.anomalies
    assert np.array_equal(nav.last_dist.cpu().numpy(), dist) and dist[0] == 1.0
    assert float(np.abs(reward - want).max()) <= TOL_REWARD and abs(float(reward[0])) <= TOL_REWARD      # (the DTW of [p, q] against [p, g] is that of [p])
    assert float(np.abs(nav.last_ndtw.cpu().numpy() - ndtw).max()) <= TOL_NDTW and want[1] > 0
    assert nav.cur.cpu().tolist() == [ix("q"), ix("q")]


@pytest.mark.parametrize("V", [9, 70])
def test_random_rollouts_vs_restatement(V):
    """B = 37 episodes (not a multiple of the workgroup's four waves) over the three scans, ground truths of 1, 2, 64, 65 and 130
    nodes, T = 12 random steps (stops, moves, revisits; the teacher mode changes with the step), candidates padded to V: every step's
    target, mask, distance, nDTW and reward, and the final state, against the restatement."""
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import NavEpisodes
    G, B, T = graphs(), 37, 12
    rng = np.random.Generator(np.random.PCG64(100 + V))
    nbrs = [neighbours(G, s) for s in G.scans]
    scan = [b % 3 for b in range(B)]
    gts = [random_walk(rng, nbrs[scan[b]], rng.integers(len(nbrs[scan[b]])), (1, 2, 64, 65, 130)[b % 5], revisit=0.2) for b in range(B)]
    start = [gt[0] if b % 4 else int(rng.integers(len(nbrs[scan[b]]))) for b, gt in enumerate(gts)]
    name = lambda b, v: G.viewpoint(G.scans[scan[b]], v)
    nav = NavEpisodes(G, T, B, max_gt=130).reset([G.scans[s] for s in scan], [name(b, v) for b, v in enumerate(start)],
                                                 [[name(b, v) for v in gt] for b, gt in enumerate(gts)])
    glen = np.array([len(g_) for g_ in gts], np.int32)
    gpad = np.full((B, 130), -1, np.int32)
    for b, g_ in enumerate(gts):
        gpad[b, :len(g_)] = g_
    ref = EpisodesRef(host_tables(G), scan, start, gpad, glen)
    assert np.array_equal(nav.last_dist.cpu().numpy(), ref.last_dist) and float(np.abs(nav.last_ndtw.cpu().numpy() - ref.last_ndtw).max()) <= TOL_NDTW
    ended = np.zeros(B, bool)
    worst_n = worst_r = 0.0
    for t in range(T):
        cand, cl = np.full((B, V), -1, np.int32), np.zeros(B, np.int32)
        env = np.full(B, -1, np.int32)
        for b in range(B):
            nb = [nbrs[scan[b]][ref.cur[b]][j] for j in rng.permutation(len(nbrs[scan[b]][ref.cur[b]]))]
            cand[b, :len(nb)], cl[b] = nb, len(nb) + 1
            if not ended[b] and rng.random() > 0.12:
                env[b] = int(rng.integers(len(nb)))
        mode = MODES[t % 3]
        target, bt = ops.nav_observe(nav, t, d(cand), d(cl), d(ended.astype(np.uint8)), mode=mode)
        reward = ops.nav_advance(nav, d(cand), d(env), d((~ended).astype(np.float32)), torch.full((B,), float("nan"), device=DEV)).cpu().numpy()
        w_target, w_bt = ref.observe(t, cand, cl, ended, mode)
        w_reward, w_dist, w_ndtw = ref.advance(cand, env, (~ended).astype(np.float32))
        assert np.array_equal(target.cpu().numpy(), w_target), (t, mode)
        assert np.array_equal(bt.cpu().numpy(), w_bt), t
        assert np.array_equal(nav.last_dist.cpu().numpy(), w_dist) and np.array_equal(nav.cur.cpu().numpy(), ref.cur), t
        worst_n = max(worst_n, float(np.abs(nav.last_ndtw.cpu().numpy().astype(np.float64) - w_ndtw).max()))
        worst_r = max(worst_r, float(np.abs(reward.astype(np.float64) - w_reward).max()))
        ended |= env == -1
    print(f"[random rollouts V {V}] max|d ndtw| {worst_n:.3e}  max|d reward| {worst_r:.3e}  anomalies {ref.anomalies}")
    assert worst_n <= TOL_NDTW and worst_r <= TOL_REWARD
    assert nav.anomalies.cpu().tolist() == ref.anomalies and ref.anomalies[0] > 0
    path, n = nav.path.cpu().numpy(), nav.path_len.cpu().numpy()
    row = nav.dtw_row.cpu().numpy()
    for b in range(B):
        assert path[b, :n[b]].tolist() == ref.path[b]
        assert np.isinf(row[b, 0]) and np.abs(row[b, 1:glen[b] + 1] - ref.row[b][1:]).max() <= 1e-12 * ref.row[b][1:].max()


def _golden_eval_inputs(store):
    e = lambda k: store["eval/" + k]
    return d(e("scan")), d(e("path").astype(np.int32)), d(e("path_len")), d(e("gt").astype(np.int32)), d(e("gt_len"))


def test_golden_eval_rows():
    """ops.nav_eval on the golden's 42 trajectories (lengths 1, 2, 63, 64, 65, 130; the NaN corner) against env.py::_eval_item"""
    from vln_hamt_amd import ops
    store = load_npz("nav_reward.npz")
    out = ops.nav_eval(graphs(), *_golden_eval_inputs(store))
    assert out.dtype == torch.float64 and out.shape == (len(store["eval/scan"]), len(COLS))
    close_metrics(out.cpu().numpy(), store["eval/metrics"], "nav_eval vs reference")


def test_eval_metrics_equal_the_goldens_averages():
    """NavGraphs.eval_metrics: the reference's (avg_metrics, metrics) pair -- keys, `* 100` scalings, the per-item lists"""
    store = load_npz("nav_reward.npz")
    G, e = graphs(), (lambda k: store["eval/" + k])
    names = lambda s, p, n: [G.viewpoint(G.scans[s], v) for v in p[:n]]
    preds = [{"instr_id": f"i{i}", "trajectory": [(v, 0.0, 0.0) for v in names(e("scan")[i], e("path")[i], e("path_len")[i])]} for i in range(len(e("scan")))]
    gt_trajs = {f"i{i}": (G.scans[e("scan")[i]], names(e("scan")[i], e("gt")[i], e("gt_len")[i])) for i in range(len(e("scan")))}
    avg, metrics = G.eval_metrics(preds, gt_trajs)
    assert list(avg) == e("avg_keys").tolist() and list(metrics) == list(COLS) + ["instr_id"]
    close_metrics(np.array([[avg[k] for k in avg]]), e("avg")[None], "eval_metrics averages")
    assert metrics["instr_id"] == [p["instr_id"] for p in preds] and metrics["trajectory_steps"] == (e("path_len") - 1).tolist()
    close_metrics(np.stack([np.asarray(metrics[c], np.float64) for c in COLS], 1), e("metrics"), "eval_metrics items")


def test_eval_random_trajectories_vs_restatement():
    """300 random trajectories over the three scans, path and ground-truth lengths 1..130 (one, two and three 64-lane chunks), in one launch"""
    from vln_hamt_amd import ops
    G = graphs()
    rng = np.random.Generator(np.random.PCG64(41))
    nbrs, tables = [neighbours(G, s) for s in G.scans], host_tables(G)
    N = 300
    scan = rng.integers(0, 3, N).astype(np.int32)
    paths, gts = [], []
    for i in range(N):
        start = int(rng.integers(len(nbrs[scan[i]])))
        paths.append(random_walk(rng, nbrs[scan[i]], start, int(rng.integers(1, 131))))
        gts.append(random_walk(rng, nbrs[scan[i]], start, int(rng.integers(1, 131)), revisit=0.1))
    pack = lambda ps: (np.array([p + [-1] * (130 - len(p)) for p in ps], np.int32), np.array([len(p) for p in ps], np.int32))
    (pa, pl), (ga, gl) = pack(paths), pack(gts)
    out = ops.nav_eval(G, d(scan), d(pa), d(pl), d(ga), d(gl)).cpu().numpy()
    want = np.stack([eval_ref(tables[scan[i]][0], paths[i], gts[i]) for i in range(N)])
    close_metrics(out, want, "nav_eval vs restatement")


def test_over_long_input_is_refused():
    """A ground truth wider than HAMT_NAV_MAX_GT = 512 (or a path wider than 4096): HAMT_ERR_UNSUPPORTED, nothing launched; 512 runs"""
    from vln_hamt_amd import ops
    from vln_hamt_amd._lib import HamtError
    from vln_hamt_amd.agent import NavEpisodes
    G = graphs()
    one = lambda w: torch.zeros(1, w, dtype=torch.int32, device=DEV)
    n1, s = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.nav_eval(G, s, one(512), n1, one(512), n1)
    assert float(out[0, 0]) == 0.0 and float(out[0, 2]) == 0.0
    with pytest.raises(HamtError, match=r"status -2"):
        ops.nav_eval(G, s, one(8), n1, one(513), n1)
    with pytest.raises(HamtError, match=r"status -2"):
        ops.nav_eval(G, s, one(4097), n1, one(8), n1)
    with pytest.raises(HamtError):
        NavEpisodes(G, 4, 2, max_gt=513)
    nav = NavEpisodes(G, 4, 1, max_gt=8)
    with pytest.raises(HamtError):
        nav.reset(["scanA"], ["a00"], [["a00"] * 9])
    bad = ops.nav_eval(G, s, one(8), n1 * 9, one(8), n1)                 # a length beyond its row: a row of NaN, nothing read
    assert bool(torch.isnan(bad).all())


def test_captured_step_equals_eager_over_three_replays():
    """graph.GraphedInference over `RolloutRecorder.step(nav=..., sync=False)` (observe -> policy step -> advance) with the recorder's and
    the episodes' state declared: three replays without a reset in between walk the golden's first three steps exactly as three
    eager calls do -- every output and the whole episode state bit-identical, and the shortest-path teacher's targets the golden's."""
    from vln_hamt_amd.agent import RolloutRecorder
    from vln_hamt_amd.graph import GraphedInference
    store = load_npz("nav_reward.npz")
    g = lambda k: store["roll/" + k]
    T, B, V = g("cand").shape
    logits = d(_logits(store))
    outs = {}
    for name in ("graph", "eager"):
        rec = RolloutRecorder(T, B, DEV, ignoreid=int(store["meta/ignoreid"])).reset(B)
        nav = _golden_episodes(store, T)

        def fn(logit, cand, cl, forced, rec=rec, nav=nav):
            a_t, env, _ = rec.step(0, logit, cand_lens=cl, feedback="sample", forced_action=forced, nav=nav, cand_nodes=cand,
                                   teacher_mode="shortest", sync=False)
            return a_t, env, rec.target, rec.bt_mask, rec.reward[0], rec.ml[0]
        call = fn
        if name == "graph":
            gi = GraphedInference(fn, state=(rec.ended, rec.hist_len, *nav.state_tensors()))
            call = lambda *a: gi("step", *a)
        outs[name] = []
        with torch.no_grad():
            for k in range(3):
                out = [t.clone() for t in call(logits[k], d(g("cand")[k]), d(g("cand_len")[k]), d(g("a_t")[k]))]
                outs[name].append(out + [rec.ended.clone(), rec.hist_len.clone(), nav.arena.clone()])
    for k in range(3):
        for w, got in zip(outs["eager"][k], outs["graph"][k]):
            assert torch.equal(w, got), k
        assert np.array_equal(outs["graph"][k][2].cpu().numpy(), g("target/shortest")[k])
        assert np.array_equal(outs["graph"][k][1].cpu().numpy(), g("env_action")[k])
        assert float(np.abs(outs["graph"][k][4].cpu().numpy() - g("reward")[k]).max()) <= TOL_REWARD


def test_a_nav_step_makes_no_host_sync_but_the_action_copy():
    """RolloutRecorder.step(nav=...) under torch.cuda.set_sync_debug_mode('error'): observe, policy step and advance read nothing back;
    the declared copy of the int32 environment actions is the only transfer"""
    from vln_hamt_amd.agent import RolloutRecorder
    store = load_npz("nav_reward.npz")
    g = lambda k: store["roll/" + k]
    T, B, V = g("cand").shape
    logits, cand, cl, a_t = d(_logits(store)), d(g("cand")), d(g("cand_len")), d(g("a_t"))
    rec = RolloutRecorder(T, B, DEV).reset(B)
    nav = _golden_episodes(store, T)
    rec.step(0, logits[0], cand_lens=cl[0], forced_action=a_t[0], nav=nav, cand_nodes=cand[0])      # (first use: library load, allocator)
    rec.reset()
    nav = _golden_episodes(store, T)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, env0, _ = rec.step(0, logits[0], cand_lens=cl[0], forced_action=a_t[0], nav=nav, cand_nodes=cand[0], teacher_mode="path_index")
        env0 = env0.copy()
        _, env1, _ = rec.step(1, logits[1], cand_lens=cl[1], forced_action=a_t[1], nav=nav, cand_nodes=cand[1], teacher_mode="shortest", sync=False)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert isinstance(env0, np.ndarray) and np.array_equal(env0, g("env_action")[0])
    assert torch.is_tensor(env1) and np.array_equal(env1.cpu().numpy(), g("env_action")[1])
    assert float(np.abs(rec.reward[:2].cpu().numpy() - g("reward")[:2]).max()) <= TOL_REWARD


def test_rollout_loss_from_device_rewards():
    """The rollout's loss (imitation + A2C through a real Critic) with target, back-track mask and rewards from the device equals the
    loss of a second recorder that is handed the restatement's targets and masks and `set_rewards` of its rewards: 1e-6 relative."""
    from _policy_ref import critic_state_dict
    from vln_hamt_amd.agent import RolloutRecorder
    from vln_hamt_amd.models.model_HAMT import Critic
    store = load_npz("nav_reward.npz")
    g = lambda k: store["roll/" + k]
    T, B, V = g("cand").shape
    critic = Critic(types.SimpleNamespace(dropout=0.5, hamt_precision="fp32"))
    critic.load_state_dict(critic_state_dict(load_npz("policy_step.npz")), strict=True)
    critic = critic.to(DEV).eval()
    gen = torch.Generator().manual_seed(8)
    hidden, last_h = (torch.randn(T, B, 768, generator=gen) * 0.5).to(DEV), (torch.randn(B, 768, generator=gen) * 0.5).to(DEV)
    _, rec, nav, logits = _run_golden(store, "path_step", check=False)
    loss, _ = rec.loss(critic, hidden, last_h, train_ml=0.2)

    ref = EpisodesRef(golden_tables(store), g("scan"), g("start"), g("gt"), g("gt_len"))
    rec2 = RolloutRecorder(T, B, DEV, ignoreid=int(store["meta/ignoreid"])).reset(B)
    rewards = []
    for t in range(T):
        target, bt = ref.observe(t, g("cand")[t], g("cand_len")[t], g("ended")[t], "path_step", int(store["meta/ignoreid"]))
        rec2.step(t, logits[t], target=d(target), cand_lens=d(g("cand_len")[t]), bt_mask=d(bt), feedback="sample", forced_action=d(g("a_t")[t]))
        rewards.append(ref.advance(g("cand")[t], g("env_action")[t], (~g("ended")[t]).astype(np.float32))[0])
    rec2.set_rewards(np.stack(rewards))
    loss2, _ = rec2.loss(critic, hidden, last_h, train_ml=0.2)
    loss, loss2 = float(loss.detach()), float(loss2.detach())
    rel = abs(loss - loss2) / abs(loss2)
    print(f"[rollout loss] device rewards {loss:.7f}  host rewards {loss2:.7f}  relative {rel:.3e}")
    assert rel <= 1e-6, rel
