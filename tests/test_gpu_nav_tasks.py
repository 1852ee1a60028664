"""-m gpu: the navigation graphs on the device for CVDN, REVERIE and R2R-Back (csrc/nav.hip -> ops.nav_advance_goals / nav_advance_back /
nav_eval_goals / nav_eval_back -> agent.GoalSetEpisodes / ReturnEpisodes / NavGraphs.eval_metrics_* -> RolloutRecorder.step(nav=...))
against the reference's own statements (tests/golden/nav_tasks.npz) and the numpy restatement (tests/_nav_tasks_ref.py).

Bounds (tests/_nav_ref.py's): integers, masks, `ended`, `first_ended`, `midstop_at` and the fp32 distance exact; goal-set rewards exact
(constants chosen by comparing exactly rounded values); return-trip ndtw 2.4e-7 and reward 1e-6; metrics 1e-12 relative with NaNs in
the same places."""
import numpy as np
import pytest
import torch

from _nav_ref import CONNECTIVITY, MODES, TOL_NDTW, TOL_REWARD, close_metrics, host_tables, neighbours, random_walk
from _nav_tasks_ref import BACK_COLS, GOALS_COLS, GoalSetRef, ReturnRef, eval_back_ref, eval_goals_ref
from _util import load_npz
from test_nav_tasks import GOLDEN, back_golden_rollout, goals_golden_rollout

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


def _names(store, prefix, key, len_key):
    G, g = graphs(), (lambda k: store[prefix + "/" + k])
    scans = [G.scans[s] for s in g("scan")]
    return scans, [[G.viewpoint(sc, v) for v in row[:n]] for sc, row, n in zip(scans, g(key), g(len_key))]


def _episodes(store, prefix, T, poison=False):
    """the golden's episodes as a GoalSetEpisodes (`goals`) or a ReturnEpisodes (`back`, `back_eval`)"""
    from vln_hamt_amd.agent import GoalSetEpisodes, ReturnEpisodes
    G, g = graphs(), (lambda k: store[prefix + "/" + k])
    scans, gts = _names(store, prefix, "gt", "gt_len")
    starts = [G.viewpoint(sc, v) for sc, v in zip(scans, g("start"))]
    if prefix == "goals":
        nav, extra = GoalSetEpisodes(G, T, len(scans), max_gt=8, max_goals=65), _names(store, prefix, "goals", "goal_len")[1]
    else:
        nav, extra = ReturnEpisodes(G, T, len(scans), max_gt=128), [G.viewpoint(sc, v) for sc, v in zip(scans, g("midstop"))]
    if poison:
        nav.arena.fill_(0xFF)
    return nav.reset(scans, starts, gts, extra)


def _logits(store, prefix, seed=3):
    g = lambda k: store[prefix + "/" + k]
    T, B, V = g("cand").shape
    x = np.random.Generator(np.random.PCG64(seed)).standard_normal((T, B, V)).astype(np.float32)
    x[np.arange(V)[None, None] >= g("cand_len")[..., None]] = -np.inf
    return x


def _recorder(store, prefix, poison=False):
    from vln_hamt_amd.agent import RolloutRecorder
    T, B, _ = store[prefix + "/cand"].shape
    rec = RolloutRecorder(T, B, DEV, ignoreid=int(store["meta/ignoreid"]))
    if poison:
        for buf in (rec.ml, rec.logp, rec.ent, rec.mask, rec.reward):
            buf.fill_(float("nan"))
    return rec.reset(B)


def _run_goals(store, mode, poison=False, check=True):
    g = lambda k: store["goals/" + k]
    T, B, V = g("cand").shape
    rec, nav, logits = _recorder(store, "goals", poison), _episodes(store, "goals", T, poison), d(_logits(store, "goals"))
    res = {"init_last_dist": nav.last_dist.cpu().numpy()}

    def step(t, cand, cand_len, ended, a_t):
        assert np.array_equal(rec.ended.cpu().numpy().astype(bool), ended) and np.array_equal(nav.cur.cpu().numpy(), g("cur")[t])
        _, env, _ = rec.step(t, logits[t], cand_lens=d(cand_len), feedback="sample", forced_action=d(a_t), nav=nav, cand_nodes=d(cand), teacher_mode=mode)
        assert np.array_equal(env, g("env_action")[t]), (t, env)
        out = (rec.target.cpu().numpy(), rec.bt_mask.cpu().numpy(), rec.reward[t].cpu().numpy(), nav.last_dist.cpu().numpy())
        res[f"hist_len{t}"] = rec.hist_len.cpu().numpy()
        for k, v in zip(("target", "bt_mask", "reward", "dist"), out):
            res[f"{k}{t}"] = v
        return out
    if check:
        goals_golden_rollout(store, mode, step)
    else:
        for t in range(T):
            step(t, g("cand")[t], g("cand_len")[t], g("ended")[t], g("a_t")[t])
    res.update(path=nav.path.cpu().numpy(), path_len=nav.path_len.cpu().numpy(), anomalies=nav.anomalies.cpu().numpy(), cur=nav.cur.cpu().numpy(),
               mask=rec.mask.cpu().numpy(), ended=rec.ended.cpu().numpy())
    return res, rec, nav


def _hist_len(ended_rows):
    """hist_lens of the reference after each step: 1, then += 1 for every episode not ended before the step"""
    return 1 + np.cumsum(~ended_rows, axis=0)


@pytest.mark.parametrize("mode", MODES)
def test_goal_set_rollout_through_the_recorder(mode):
    """The golden's B = 6, T = 7 goal-set rollout (sizes 0, 1, 2, 3 and 65, three scans in one batch) through GoalSetEpisodes and
    RolloutRecorder.step(nav=...): target, back-track mask, distance and reward of every step against cvdn's own statements, exactly"""
    store = load_npz(GOLDEN)
    g = lambda k: store["goals/" + k]
    res, rec, nav = _run_goals(store, mode)
    assert np.array_equal(res["init_last_dist"], g("init_last_dist"))
    assert res["anomalies"].tolist() == [int(g(f"assert/{mode}").sum()), 0]
    assert np.array_equal(res["path_len"], g("path_len")) and np.array_equal(res["mask"], g("mask"))
    assert np.array_equal(res["ended"].astype(bool), g("final_ended"))
    for t, want in enumerate(_hist_len(g("ended"))):
        assert np.array_equal(res[f"hist_len{t}"], want), t
    for b, n in enumerate(g("path_len")):
        assert np.array_equal(res["path"][b, :n], g("path")[b, :n])


def _run_back(store, prefix, poison=False, check=True, rec=None, end_on_miss=None, feedback=None):
    g = lambda k: store[prefix + "/" + k]
    T, B, V = g("cand").shape
    rec = _recorder(store, prefix, poison) if rec is None else rec.reset(B)
    nav, logits = _episodes(store, prefix, T, poison), d(_logits(store, prefix))
    feedback = feedback or ("sample" if prefix == "back" else "argmax")              # (end_on_miss defaults to feedback == 'sample')
    res = {"init_last_dist": nav.last_dist.cpu().numpy(), "init_last_ndtw": nav.last_ndtw.cpu().numpy()}

    def step(t, cand, cand_len, a_t):
        assert np.array_equal(rec.ended.cpu().numpy().astype(bool), g("ended")[t]) and np.array_equal(nav.cur.cpu().numpy(), g("cur")[t])
        _, env, _ = rec.step(t, logits[t], cand_lens=d(cand_len), feedback=feedback, forced_action=d(a_t), nav=nav, cand_nodes=d(cand),
                             end_on_miss=end_on_miss)
        assert np.array_equal(env, g("env_action")[t]), (t, env)
        out = dict(target=rec.target.cpu().numpy(), bt_mask=rec.bt_mask.cpu().numpy(), reward=rec.reward[t].cpu().numpy(),
                   last_dist=nav.last_dist.cpu().numpy(), ndtw=nav.last_ndtw.cpu().numpy(), ended=rec.ended.cpu().numpy(),
                   first_ended=nav.first_ended.cpu().numpy(), midstop_at=nav.midstop_at.cpu().numpy(), mask=rec.mask[t].cpu().numpy(),
                   hist_len=rec.hist_len.cpu().numpy())
        for k, v in out.items():
            res[f"{k}{t}"] = v
        return out
    if check:
        back_golden_rollout(store, prefix, step)
    else:
        for t in range(T):
            step(t, g("cand")[t], g("cand_len")[t], g("a_t")[t])
    res.update(path=nav.path.cpu().numpy(), path_len=nav.path_len.cpu().numpy(), anomalies=nav.anomalies.cpu().numpy(), dtw_row=nav.dtw_row.cpu().numpy())
    return res, rec, nav


@pytest.mark.parametrize("prefix", ["back", "back_eval"])
def test_return_trip_rollout_through_the_recorder(prefix):
    """The golden's B = 6, T = 8 return trips through ReturnEpisodes and RolloutRecorder.step(nav=...): with feedback 'sample' (RL
    training: a missed mid-stop ends the episode; rewards against agent_r2rback.py's block) and with 'argmax' (it goes on): `ended`,
    `first_ended`, `midstop_at`, the mask rows and `hist_len` of every step, the walked paths, `midstops()`"""
    store = load_npz(GOLDEN)
    g = lambda k: store[prefix + "/" + k]
    res, rec, nav = _run_back(store, prefix)
    if prefix == "back":
        assert np.array_equal(res["init_last_dist"], g("init_last_dist")) and float(np.abs(res["init_last_ndtw"] - g("init_last_ndtw")).max()) <= TOL_NDTW
    assert res["anomalies"].tolist() == [int(g("assert/path_step").sum()), 0]
    for t, want in enumerate(_hist_len(g("ended"))):
        assert np.array_equal(res[f"hist_len{t}"], want), t
    assert np.array_equal(res["path_len"], g("path_len"))
    for b, n in enumerate(g("path_len")):
        assert np.array_equal(res["path"][b, :n], g("path")[b, :n])
    G = graphs()
    want = [None if v < 0 else G.viewpoint(G.scans[s], v) for s, v in zip(g("scan"), g("midstop_at")[-1])]
    assert nav.midstops() == want and None in want and any(w is not None for w in want)


def test_poisoned_state_changes_nothing(monkeypatch):
    """Every arena pre-filled with 0xFF, the recorder's arrays with NaN, before `reset`, and every torch.empty of the ops poisoned:
    bit-identical results and state for both kinds of episodes"""
    from test_gpu_policy_step import _poisoned_empty
    store = load_npz(GOLDEN)
    want = (_run_goals(store, "path_index", check=False)[0], _run_back(store, "back", check=False)[0])
    monkeypatch.setattr(torch, "empty", _poisoned_empty(torch.empty))
    got = (_run_goals(store, "path_index", poison=True, check=False)[0], _run_back(store, "back", poison=True, check=False)[0])
    monkeypatch.undo()
    for w_, g_ in zip(want, got):
        assert set(w_) == set(g_)
        for k, w in w_.items():
            assert np.array_equal(w, g_[k], equal_nan=k == "dtw_row") and (k == "dtw_row" or not np.isnan(g_[k].astype(np.float64)).any()), k


def _preds(store, flavour):
    G, e = graphs(), (lambda k: store[flavour + "/" + k])
    scans, paths = _names(store, flavour, "path", "path_len")
    return scans, [{"instr_id": f"i{i}", "trajectory": [(v, 0.0, 0.0) for v in p]} for i, p in enumerate(paths)]


def _check_metrics(store, flavour, avg, metrics, cols):
    e = lambda k: store[flavour + "/" + k]
    assert list(avg) == e("avg_keys").tolist() and list(metrics) == list(cols) + ["instr_id"]
    close_metrics(np.array([[avg[k] for k in avg]]), e("avg")[None], flavour + " averages")
    assert metrics["instr_id"] == [f"i{i}" for i in range(len(e("scan")))] and metrics["trajectory_steps"] == (e("path_len") - 1).tolist()
    got = np.stack([np.asarray(metrics[c], np.float64) for c in cols], 1)
    close_metrics(got, e("metrics"), flavour + " items")
    for c, k in enumerate(cols):
        if k in ("success", "oracle_success", "rgs"):
            assert np.array_equal(got[:, c], e("metrics")[:, c]), k


def test_eval_metrics_cvdn():
    """NavGraphs.eval_metrics_cvdn against cvdn/env.py::eval_metrics: keys, scalings, the per-item lists"""
    store = load_npz(GOLDEN)
    scans, preds = _preds(store, "cvdn")
    goals = _names(store, "cvdn", "goals", "goal_len")[1]
    avg, metrics = graphs().eval_metrics_cvdn(preds, {f"i{i}": (s, e_) for i, (s, e_) in enumerate(zip(scans, goals))})
    _check_metrics(store, "cvdn", avg, metrics, GOALS_COLS[:6])


def test_eval_metrics_reverie():
    """NavGraphs.eval_metrics_reverie against reverie/env.py::ReverieNavRefBatch.eval_metrics, `rgs` / `rgspl` included"""
    store = load_npz(GOLDEN)
    scans, preds = _preds(store, "reverie")
    goals, gts = _names(store, "reverie", "goals", "goal_len")[1], _names(store, "reverie", "gt", "gt_len")[1]
    for p, o in zip(preds, store["reverie/pred_obj"]):
        p["predObjId"] = None if o == -99 else int(o)
    avg, metrics = graphs().eval_metrics_reverie(preds, {f"i{i}": (s, g_, i) for i, (s, g_) in enumerate(zip(scans, gts))},
                                                 {f"{s}_{i}": e_ for i, (s, e_) in enumerate(zip(scans, goals))})
    _check_metrics(store, "reverie", avg, metrics, ("trajectory_steps", "trajectory_lengths", "success", "oracle_success", "spl", "rgs", "rgspl"))


def test_eval_metrics_back():
    """NavGraphs.eval_metrics_back against env.py::R2RBackBatch.eval_metrics (the NaN corner included)"""
    store = load_npz(GOLDEN)
    G, e = graphs(), (lambda k: store["backm/" + k])
    scans, preds = _preds(store, "backm")
    gts = _names(store, "backm", "gt", "gt_len")[1]
    for p, s, m in zip(preds, scans, e("midstop")):
        p["midstop"] = None if m < 0 else G.viewpoint(s, m)
    avg, metrics = G.eval_metrics_back(preds, {f"i{i}": (s, g_) for i, (s, g_) in enumerate(zip(scans, gts))},
                                       {f"i{i}": G.viewpoint(s, m) for i, (s, m) in enumerate(zip(scans, e("gt_midstop")))})
    _check_metrics(store, "backm", avg, metrics, BACK_COLS)


def _random_setup(B, V, seed):
    G = graphs()
    rng = np.random.Generator(np.random.PCG64(seed))
    nbrs = [neighbours(G, s) for s in G.scans]
    scan = [2 if b % 2 == 0 else b % 3 for b in range(B)]
    gts = [random_walk(rng, nbrs[scan[b]], rng.integers(len(nbrs[scan[b]])), (65, 2, 1, 65, 7)[b % 5], revisit=0.2) for b in range(B)]
    start = [gt[0] if b % 4 else int(rng.integers(len(nbrs[scan[b]]))) for b, gt in enumerate(gts)]
    gpad = np.full((B, 65), -1, np.int32)
    for b, g_ in enumerate(gts):
        gpad[b, :len(g_)] = g_
    name = lambda b, v: G.viewpoint(G.scans[scan[b]], v)
    return G, rng, nbrs, scan, gts, start, gpad, np.array([len(g_) for g_ in gts], np.int32), name


def _random_step(rng, nbrs, scan, cur, ended, V):
    B = len(scan)
    cand, cl, env = np.full((B, V), -1, np.int32), np.zeros(B, np.int32), np.full(B, -1, np.int32)
    for b in range(B):
        nb = nbrs[scan[b]][cur[b]]
        nb = [nb[j] for j in rng.permutation(len(nb))][:V - 1]
        cand[b, :len(nb)], cl[b] = nb, len(nb) + 1
        if not ended[b] and rng.random() > 0.15:
            env[b] = int(rng.integers(len(nb)))
    return cand, cl, env


@pytest.mark.parametrize("B,V", [(5, 3), (9, 70)])
def test_random_goal_set_rollouts_vs_restatement(B, V):
    """B = 5 / 9 episodes (a partly filled workgroup of 4 waves), goal lists of 64, 65, 130, 256 and 0 entries over four nodes each, ground truths
    of 65 nodes, candidates padded to V = 3 / 70, T = 10 random steps: every step's target, mask, distance and reward, and the final
    state, equal the restatement's"""
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import GoalSetEpisodes
    G, rng, nbrs, scan, gts, start, gpad, glen, name = _random_setup(B, V, 300 + V)
    T = 10
    sets = [[int(v) for v in rng.choice(rng.integers(len(nbrs[scan[b]]), size=4), size=(64, 65, 130, 256, 0)[b % 5])] for b in range(B)]     # (four nodes, repeated)
    nav = GoalSetEpisodes(G, T, B, max_gt=65, max_goals=256).reset([G.scans[s] for s in scan], [name(b, v) for b, v in enumerate(start)],
                                                                   [[name(b, v) for v in gt] for b, gt in enumerate(gts)],
                                                                   [[name(b, v) for v in e_] for b, e_ in enumerate(sets)])
    epad = np.full((B, 256), -1, np.int32)
    for b, e_ in enumerate(sets):
        epad[b, :len(e_)] = e_
    ref = GoalSetRef(host_tables(G), scan, start, gpad, glen, epad, np.array([len(e_) for e_ in sets], np.int32))
    assert np.array_equal(nav.last_dist.cpu().numpy(), ref.last_dist)
    ended = np.zeros(B, bool)
    for t in range(T):
        cand, cl, env = _random_step(rng, nbrs, scan, ref.cur, ended, V)
        mode = MODES[t % 3]
        target, bt = ops.nav_observe(nav, t, d(cand), d(cl), d(ended.astype(np.uint8)), mode=mode)
        mask = (~ended).astype(np.float32)
        reward = ops.nav_advance_goals(nav, d(cand), d(env), d(mask), torch.full((B,), float("nan"), device=DEV)).cpu().numpy()
        w_target, w_bt = ref.observe(t, cand, cl, ended, mode)
        w_reward, w_dist = ref.advance(cand, env, mask)
        assert np.array_equal(target.cpu().numpy(), w_target) and np.array_equal(bt.cpu().numpy(), w_bt), (t, mode)
        assert np.array_equal(nav.last_dist.cpu().numpy(), w_dist) and np.array_equal(nav.cur.cpu().numpy(), ref.cur), t
        assert np.array_equal(reward, w_reward), (t, reward, w_reward)
        ended |= env == -1
    assert nav.anomalies.cpu().tolist() == ref.anomalies
    path, n = nav.path.cpu().numpy(), nav.path_len.cpu().numpy()
    for b in range(B):
        assert path[b, :n[b]].tolist() == ref.path[b]


@pytest.mark.parametrize("B,V", [(5, 3), (9, 70)])
def test_random_return_trips_vs_restatement(B, V):
    """The same shapes for return trips (ground truths of 65, 2, 1 and 7 nodes), `end_on_miss` on for the even steps' batch and off for
    the odd one: reward, fp32 distance, nDTW, `ended`, `first_ended`, `midstop_at`, the DTW rows and the anomaly counters"""
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import ReturnEpisodes
    for end_on_miss in (True, False):
        G, rng, nbrs, scan, gts, start, gpad, glen, name = _random_setup(B, V, 500 + V + int(end_on_miss))
        T = 10
        mids = [gt[len(gt) // 2] for gt in gts]
        nav = ReturnEpisodes(G, T, B, max_gt=65).reset([G.scans[s] for s in scan], [name(b, v) for b, v in enumerate(start)],
                                                       [[name(b, v) for v in gt] for b, gt in enumerate(gts)], [name(b, v) for b, v in enumerate(mids)])
        ref = ReturnRef(host_tables(G), scan, start, gpad, glen, mids)
        assert np.array_equal(nav.last_dist.cpu().numpy(), ref.last_dist)
        ended, dev_ended = np.zeros(B, bool), torch.zeros(B, dtype=torch.uint8, device=DEV)
        worst_n = worst_r = 0.0
        for t in range(T):
            cand, cl, env = _random_step(rng, nbrs, scan, ref.cur, ended, V)
            mask = (~ended).astype(np.float32)
            dev_ended.copy_(d((ended | (env < 0)).astype(np.uint8)))                     # (what the policy step leaves)
            reward = ops.nav_advance_back(nav, d(cand), d(env), d(mask), torch.full((B,), float("nan"), device=DEV), dev_ended,
                                          end_on_miss=end_on_miss).cpu().numpy()
            w_reward, w_dist, w_ndtw, ended = ref.advance(cand, env, mask, ended | (env < 0), end_on_miss=end_on_miss)
            assert np.array_equal(dev_ended.cpu().numpy().astype(bool), ended), t
            assert np.array_equal(nav.first_ended.cpu().numpy().astype(bool), ref.first_ended) and np.array_equal(nav.midstop_at.cpu().numpy(), ref.midstop_at), t
            assert np.array_equal(nav.last_dist.cpu().numpy(), ref.last_dist) and np.array_equal(nav.cur.cpu().numpy(), ref.cur), t
            worst_n = max(worst_n, float(np.abs(nav.last_ndtw.cpu().numpy().astype(np.float64) - w_ndtw).max()))
            worst_r = max(worst_r, float(np.abs(reward.astype(np.float64) - w_reward).max()))
        print(f"[random return trips B {B} V {V} end_on_miss {end_on_miss}] max|d ndtw| {worst_n:.3e}  max|d reward| {worst_r:.3e}  anomalies {ref.anomalies}")
        assert worst_n <= TOL_NDTW and worst_r <= TOL_REWARD
        assert nav.anomalies.cpu().tolist() == ref.anomalies
        assert ref.first_ended.any() and (ref.midstop_at >= 0).any() and ended.any()
        row = nav.dtw_row.cpu().numpy()
        for b in range(B):
            assert np.abs(row[b, 1:glen[b] + 1] - ref.row[b][1:]).max() <= 1e-12 * max(ref.row[b][1:].max(), 1e-300)


def test_eval_random_trajectories_vs_restatement():
    """120 random trajectories per kernel over the three scans: paths of 1..130 nodes; goal sets of 1, 64, 65, 130 and 256 entries
    (distinct where the scan has that many nodes) with and without a ground truth of up to 65 nodes; return trips with mid-stops set,
    unset, near and far"""
    from vln_hamt_amd import ops
    G = graphs()
    rng = np.random.Generator(np.random.PCG64(43))
    nbrs, tb = [neighbours(G, s) for s in G.scans], host_tables(G)
    N = 120
    scan = rng.integers(0, 3, N).astype(np.int32)
    paths, gts, sets, mids, gmids = [], [], [], [], []
    for i in range(N):
        n = len(nbrs[scan[i]])
        start = int(rng.integers(n))
        paths.append(random_walk(rng, nbrs[scan[i]], start, int(rng.integers(1, 131))))
        gts.append(random_walk(rng, nbrs[scan[i]], start, int(rng.integers(1, 66)), revisit=0.1))
        sets.append([int(v) for v in rng.integers(n, size=(1, 64, 65, 130, 256, 3)[i % 6])])
        gmids.append(gts[-1][len(gts[-1]) // 2])
        mids.append(-1 if i % 5 == 0 else gmids[-1] if i % 5 == 1 else paths[-1][int(rng.integers(len(paths[-1])))])
    pack = lambda ps, w: (np.array([p + [-1] * (w - len(p)) for p in ps], np.int32), np.array([len(p) for p in ps], np.int32))
    (pa, pl), (ga, gl), (ea, el) = pack(paths, 130), pack(gts, 65), pack(sets, 256)
    out = ops.nav_eval_goals(G, d(scan), d(pa), d(pl), d(ea), d(el)).cpu().numpy()
    close_metrics(out, np.stack([eval_goals_ref(tb[scan[i]][0], paths[i], sets[i]) for i in range(N)]), "nav_eval_goals (no gt) vs restatement")
    out = ops.nav_eval_goals(G, d(scan), d(pa), d(pl), d(ea), d(el), d(ga), d(gl)).cpu().numpy()
    close_metrics(out, np.stack([eval_goals_ref(tb[scan[i]][0], paths[i], sets[i], gts[i]) for i in range(N)]), "nav_eval_goals (gt) vs restatement")
    out = ops.nav_eval_back(G, d(scan), d(pa), d(pl), d(ga), d(gl), d(np.array(mids, np.int32)), d(np.array(gmids, np.int32))).cpu().numpy()
    want = np.stack([eval_back_ref(tb[scan[i]][0], paths[i], gts[i], mids[i], gmids[i]) for i in range(N)])
    close_metrics(out, want, "nav_eval_back vs restatement")
    assert np.array_equal(out[:, 3], want[:, 3]) and {0.0, 1.0} == set(want[:, 3].tolist())


def test_too_many_goals_are_refused():
    """257 goals (HAMT_NAV_MAX_GOALS = 256): HAMT_ERR_UNSUPPORTED, nothing launched; 256 runs; a length or a node outside its table: NaN"""
    from vln_hamt_amd import ops
    from vln_hamt_amd._lib import HamtError
    from vln_hamt_amd.agent import GoalSetEpisodes
    G = graphs()
    one = lambda w: torch.zeros(1, w, dtype=torch.int32, device=DEV)
    n1, s = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.nav_eval_goals(G, s, one(4), n1, one(256), n1 * 256)
    assert out[0].tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    with pytest.raises(HamtError, match=r"status -2"):
        ops.nav_eval_goals(G, s, one(4), n1, one(257), n1)
    with pytest.raises(HamtError):
        GoalSetEpisodes(G, 4, 2, max_goals=257)
    nav = GoalSetEpisodes(G, 4, 1, max_gt=4, max_goals=2)
    with pytest.raises(HamtError):
        nav.reset(["scanA"], ["a00"], [["a00"]], [["a00", "a01", "a02"]])
    nav.reset(["scanA"], ["a00"], [["a00"]], [["a01", "a02"]])
    nav.E_max = 257                                                       # (the binding's own check, behind the class's)
    with pytest.raises(HamtError, match=r"status -2"):
        ops.nav_advance_goals(nav, one(3), s - 1, torch.ones(1, device=DEV), torch.zeros(1, device=DEV))
    assert bool(torch.isnan(ops.nav_eval_goals(G, s, one(4), n1, one(8), n1 * 9)).all())             # a goal count beyond its row
    assert bool(torch.isnan(ops.nav_eval_goals(G, s, one(4), n1, one(8), n1 * 0)).all())             # an empty goal set has no nearest goal
    assert bool(torch.isnan(ops.nav_eval_back(G, s, one(4), n1, one(4), n1, n1 * 7, n1)).all())      # a mid-stop outside scanA's 7 nodes
    assert not bool(torch.isnan(ops.nav_eval_back(G, s, one(4), n1 * 2, one(4), n1 * 2, n1 * -1, n1)[0, :8]).any())


def test_captured_return_trip_step_equals_eager_for_a_whole_rollout():
    """graph.GraphedInference over `RolloutRecorder.step(nav=..., sync=False)` (observe -> policy step -> advance_back) with the
    recorder's `ended` / `hist_len` and the episodes' state declared: T replays walk the golden's whole return-trip rollout exactly as T
    eager calls do -- every output and the whole episode state bit-identical, `ended` the golden's"""
    from vln_hamt_amd.graph import GraphedInference
    store = load_npz(GOLDEN)
    g = lambda k: store["back/" + k]
    T, B, V = g("cand").shape
    logits = d(_logits(store, "back"))
    outs = {}
    for name in ("graph", "eager"):
        rec, nav = _recorder(store, "back"), _episodes(store, "back", T)

        def fn(logit, cand, cl, forced, rec=rec, nav=nav):
            a_t, env, _ = rec.step(0, logit, cand_lens=cl, feedback="sample", forced_action=forced, nav=nav, cand_nodes=cand,
                                   teacher_mode="shortest", sync=False)
            return a_t, env, rec.target, rec.bt_mask, rec.reward[0], rec.ml[0], rec.mask[0]
        call = fn
        if name == "graph":
            gi = GraphedInference(fn, state=(rec.ended, rec.hist_len, *nav.state_tensors()))
            call = lambda *a: gi("step", *a)
        outs[name] = []
        with torch.no_grad():
            for k in range(T):
                out = [t.clone() for t in call(logits[k], d(g("cand")[k]), d(g("cand_len")[k]), d(g("a_t")[k]))]
                outs[name].append(out + [rec.ended.clone(), rec.hist_len.clone(), nav.arena.clone()])
    for k in range(T):
        for w, got in zip(outs["eager"][k], outs["graph"][k]):
            assert torch.equal(w, got), k
        assert np.array_equal(outs["graph"][k][1].cpu().numpy(), g("env_action")[k])
        assert np.array_equal(outs["graph"][k][7].cpu().numpy().astype(bool), g("ended_after")[k])
        assert float(np.abs(outs["graph"][k][4].cpu().numpy() - g("reward")[k]).max()) <= TOL_REWARD


def test_r2r_rollout_is_unchanged_after_a_return_trip_on_the_same_recorder():
    """The R2R golden rollout (tests/golden/nav_reward.npz) through a recorder that has just served a return-trip rollout, against the
    same rollout through a fresh recorder: bit-identical"""
    import test_gpu_nav_graph as r2r
    from vln_hamt_amd.agent import RolloutRecorder
    store, base = load_npz(GOLDEN), load_npz("nav_reward.npz")
    g = lambda k: base["roll/" + k]
    T, B, V = g("cand").shape
    want = r2r._run_golden(base, "path_step", check=False)[0]
    rec = RolloutRecorder(max(T, store["back/cand"].shape[0]), B, DEV, ignoreid=int(base["meta/ignoreid"]))
    _run_back(store, "back", check=False, rec=rec)
    rec.reset(B)
    nav, logits = r2r._golden_episodes(base, T), r2r.d(r2r._logits(base))
    for t in range(T):
        _, env, _ = rec.step(t, logits[t], cand_lens=d(g("cand_len")[t]), feedback="sample", forced_action=d(g("a_t")[t]), nav=nav,
                             cand_nodes=d(g("cand")[t]), teacher_mode="path_step")
        assert np.array_equal(env, g("env_action")[t])
        for k, v in (("target", rec.target), ("bt_mask", rec.bt_mask), ("reward", rec.reward[t]), ("dist", nav.last_dist), ("ndtw", nav.last_ndtw)):
            assert np.array_equal(v.cpu().numpy(), want[f"{k}{t}"]), (k, t)
    assert np.array_equal(rec.mask[:T].cpu().numpy(), want["mask"]) and np.array_equal(nav.path.cpu().numpy(), want["path"])
    assert np.array_equal(nav.dtw_row.cpu().numpy(), want["dtw_row"]) and nav.anomalies.cpu().tolist() == want["anomalies"].tolist()
