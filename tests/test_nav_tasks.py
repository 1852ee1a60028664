"""Not gpu: the navigation graphs on the device for CVDN, REVERIE and R2R-Back (the goal-set and return-trip kernels of
vln_hamt_amd/csrc/nav.hip, ops.nav_advance_goals / nav_advance_back / nav_eval_goals / nav_eval_back, agent.GoalSetEpisodes /
ReturnEpisodes) -- the numpy restatement the GPU tests compare against reproduces the REFERENCE's own statements
(tests/golden/nav_tasks.npz, tools/gen_nav_tasks_golden.py), the golden holds the corners it was scripted for, the new entry points are
declared and bound, and the cross-compiled kernels use no scratch memory."""
import os
import re
import subprocess

import numpy as np
import pytest

from _nav_ref import MODES, TOL_NDTW, TOL_REWARD, close_metrics
from _nav_tasks_ref import BACK_COLS, GOALS_COLS, GoalSetRef, ReturnRef, eval_back_ref, eval_goals_ref
from _util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hamt_nav_advance_goals", "hamt_nav_advance_back", "hamt_nav_eval_goals", "hamt_nav_eval_back")
KERNELS = r"nav_(goals|back)_(step|eval)_kernel"
GOLDEN = "nav_tasks.npz"


def _entry_points():
    from vln_hamt_amd import _lib
    return [_lib.SIGNATURES[n] for n in NAMES]


def tables(store):
    """[(dist fp64 [n, n], nxt int32 [n, n])] per scan: the networkx tables of tests/golden/nav_reward.npz (the same three scans)"""
    from _nav_ref import golden_tables
    base = load_npz("nav_reward.npz")
    assert base["meta/scans"].tolist() == store["meta/scans"].tolist()
    return golden_tables(base)


def env_of(a_t, cand_len, ended, ignoreid):
    """the environment action of a_t (cvdn/agent.py:138-141, ops.policy_step)"""
    return np.where((a_t == cand_len - 1) | (a_t == ignoreid) | ended, -1, a_t).astype(np.int32)


def goals_golden_rollout(store, mode, step):
    """drive `step(t, cand_node, cand_len, ended, a_t) -> (target, bt_mask, reward, dist)` over the golden's goal-set rollout: every
    answer equal to the reference's (the rewards are constants picked by comparing exactly rounded values)"""
    g = lambda k: store["goals/" + k]
    T, B = g("cand_len").shape
    for t in range(T):
        target, bt, reward, dist = step(t, g("cand")[t], g("cand_len")[t], g("ended")[t], g("a_t")[t])
        assert np.array_equal(target, g(f"target/{mode}")[t]), (mode, t, target, g(f"target/{mode}")[t])
        assert np.array_equal(bt, g("bt_mask")[t]), (t, bt, g("bt_mask")[t])
        assert np.array_equal(dist, g("dist")[t]), (t, dist, g("dist")[t])
        assert np.array_equal(reward, g("reward")[t]), (t, reward, g("reward")[t])


def back_golden_rollout(store, prefix, step):
    """drive `step(t, cand_node, cand_len, a_t) -> dict(target, bt_mask, reward, last_dist, ndtw, ended, first_ended, midstop_at, mask)`
    over a return-trip rollout of the golden (`back`: with the reference's rewards; `back_eval`: train_rl off, state only)"""
    g = lambda k: store[prefix + "/" + k]
    T, B = g("cand_len").shape
    for t in range(T):
        out = step(t, g("cand")[t], g("cand_len")[t], g("a_t")[t])
        assert np.array_equal(out["target"], g("target/path_step")[t]), (t, out["target"], g("target/path_step")[t])
        assert np.array_equal(out["bt_mask"], g("bt_mask")[t]), t
        assert np.array_equal(out["mask"], (~g("ended")[t]).astype(np.float32)), t
        assert np.array_equal(out["ended"].astype(bool), g("ended_after")[t]), (t, out["ended"], g("ended_after")[t])
        assert np.array_equal(out["first_ended"].astype(bool), g("first_ended_after")[t]), (t, out["first_ended"])
        assert np.array_equal(out["midstop_at"], g("midstop_at")[t]), (t, out["midstop_at"], g("midstop_at")[t])
        if prefix == "back":
            assert np.array_equal(out["mask"], g("mask")[t]) and np.array_equal(out["last_dist"], g("last_dist")[t]), (t, out["last_dist"])      # fp32: exact
            e_n = float(np.abs(out["ndtw"].astype(np.float64) - g("ndtw")[t]).max())
            e_r = float(np.abs(out["reward"].astype(np.float64) - g("reward")[t]).max())
            print(f"[{prefix} step {t}] max|d ndtw| {e_n:.3e}  max|d reward| {e_r:.3e}")
            assert e_n <= TOL_NDTW and e_r <= TOL_REWARD, (t, e_n, e_r)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_reproduces_the_goal_set_rollout(mode):
    """GoalSetRef against cvdn/env.py's `min_dist` block and cvdn/agent.py's init and reward blocks: everything exact"""
    _entry_points()
    store = load_npz(GOLDEN)
    g = lambda k: store["goals/" + k]
    ep = GoalSetRef(tables(store), g("scan"), g("start"), g("gt"), g("gt_len"), g("goals"), g("goal_len"))
    assert np.array_equal(ep.last_dist, g("init_last_dist"))
    ignoreid = int(store["meta/ignoreid"])

    def step(t, cand, cand_len, ended, a_t):
        assert ep.cur == g("cur")[t].tolist()
        target, bt = ep.observe(t, cand, cand_len, ended, mode, ignoreid)
        env = env_of(a_t, cand_len, ended, ignoreid)
        assert np.array_equal(env, g("env_action")[t])
        reward, dist = ep.advance(cand, env, (~ended).astype(np.float32))
        return target, bt, reward, dist
    goals_golden_rollout(store, mode, step)
    assert ep.anomalies == [int(g(f"assert/{mode}").sum()), 0], ep.anomalies
    for b in range(ep.B):
        assert ep.path[b] == g("path")[b, :g("path_len")[b]].tolist()


@pytest.mark.parametrize("prefix", ["back", "back_eval"])
def test_restatement_reproduces_the_return_trip_rollout(prefix):
    """ReturnRef against agent_r2rback.py's init, env-action / mid-stop and reward blocks, with train_rl (`back`: a missed mid-stop
    ends the episode) and without (`back_eval`: it goes on)"""
    _entry_points()
    store = load_npz(GOLDEN)
    g = lambda k: store[prefix + "/" + k]
    ep = ReturnRef(tables(store), g("scan"), g("start"), g("gt"), g("gt_len"), g("midstop"))
    if prefix == "back":
        assert np.array_equal(ep.last_dist, g("init_last_dist")) and float(np.abs(ep.last_ndtw - g("init_last_ndtw")).max()) <= TOL_NDTW
    ignoreid = int(store["meta/ignoreid"])
    ended = np.zeros(ep.B, bool)

    def step(t, cand, cand_len, a_t):
        nonlocal ended
        assert ep.cur == g("cur")[t].tolist() and np.array_equal(ended, g("ended")[t]) and np.array_equal(ep.first_ended, g("first_ended")[t])
        target, bt = ep.observe(t, cand, cand_len, ended, "path_step", ignoreid)
        env, mask = env_of(a_t, cand_len, ended, ignoreid), (~ended).astype(np.float32)
        assert np.array_equal(env, g("env_action")[t])
        reward, dist, ndtw, ended = ep.advance(cand, env, mask, ended | (env < 0), end_on_miss=prefix == "back")
        if prefix == "back":
            assert np.array_equal(dist, g("dist")[t]), (t, dist, g("dist")[t])
        return dict(target=target, bt_mask=bt, reward=reward, last_dist=ep.last_dist.copy(), ndtw=ndtw, ended=ended, first_ended=ep.first_ended.copy(),
                    midstop_at=ep.midstop_at.copy(), mask=mask)
    back_golden_rollout(store, prefix, step)
    assert ep.anomalies == [int(g("assert/path_step").sum()), 0], ep.anomalies
    for b in range(ep.B):
        assert ep.path[b] == g("path")[b, :g("path_len")[b]].tolist()


def eval_rows(store, flavour, fn):
    """`fn(dist, i, get)` per trajectory of an evaluation part of the golden, stacked"""
    e = lambda k: store[flavour + "/" + k]
    tb = tables(store)
    return np.stack([fn(tb[e("scan")[i]][0], i, e) for i in range(len(e("scan")))])


def test_restatement_reproduces_the_reference_metrics():
    """eval_goals_ref / eval_back_ref against cvdn/env.py, reverie/env.py and R2RBackBatch `_eval_item` (through `eval_metrics`): 1e-12
    relative, NaN where the reference has NaN, the 0 / 1 columns exact"""
    _entry_points()
    store = load_npz(GOLDEN)
    cut = lambda e, k, i: e(k)[i, :e(k + "_len")[i]]
    got = eval_rows(store, "cvdn", lambda dist, i, e: eval_goals_ref(dist, cut(e, "path", i), e("goals")[i, :e("goal_len")[i]]))
    close_metrics(got[:, :6], store["cvdn/metrics"], "cvdn restatement vs reference")
    assert np.array_equal(got[:, [0, 2, 3]], store["cvdn/metrics"][:, [0, 2, 3]])
    got = eval_rows(store, "reverie", lambda dist, i, e: eval_goals_ref(dist, cut(e, "path", i), e("goals")[i, :e("goal_len")[i]], cut(e, "gt", i)))
    want = store["reverie/metrics"]
    close_metrics(got[:, :5], want[:, :5], "reverie restatement vs reference")
    close_metrics((want[:, 5] * got[:, 6])[:, None], want[:, 6:7], "reverie rgspl = rgs * spl_ratio")
    assert np.array_equal(got[:, [0, 2, 3]], want[:, [0, 2, 3]])
    got = eval_rows(store, "backm", lambda dist, i, e: eval_back_ref(dist, cut(e, "path", i), cut(e, "gt", i), e("midstop")[i], e("gt_midstop")[i]))
    close_metrics(got, store["backm/metrics"], "return-trip restatement vs reference")
    assert np.array_equal(got[:, [1, 3]], store["backm/metrics"][:, [1, 3]])


def test_golden_holds_the_corners_the_issue_names():
    _entry_points()
    store = load_npz(GOLDEN)
    tb = tables(store)
    ignoreid = int(store["meta/ignoreid"])
    # ---- the goal-set rollout
    g = lambda k: store["goals/" + k]
    T, B = g("cand_len").shape
    assert (B, T) == (6, 7) and set(g("scan").tolist()) == {0, 1, 2}
    assert {0, 1, 3, 65} <= set(g("goal_len").tolist()) and g("scan")[g("goal_len") == 65].tolist() == [2]        # across the 64-lane stride, on scanC
    assert any(len(set(row[:n].tolist())) < n for row, n in zip(g("goals"), g("goal_len")))                     # a duplicate node
    r, m, env, d = g("reward"), g("mask"), g("env_action"), g("dist")
    last = np.concatenate([g("init_last_dist")[None], d[:-1]])
    live = m == 1
    assert (live & (env == -1) & (d == 0) & (r == 2)).any()                                                     # a stop on a goal
    assert (live & (env == -1) & (d > 0) & (d < 3) & (r == -2)).any()                                           # R2R's rule would say +2
    assert (live & (env >= 0) & (d < last) & (r == 1)).any() and (live & (env >= 0) & (d > last) & (r == -1)).any()
    assert (live & (env >= 0) & (d == last) & (r == 0)).any()                                                   # the distance unchanged: 0, no error
    assert (live & (env >= 0) & (d == last) & (r == 0) & (g("goal_len")[None] > 0)).any()                       # ... also with a goal set
    assert (~live).any() and (r[~live] == 0).all() and (env[~live] == -1).all()                                 # rows after the end
    assert not g("final_ended").all() and g("final_ended").any()
    changed = decided_by_last = False
    for b in range(B):                                                                                          # which goal is the nearest, step by step
        E, dist = g("goal_len")[b], tb[g("scan")[b]][0]
        if E == 0:
            continue
        walked = g("path")[b, :g("path_len")[b]]
        near = [int(np.argmin(dist[v, g("goals")[b, :E]])) for v in walked]
        changed |= len({g("goals")[b, k] for k in near}) > 1
        decided_by_last |= E == 65 and 64 in near
    assert changed and decided_by_last
    for mode in MODES:
        assert (g(f"target/{mode}")[g("ended")] == ignoreid).all()
    assert not np.array_equal(g("target/path_step"), g("target/shortest"))
    # ---- the return trips
    b_, be = (lambda k: store["back/" + k]), (lambda k: store["back_eval/" + k])
    T, B = b_("cand_len").shape
    assert (B, T) == (6, 8) and set(b_("scan").tolist()) == {0, 1, 2} and b_("gt_len").max() > 64
    for gt, n, mid in zip(b_("gt"), b_("gt_len"), b_("midstop")):                                               # the mid-stop twice in a row
        assert any(gt[j] == mid and gt[j + 1] == mid for j in range(n - 1))
    r, m, env, d, fe = b_("reward"), b_("mask"), b_("env_action"), b_("dist"), b_("first_ended")
    live, stop = m == 1, env == -1
    first, second = live & stop & ~fe, live & stop & fe
    hit_both = (first & (d < 3)).any(0) & (second & (d < 3)).any(0)
    assert hit_both.any()                                                                                       # a hit mid-stop, then a hit final stop
    assert (first & (d > 0) & (d < 3) & (r > 2)).any()                                                          # a hit that is not exact
    missed = (first & (d >= 3)).any(0)
    assert missed.any() and (r[first & (d >= 3)] == -2).all()
    t_miss, e_miss = [int(v[0]) for v in np.nonzero(first & (d >= 3))]
    assert b_("ended_after")[t_miss, e_miss] and not be("ended_after")[t_miss, e_miss]                          # ends at once / goes on
    assert np.array_equal(b_("a_t")[:t_miss + 1], be("a_t")[:t_miss + 1]) and be("env_action")[t_miss + 1, e_miss] >= 0      # the same script
    assert be("ended_after")[-1, e_miss] and be("path_len")[e_miss] > b_("path_len")[e_miss]
    after = np.zeros_like(first)
    after[1:] = first[:-1]                                                                                     # the step after the first stop
    d0 = np.array([[tb[s][0][v, mid] for s, v, mid in zip(b_("scan"), row, b_("midstop"))] for row in np.concatenate([b_("cur")[1:], b_("cur")[-1:]])])
    prev0 = np.array([[tb[s][0][v, mid] for s, v, mid in zip(b_("scan"), row, b_("midstop"))] for row in b_("cur")])
    assert (after & live & (env >= 0) & (r > 0) & (d0 > prev0)).any()                                           # closer to the END, away from the mid-stop: > 0
    assert (b_("midstop_at")[-1] == -1).any() and not b_("ended_after")[-1].all()                               # an episode that never stops
    assert ((b_("a_t") == ignoreid) & first).any()                                                              # an ignored action as the stop
    assert (second & (d >= 3) & (r == -2)).any()                                                                # a missed final stop
    assert (~live).any() and (r[~live] == 0).all() and (env[~live] == -1).all()
    # ---- evaluation
    for flavour, n_cols in (("cvdn", 6), ("reverie", 7), ("backm", 9)):
        e = lambda k: store[flavour + "/" + k]
        assert 26 <= len(e("scan")) <= 34 and e("metrics").shape == (len(e("scan")), n_cols)
        pl = e("path_len")[e("scan") == 2]
        assert {1, 2, 64, 65, 130} <= set(pl.tolist()), flavour
    for flavour in ("cvdn", "reverie"):
        e = lambda k: store[flavour + "/" + k]
        assert {1, 3, 65} <= set(e("goal_len").tolist())
        assert {0.0, 1.0} == set(e("metrics")[:, 2].tolist()) and (e("metrics")[:, 3] > e("metrics")[:, 2]).any()      # oracle success alone
    c = store["cvdn/metrics"]
    assert (c[:, 5] > 0).any() and (c[:, 5] < 0).any()                                                          # gp of both signs
    inside = [p[0] in gs[:n] for p, gs, n in zip(store["cvdn/path"], store["cvdn/goals"], store["cvdn/goal_len"])]
    assert any(inside) and (c[np.array(inside), 5] <= 0).all()                                                  # gt_lengths 0
    assert store["cvdn/avg_keys"].tolist() == ["steps", "lengths", "sr", "oracle_sr", "spl", "gp"]
    rv = store["reverie/metrics"]
    assert store["reverie/avg_keys"].tolist() == ["steps", "lengths", "sr", "oracle_sr", "spl", "rgs", "rgspl"]
    assert ((rv[:, 5] == 1) & (rv[:, 2] == 0)).any() and ((rv[:, 5] == 0) & (rv[:, 2] == 1)).any() and (store["reverie/pred_obj"] == -99).any()
    e = lambda k: store["backm/" + k]
    mid_ok = np.array([mid >= 0 and tb[s][0][mid, gm] <= 3.0 for s, mid, gm in zip(e("scan"), e("midstop"), e("gt_midstop"))])
    end_ok = e("metrics")[:, 0] <= 3.0
    for a in (True, False):                                                                                     # each of the two conditions, held and failed
        for b in (True, False):
            assert ((mid_ok == a) & (end_ok == b)).any(), (a, b)
    assert np.array_equal(e("metrics")[:, 3], (mid_ok & end_ok).astype(np.float64)) and (e("midstop") == -1).any()
    assert np.isnan(e("metrics")).sum() == 1 and np.isnan(e("metrics")[:, 8]).sum() == 1                        # the NaN corner: CLS only, once
    assert e("avg_keys").tolist() == ["steps", "lengths", "nav_error", "sr", "spl", "nDTW", "SDTW", "CLS"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", GOLDEN)) < 200 * 1024


def test_symbols_in_header_and_binding():
    sigs = _entry_points()
    src = open(os.path.join(ROOT, "include", "hamt.h")).read()
    for name, sig in zip(NAMES, sigs):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(sig), name
    for k, v in (("MAX_GOALS", 256), ("GOALS_EVAL_COLS", 7), ("BACK_EVAL_COLS", 9)):
        assert re.search(rf"#define HAMT_NAV_{k} {v}\b", src), k
    from vln_hamt_amd import _lib, ops
    from vln_hamt_amd.agent import nav_graph
    assert '"nav.hip"' in open(os.path.join(ROOT, "vln_hamt_amd", "csrc", "build.py")).read()
    assert ops.NAV_GOALS_EVAL_COLS == GOALS_COLS and ops.NAV_BACK_EVAL_COLS == BACK_COLS and nav_graph.MAX_GOALS == 256
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES) and lib.hamt_version() == 2
    import inspect
    from vln_hamt_amd.agent import GoalSetEpisodes, NavEpisodes, NavGraphs, ReturnEpisodes, RolloutRecorder
    assert "end_on_miss" in inspect.signature(RolloutRecorder.step).parameters
    assert all(callable(getattr(NavGraphs, k)) for k in ("eval_metrics_cvdn", "eval_metrics_reverie", "eval_metrics_back"))
    assert callable(ReturnEpisodes.midstops) and issubclass(GoalSetEpisodes, NavEpisodes) and issubclass(ReturnEpisodes, NavEpisodes)
    for cls in (GoalSetEpisodes, ReturnEpisodes):                         # the R2R layout first, new fields appended
        assert cls.FIELDS[:len(NavEpisodes.FIELDS)] == NavEpisodes.FIELDS and len(cls.FIELDS) > len(NavEpisodes.FIELDS)
    assert [f[0] for f in NavEpisodes.FIELDS] == ["scan", "cur", "goal", "gt_len", "path_len", "anomalies", "gt", "path", "last_dist", "last_ndtw", "dtw_row"]
    assert {"first_ended", "midstop_at"} <= set(ReturnEpisodes.MUTATED) and "last_dist" in GoalSetEpisodes.MUTATED


def test_new_nav_kernels_use_no_scratch(tmp_path):
    """The cross-compiled gfx950 code objects of the four new kernels: no scratch memory, no spilled registers, no LDS -- resource counts
    read from the ELF notes as tests/test_nav_graph.py reads them"""
    from test_kernel_resources import OBJCOPY, READELF, _code_objects
    from vln_hamt_amd import _lib
    _entry_points()
    if not (os.path.exists(READELF) and os.path.exists(OBJCOPY)):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = []
    for co in _code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or not re.search(KERNELS, name.group(1)):
                continue
            num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
            seen.append(name.group(1))
            print(name.group(1), "vgprs", num("vgpr_count"), "sgprs", num("sgpr_count"))
            assert num("vgpr_spill_count") == 0 and num("sgpr_spill_count") == 0 and num("private_segment_fixed_size") == 0, (name.group(1), blk)
            assert num("group_segment_fixed_size") == 0, name.group(1)
    assert len(seen) == 4 and all(any(k in s for s in seen) for k in ("goals_step", "goals_eval", "back_step", "back_eval")), seen
