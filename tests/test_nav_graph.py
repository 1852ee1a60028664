"""Not gpu: the navigation graphs on the device (vln_hamt_amd/csrc/nav.hip, ops.nav_observe / nav_advance / nav_eval, agent.NavGraphs /
NavEpisodes) -- the numpy restatement the GPU tests compare against reproduces the REFERENCE's own statements
(tests/golden/nav_reward.npz, tools/gen_nav_golden.py), the host tables equal networkx's, the new entry points are declared and bound,
and the cross-compiled kernels use no scratch memory."""
import os
import re
import subprocess

import numpy as np
import pytest

from _nav_ref import COLS, CONNECTIVITY, MODES, TOL_NDTW, TOL_REWARD, EpisodesRef, close_metrics, eval_ref, golden_tables
from _util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hamt_nav_observe", "hamt_nav_advance", "hamt_nav_eval")


def _entry_points():
    from vln_hamt_amd import _lib
    return [_lib.SIGNATURES[n] for n in NAMES]


def golden_rollout(store, mode, step):
    """drive `step(t, cand_node, cand_len, ended, a_t) -> (target, bt_mask, reward, dist, ndtw)` over the golden's scripted rollout
    and hold every answer to the reference's, at the issue's bounds"""
    g = lambda k: store["roll/" + k]
    T, B = g("cand_len").shape
    for t in range(T):
        target, bt, reward, dist, ndtw = step(t, g("cand")[t], g("cand_len")[t], g("ended")[t], g("a_t")[t])
        assert np.array_equal(target, g(f"target/{mode}")[t]), (mode, t, target, g(f"target/{mode}")[t])
        assert np.array_equal(bt, g("bt_mask")[t]), (t, bt, g("bt_mask")[t])
        assert np.array_equal(dist, g("dist")[t]), (t, dist, g("dist")[t])                      # fp32: exact
        e_n, e_r = float(np.abs(ndtw.astype(np.float64) - g("ndtw")[t]).max()), float(np.abs(reward.astype(np.float64) - g("reward")[t]).max())
        print(f"[{mode} step {t}] max|d ndtw| {e_n:.3e}  max|d reward| {e_r:.3e}")
        assert e_n <= TOL_NDTW and e_r <= TOL_REWARD, (t, e_n, e_r)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_reproduces_the_reference_rollout(mode):
    """tests/_nav_ref.py against the reference's `_teacher_action` over `_teacher_path_action`, its back-track block, its init block and
    its reward block on the scripted rollout: integers, masks and the fp32 distance exact, ndtw within two fp32 ulps at 1, the reward
    within 1e-6; the anomaly counter is the number of places the reference's assert fired."""
    _entry_points()
    store = load_npz("nav_reward.npz")
    g = lambda k: store["roll/" + k]
    ep = EpisodesRef(golden_tables(store), g("scan"), g("start"), g("gt"), g("gt_len"))
    assert np.array_equal(ep.last_dist, g("init_last_dist")) and float(np.abs(ep.last_ndtw - g("init_last_ndtw")).max()) <= TOL_NDTW
    ignoreid = int(store["meta/ignoreid"])

    def step(t, cand, cand_len, ended, a_t):
        assert ep.cur == g("cur")[t].tolist()
        target, bt = ep.observe(t, cand, cand_len, ended, mode, ignoreid)
        env = np.where((a_t == cand_len - 1) | ended, -1, a_t).astype(np.int32)               # (agent_cmt.py:372-375, ops.policy_step)
        assert np.array_equal(env, g("env_action")[t])
        reward, dist, ndtw = ep.advance(cand, env, (~ended).astype(np.float32))
        return target, bt, reward, dist, ndtw
    golden_rollout(store, mode, step)
    assert ep.anomalies == [int(g(f"assert/{mode}").sum()), 0], ep.anomalies
    for b in range(ep.B):
        assert ep.path[b] == g("path")[b, :g("path_len")[b]].tolist()


def test_restatement_reproduces_the_reference_metrics():
    """eval_ref against env.py::_eval_item (through eval_metrics) for the golden's 42 trajectories: 1e-12 relative, NaN where the
    reference has NaN"""
    _entry_points()
    store = load_npz("nav_reward.npz")
    tables = golden_tables(store)
    e = lambda k: store["eval/" + k]
    got = np.stack([eval_ref(tables[e("scan")[i]][0], e("path")[i, :e("path_len")[i]], e("gt")[i, :e("gt_len")[i]]) for i in range(len(e("scan")))])
    close_metrics(got, e("metrics"), "restatement vs reference")
    assert np.array_equal(got[:, 2], e("metrics")[:, 2]) and np.array_equal(got[:, 4], e("metrics")[:, 4])      # steps and success: exact


def test_host_tables_equal_networkx():
    """NavGraphs' host tables (data.r2r_data's Dijkstra, the next-hop rule of agent/nav_graph.py) against the golden's networkx
    all_pairs_dijkstra distances and path[1], in connectivity-file node order.  Bound 1e-12 relative; largest seen here: 0 (both add
    the same edge lengths along the same shortest path in the same order)."""
    _entry_points()
    from vln_hamt_amd.agent import NavGraphs
    store = load_npz("nav_reward.npz")
    graphs = NavGraphs(CONNECTIVITY)
    assert graphs.scans == store["meta/scans"].tolist() and graphs.device is None
    worst = 0.0
    for i, scan in enumerate(graphs.scans):
        want = store[f"graph/{scan}/dist"]
        assert graphs.nodes[scan] == store[f"graph/{scan}/nodes"].tolist()
        assert graphs.dist_host[scan].dtype == np.float64 and graphs.dist_host[scan].shape == want.shape
        worst = max(worst, float((np.abs(graphs.dist_host[scan] - want) / np.maximum(want, 1e-300)).max()))
        assert np.array_equal(graphs.nxt_host[scan], store[f"graph/{scan}/next"]), scan
        assert graphs.scan_n_host[i] == len(want) and graphs.scan_offset_host[i] == sum(int(n) ** 2 for n in graphs.scan_n_host[:i])
        for k, vp in enumerate(graphs.nodes[scan]):
            assert graphs.node_id(scan, vp) == k and graphs.viewpoint(scan, k) == vp
    print(f"[host tables] max relative difference to networkx {worst:.3e}; smallest next-hop gap {float(store['meta/next_hop_gap']):.3e}")
    assert worst <= 1e-12
    assert float(store["meta/next_hop_gap"]) > 1e-6                       # (no tie in the fixtures: the lowest-index rule is not what decides)


def test_dijkstra_result_is_unchanged():
    """the tables are built from data.r2r_data.load_nav_graphs as it stands (tests/golden/r2r_data.npz pins it elsewhere): same keys"""
    _entry_points()
    from vln_hamt_amd.agent import NavGraphs
    from vln_hamt_amd.data.r2r_data import load_nav_graphs
    _, dists = load_nav_graphs(CONNECTIVITY[0])
    graphs = NavGraphs(CONNECTIVITY[0])
    for scan, tab in dists.items():
        for a, row in tab.items():
            for b, d in row.items():
                assert graphs.dist_host[scan][graphs.node_id(scan, a), graphs.node_id(scan, b)] == d


def test_golden_holds_the_corners_the_issue_names():
    _entry_points()
    store = load_npz("nav_reward.npz")
    g, e = (lambda k: store["roll/" + k]), (lambda k: store["eval/" + k])
    T, B = g("cand_len").shape
    assert (B, T) == (6, 7) and set(g("scan").tolist()) == {0, 1, 2}                                      # all three scans in one batch
    assert len(set(g("cand_len").flatten().tolist())) > 3                                                 # ragged
    r, m, env, d = g("reward"), g("mask"), g("env_action"), g("dist")
    last = np.concatenate([g("init_last_dist")[None], d[:-1]])
    live = m == 1
    assert (live & (env == -1) & (d < 3.0) & (r >= 2.0)).any()                                            # a correct stop
    assert (live & (env == -1) & (d >= 3.0) & (r == -2.0)).any()                                          # a wrong stop
    assert (live & (env >= 0) & (d < last) & (r > 0)).any() and (live & (env >= 0) & (d > last) & (r < 0)).any()     # closer, away
    assert (live & (env >= 0) & (last <= 1.0) & (d > last) & (r < -1.5)).any()                            # the miss-the-target penalty
    assert (~live).any() and (r[~live] == 0).all() and (env[~live] == -1).all()                           # steps after the end
    assert not ((env >= 0) & (d == last)).any()                                                           # no move leaves the fp32 distance unchanged
    assert g("bt_mask").sum() >= 6 and (g("path_len") > np.array([len(set(p[:n])) for p, n in zip(g("path"), g("path_len"))])).any()     # revisits
    assert not g("final_ended").all() and g("final_ended").any()
    assert g("gt_len").max() > 64 and g("gt_len").min() == 1                                              # a gt across 64 lanes; t >= gt_len - 1 at once
    assert g("assert/path_step").any() and g("assert/path_index").any() and not g("assert/shortest").any()
    for mode in MODES:                                                                                    # the modes really differ
        assert (g(f"target/{mode}")[g("ended")] == int(store["meta/ignoreid"])).all()
    assert not np.array_equal(g("target/path_step"), g("target/path_index")) and not np.array_equal(g("target/path_index"), g("target/shortest"))
    pl, gl = e("path_len")[e("scan") == 2], e("gt_len")[e("scan") == 2]
    assert {1, 2, 63, 64, 65, 130} <= set(pl.tolist()) and {64, 65, 130} <= set(gl.tolist())
    assert 38 <= len(e("scan")) <= 48
    mt = e("metrics")
    assert np.isnan(mt[:, 10]).sum() == 1 and np.isnan(mt).sum() == 1                                     # the NaN corner: CLS only, once
    i = int(np.argwhere(np.isnan(mt[:, 10]))[0, 0])
    assert e("path_len")[i] == 1 and e("gt_len")[i] == 1
    glen = np.array([sum(store[f"graph/{store['meta/scans'][s]}/dist"][a, b] for a, b in zip(p[:n - 1], p[1:n]))
                     for s, p, n in zip(e("scan"), e("gt"), e("gt_len"))])
    assert (mt[:, 3] < glen - 1e-9).any() and (mt[:, 3] > glen + 1e-9).any()                              # trajectory_lengths on both sides of gt_lengths
    assert (mt[:, 4] == 1).any() and (mt[:, 4] == 0).any()
    assert any(len(set(p[:n].tolist())) < n for p, n in zip(e("path"), e("path_len")))                    # revisits
    assert e("avg_keys").tolist() == ["steps", "lengths", "nav_error", "oracle_error", "sr", "oracle_sr", "spl", "nDTW", "SDTW", "CLS"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "nav_reward.npz")) < 200 * 1024


def test_symbols_in_header_and_binding():
    sigs = _entry_points()
    src = open(os.path.join(ROOT, "include", "hamt.h")).read()
    for name, sig in zip(NAMES, sigs):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(sig), name
    for k, v in (("PATH_STEP", 0), ("PATH_INDEX", 1), ("SHORTEST", 2), ("MAX_GT", 512), ("EVAL_COLS", 11)):
        assert re.search(rf"#define HAMT_NAV_{k} {v}\b", src), k
    from vln_hamt_amd import _lib, ops
    from vln_hamt_amd.agent import nav_graph
    assert '"nav.hip"' in open(os.path.join(ROOT, "vln_hamt_amd", "csrc", "build.py")).read()
    assert ops.NAV_TEACHER_MODES == {"path_step": 0, "path_index": 1, "shortest": 2} and ops.NAV_EVAL_COLS == COLS
    macro = lambda k: int(re.search(rf"#define HAMT_NAV_{k} (\d+)", src).group(1))
    assert (nav_graph.MAX_GT, nav_graph.MAX_PATH) == (macro("MAX_GT"), macro("MAX_PATH")) and nav_graph.MAX_GT >= 512
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES) and lib.hamt_version() == 2
    from vln_hamt_amd.agent import NavEpisodes, NavGraphs, RolloutRecorder
    import inspect
    assert {"nav", "cand_nodes", "teacher_mode"} <= set(inspect.signature(RolloutRecorder.step).parameters)
    assert callable(NavGraphs.eval_metrics) and callable(NavEpisodes.reset) and callable(NavEpisodes.state_tensors)


def test_nav_kernels_use_no_scratch(tmp_path):
    """The cross-compiled gfx950 code object of nav.hip: no scratch memory, no spilled registers, no LDS (read as
    tests/test_policy_step.py does)."""
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
            if not name or not re.search(r"nav_(observe|advance|eval)_kernel", name.group(1)):
                continue
            num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
            seen.append(name.group(1))
            print(name.group(1), "vgprs", num("vgpr_count"), "sgprs", num("sgpr_count"))
            assert num("vgpr_spill_count") == 0 and num("sgpr_spill_count") == 0 and num("private_segment_fixed_size") == 0, (name.group(1), blk)
            assert num("group_segment_fixed_size") == 0, name.group(1)                         # wave shuffles only: no LDS
    assert len(seen) == 3 and all(any(k in s for s in seen) for k in ("observe", "advance", "eval")), seen
