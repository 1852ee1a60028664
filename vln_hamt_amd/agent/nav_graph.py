"""The navigation graphs on the device: what a rollout step and an evaluation pass read from the all-pairs shortest distances.

`NavGraphs` holds, for every scan of a connectivity directory, the fp64 distance table and the next-hop table, all scans in one device
arena.  `NavEpisodes` is the per-rollout state over them (current node, ground-truth path, the path walked, the last row of the DTW
matrix, the reward shaping's `last_dist` / `last_ndtw`), filled by ONE packed upload per rollout and advanced by `ops.nav_advance`.
Together with `ops.nav_observe` they replace the reference agent's host loops around a step -- `_teacher_action`
(finetune_src/r2r/agent_cmt.py:199-211), the back-track mask (:342-349), the reward shaping (:407-445) -- and
`NavGraphs.eval_metrics` replaces env.py::eval_metrics / `_eval_item`.  In the Matterport graph a move is deterministic (the new
viewpoint is the chosen candidate's), so none of this needs the simulator.

`GoalSetEpisodes` (CVDN, REVERIE: the goal is a set of viewpoints) and `ReturnEpisodes` (R2R-Back: to a mid-stop, then on to the path's
end) are the same state with a few more fields, advanced by `ops.nav_advance_goals` / `ops.nav_advance_back`;
`NavGraphs.eval_metrics_cvdn` / `eval_metrics_reverie` / `eval_metrics_back` replace those environments' `eval_metrics`.

The tables and all arithmetic on them stay fp64: the fp32 `dist` the agent sees is one rounding of the same double the reference rounds.
"""
from __future__ import annotations

import json
import os
from collections import defaultdict

import numpy as np
import torch

from .. import ops
from ..data.r2r_data import load_nav_graphs

MAX_GT, MAX_PATH = 512, 4096            # HAMT_NAV_MAX_GT / HAMT_NAV_MAX_PATH
MAX_GOALS = 256                         # HAMT_NAV_MAX_GOALS


def _next_hop(w, dist):
    """nxt[x, y] = the neighbour k of x that minimises w[x, k] + dist[k, y] (lowest index on ties), nxt[x, x] = x.  `w`: [n, n] edge
    lengths, inf where there is no edge."""
    n = dist.shape[0]
    nxt = np.empty((n, n), np.int32)
    for x in range(n):
        ks = np.flatnonzero(np.isfinite(w[x]))          # ascending: argmin's first minimum is the lowest index
        nxt[x] = ks[np.argmin(w[x, ks][:, None] + dist[ks], axis=0)] if ks.size else x
        nxt[x, x] = x
    return nxt


class NavGraphs:
    """Per scan (in `scans.txt` order): `nodes[scan]` = the image_ids in connectivity-file order among the nodes that have an edge,
    `dist_host[scan]` fp64 [n, n], `nxt_host[scan]` int32 [n, n].  With a `device`, the arena: `dist` fp64 / `nxt` int32 (scan s at
    element `scan_offset[s]`, n = `scan_n[s]`).  `connectivity_dir`: a directory with `scans.txt`, or several."""

    def __init__(self, connectivity_dir, device=None):
        graphs, dists, where = {}, {}, {}
        for d in ([connectivity_dir] if isinstance(connectivity_dir, (str, os.PathLike)) else connectivity_dir):     # (several directories: their scans in turn)
            g_, d_ = load_nav_graphs(d)
            graphs.update(g_)
            dists.update(d_)
            where.update({s: d for s in g_})
        self.scans = list(graphs)
        self.scan_index = {s: i for i, s in enumerate(self.scans)}
        self.nodes, self._index, self.dist_host, self.nxt_host = {}, {}, {}, {}
        for scan in self.scans:
            adj = graphs[scan]
            with open(os.path.join(where[scan], f"{scan}_connectivity.json")) as f:
                order = [nd["image_id"] for nd in json.load(f) if nd["image_id"] in adj]
            idx = {vp: i for i, vp in enumerate(order)}
            n = len(order)
            dist, w = np.full((n, n), np.inf), np.full((n, n), np.inf)
            for a, row in dists[scan].items():
                for b_, d in row.items():
                    dist[idx[a], idx[b_]] = d
            for a, row in adj.items():
                for b_, d in row.items():
                    w[idx[a], idx[b_]] = d
            self.nodes[scan], self._index[scan], self.dist_host[scan], self.nxt_host[scan] = order, idx, dist, _next_hop(w, dist)
        ns = np.array([len(self.nodes[s]) for s in self.scans], np.int64)
        self.scan_n_host = ns.astype(np.int32)
        self.scan_offset_host = np.concatenate([[0], np.cumsum(ns * ns)[:-1]]).astype(np.int64)
        self.device = None
        if device is not None:
            self.to(device)

    def to(self, device):
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.dist = up(np.concatenate([self.dist_host[s].ravel() for s in self.scans]))
        self.nxt = up(np.concatenate([self.nxt_host[s].ravel() for s in self.scans]))
        self.scan_offset, self.scan_n = up(self.scan_offset_host), up(self.scan_n_host)
        return self

    def node_id(self, scan, viewpoint) -> int:
        return self._index[scan][viewpoint]

    def viewpoint(self, scan, node) -> str:
        return self.nodes[scan][int(node)]

    def pack(self, scans, paths, width=None):
        """(scan int32 [N], nodes int32 [N, width] padded with -1, lengths int32 [N]) of viewpoint-name paths, on the host"""
        lens = np.array([len(p) for p in paths], np.int32)
        out = np.full((len(paths), int(width or max(1, lens.max(initial=1)))), -1, np.int32)
        for i, (s, p) in enumerate(zip(scans, paths)):
            ix = self._index[s]
            out[i, :len(p)] = [ix[v] for v in p]
        return np.array([self.scan_index[s] for s in scans], np.int32), out, lens

    def eval_items(self, scans, paths, gt_paths):
        """env.py::_eval_item of N trajectories (viewpoint names) in one launch: fp64 [N, 11] on the device, columns ops.NAV_EVAL_COLS"""
        for p, g in zip(paths, gt_paths):
            assert g[0] == p[0], "Result trajectories should include the start position"
        sc, pa, pl = self.pack(scans, paths)
        _, gt, gl = self.pack(scans, gt_paths)
        up = lambda a: torch.from_numpy(a).to(self.device, non_blocking=True)
        return ops.nav_eval(self, up(sc), up(pa), up(pl), up(gt), up(gl))

    def eval_metrics(self, preds, gt_trajs):
        """env.py::eval_metrics: `preds` = [{'instr_id', 'trajectory': [(viewpoint, ...), ...]}], `gt_trajs` = {instr_id: (scan, path)}.
        Returns the reference's (avg_metrics, metrics): the same keys, the same `* 100` scalings."""
        ids = [item["instr_id"] for item in preds]
        scans = [gt_trajs[i][0] for i in ids]
        out = self.eval_items(scans, [[x[0] for x in item["trajectory"]] for item in preds], [gt_trajs[i][1] for i in ids]).cpu().numpy()
        metrics = defaultdict(list)
        for c, k in enumerate(ops.NAV_EVAL_COLS):
            metrics[k] = out[:, c].astype(np.int64).tolist() if k == "trajectory_steps" else out[:, c].tolist()
        metrics["instr_id"] = ids
        mean = lambda k: np.mean(metrics[k])
        avg_metrics = {"steps": mean("trajectory_steps"), "lengths": mean("trajectory_lengths"), "nav_error": mean("nav_error"),
                       "oracle_error": mean("oracle_error"), "sr": mean("success") * 100, "oracle_sr": mean("oracle_success") * 100,
                       "spl": mean("spl") * 100, "nDTW": mean("nDTW") * 100, "SDTW": mean("SDTW") * 100, "CLS": mean("CLS") * 100}
        return avg_metrics, metrics

    def _up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True)

    @staticmethod
    def _metric_lists(out, cols):
        metrics = defaultdict(list)
        for c, k in enumerate(cols):
            metrics[k] = out[:, c].astype(np.int64).tolist() if k == "trajectory_steps" else out[:, c].tolist()
        return metrics

    def eval_goal_items(self, scans, paths, goal_sets, gt_paths=None):
        """cvdn/env.py::_eval_item (no `gt_paths`) or the navigation part of reverie/env.py::_eval_item of N trajectories in one launch:
        fp64 [N, 7] on the device, columns ops.NAV_GOALS_EVAL_COLS.  A goal set is taken as a set: duplicates drop out."""
        sets = [list(dict.fromkeys(g)) for g in goal_sets]
        sc, pa, pl = self.pack(scans, paths)
        _, go, gl = self.pack(scans, sets)
        gt = gtl = None
        if gt_paths is not None:
            for p, g in zip(paths, gt_paths):
                assert g[0] == p[0], "Result trajectories should include the start position"
            _, gt, gtl = self.pack(scans, gt_paths)
            gt, gtl = self._up(gt), self._up(gtl)
        return ops.nav_eval_goals(self, self._up(sc), self._up(pa), self._up(pl), self._up(go), self._up(gl), gt, gtl)

    def eval_metrics_cvdn(self, preds, gt_trajs):
        """cvdn/env.py::eval_metrics: `gt_trajs` = {instr_id: (scan, end_panos)}.  Returns the reference's (avg_metrics, metrics)."""
        ids = [item["instr_id"] for item in preds]
        scans = [gt_trajs[i][0] for i in ids]
        out = self.eval_goal_items(scans, [[x[0] for x in item["trajectory"]] for item in preds], [gt_trajs[i][1] for i in ids]).cpu().numpy()
        metrics = self._metric_lists(out[:, :6], ops.NAV_GOALS_EVAL_COLS[:6])
        metrics["instr_id"] = ids
        mean = lambda k: np.mean(metrics[k])
        avg_metrics = {"steps": mean("trajectory_steps"), "lengths": mean("trajectory_lengths"), "sr": mean("success") * 100,
                       "oracle_sr": mean("oracle_success") * 100, "spl": mean("spl") * 100, "gp": mean("gp")}
        return avg_metrics, metrics

    def eval_metrics_reverie(self, preds, gt_trajs, obj2viewpoint):
        """reverie/env.py::ReverieNavRefBatch.eval_metrics: `preds` items carry 'predObjId', `gt_trajs` = {instr_id: (scan, path, objId)},
        `obj2viewpoint` = {'scan_objid': [viewpoints the object is visible from]}.  `rgs` compares object ids on the host; `rgspl` is
        rgs times the device's spl_ratio."""
        ids = [item["instr_id"] for item in preds]
        scans = [gt_trajs[i][0] for i in ids]
        goal_sets = [obj2viewpoint["%s_%s" % (gt_trajs[i][0], str(gt_trajs[i][2]))] for i in ids]
        for i, g in zip(ids, goal_sets):
            assert len(g) > 0, "%s_%s" % (gt_trajs[i][0], str(gt_trajs[i][2]))
        out = self.eval_goal_items(scans, [[x[0] for x in item["trajectory"]] for item in preds], goal_sets, [gt_trajs[i][1] for i in ids]).cpu().numpy()
        metrics = self._metric_lists(out[:, :5], ops.NAV_GOALS_EVAL_COLS[:5])
        metrics["rgs"] = [float(str(item["predObjId"]) == str(gt_trajs[i][2])) for item, i in zip(preds, ids)]
        metrics["rgspl"] = (np.asarray(metrics["rgs"]) * out[:, 6]).tolist()
        metrics["instr_id"] = ids
        mean = lambda k: np.mean(metrics[k])
        avg_metrics = {"steps": mean("trajectory_steps"), "lengths": mean("trajectory_lengths"), "sr": mean("success") * 100,
                       "oracle_sr": mean("oracle_success") * 100, "spl": mean("spl") * 100, "rgs": mean("rgs") * 100, "rgspl": mean("rgspl") * 100}
        return avg_metrics, metrics

    def eval_metrics_back(self, preds, gt_trajs, gt_midstops):
        """env.py::R2RBackBatch.eval_metrics: `preds` items carry 'midstop' (a viewpoint or None), `gt_trajs` = {instr_id: (scan, path)},
        `gt_midstops` = {instr_id: viewpoint}."""
        ids = [item["instr_id"] for item in preds]
        scans = [gt_trajs[i][0] for i in ids]
        paths, gts = [[x[0] for x in item["trajectory"]] for item in preds], [gt_trajs[i][1] for i in ids]
        for p, g in zip(paths, gts):
            assert g[0] == p[0], "Result trajectories should include the start position"
        sc, pa, pl = self.pack(scans, paths)
        _, gt, gl = self.pack(scans, gts)
        mid = np.array([-1 if item["midstop"] is None else self.node_id(s, item["midstop"]) for s, item in zip(scans, preds)], np.int32)
        gmid = np.array([self.node_id(s, gt_midstops[i]) for s, i in zip(scans, ids)], np.int32)
        out = ops.nav_eval_back(self, self._up(sc), self._up(pa), self._up(pl), self._up(gt), self._up(gl), self._up(mid), self._up(gmid)).cpu().numpy()
        metrics = self._metric_lists(out, ops.NAV_BACK_EVAL_COLS)
        metrics["success"] = out[:, 3].astype(np.int64).tolist()           # (an int in the reference)
        metrics["instr_id"] = ids
        mean = lambda k: np.mean(metrics[k])
        avg_metrics = {"steps": mean("trajectory_steps"), "lengths": mean("trajectory_lengths"), "nav_error": mean("nav_error"),
                       "sr": mean("success") * 100, "spl": mean("spl") * 100, "nDTW": mean("nDTW") * 100, "SDTW": mean("SDTW") * 100,
                       "CLS": mean("CLS") * 100}
        return avg_metrics, metrics


class NavEpisodes:
    """The B episodes of one rollout over `graphs` (on the device).  One uint8 arena holds every field, so `reset` is one upload from
    a pinned mirror:
      scan, cur, goal, gt_len, path_len int32 [B]; anomalies int32 [2] (teacher look-ups / moves the reference would have failed on);
      gt int32 [B, G_max]; path int32 [B, T_max + 1] (every node stood on); last_dist, last_ndtw fp32 [B] (agent_cmt.py:284-289);
      dtw_row fp64 [B, G_max + 1] (the last row of cal_dtw's matrix for path against gt).
    `max_gt` <= 512 (HAMT_NAV_MAX_GT); a longer ground truth is refused."""

    FIELDS = (("scan", np.int32, "B"), ("cur", np.int32, "B"), ("goal", np.int32, "B"), ("gt_len", np.int32, "B"), ("path_len", np.int32, "B"),
              ("anomalies", np.int32, "2"), ("gt", np.int32, "BG"), ("path", np.int32, "BP"), ("last_dist", np.float32, "B"),
              ("last_ndtw", np.float32, "B"), ("dtw_row", np.float64, "BR"))
    MUTATED = ("cur", "path", "path_len", "dtw_row", "last_dist", "last_ndtw", "anomalies")
    KIND = "r2r"                        # which advance launch RolloutRecorder.step makes

    def __init__(self, graphs: NavGraphs, max_steps: int, batch_size: int, max_gt: int = 64, max_goals: int = 1):
        if graphs.device is None:
            raise ops.L.HamtError("NavEpisodes: the graphs are not on a device (NavGraphs(dir, device=...)); there is no CPU path")
        self.graphs, self.T_max, self.B, self.G_max = graphs, int(max_steps), int(batch_size), int(max_gt)
        self.path_cap = self.T_max + 1
        if not 0 < self.G_max <= MAX_GT or self.path_cap > MAX_PATH:
            raise ops.L.HamtError(f"NavEpisodes: max_gt {self.G_max} / max_steps {self.T_max} outside the supported (0, {MAX_GT}] / [0, {MAX_PATH})")
        self.E_max = int(max_goals)
        if not 0 < self.E_max <= MAX_GOALS:
            raise ops.L.HamtError(f"NavEpisodes: max_goals {self.E_max} outside the supported (0, {MAX_GOALS}]")
        B = self.B
        dims = {"B": (B,), "2": (2,), "BG": (B, self.G_max), "BP": (B, self.path_cap), "BR": (B, self.G_max + 1), "BE": (B, self.E_max)}
        layout, off = [], 0
        for name, dt, d in self.FIELDS:
            nbytes = int(np.prod(dims[d])) * np.dtype(dt).itemsize
            layout.append((name, dt, dims[d], off, nbytes))
            off += (nbytes + 7) // 8 * 8
        self.arena = torch.zeros(off, dtype=torch.uint8, device=graphs.device)
        self._host = torch.zeros(off, dtype=torch.uint8).pin_memory()
        self._event = torch.cuda.Event()
        self._np = {}
        for name, dt, shape, o, nbytes in layout:
            tdt = torch.from_numpy(np.empty(0, dt)).dtype
            setattr(self, name, self.arena[o:o + nbytes].view(tdt).view(*shape))
            self._np[name] = self._host.numpy()[o:o + nbytes].view(dt).reshape(shape)

    def reset(self, scans, start_viewpoints, gt_paths):
        """New rollout: episode b stands on start_viewpoints[b] of scans[b] and is scored against gt_paths[b] (viewpoint names)."""
        self._fill(scans, start_viewpoints, gt_paths)
        return self._upload()

    def _fill(self, scans, start_viewpoints, gt_paths):
        g, h = self.graphs, self._np
        assert len(scans) == len(start_viewpoints) == len(gt_paths) == self.B, (len(scans), self.B)
        if max(len(p) for p in gt_paths) > self.G_max or min(len(p) for p in gt_paths) < 1:
            raise ops.L.HamtError(f"NavEpisodes.reset: ground-truth lengths must lie in [1, max_gt = {self.G_max}]")
        self._event.synchronize()                            # (the last upload has left the pinned mirror)
        h["scan"][:], h["gt"][:], h["gt_len"][:] = g.pack(scans, gt_paths, self.G_max)
        h["path"][:] = -1
        h["path_len"][:] = 1
        h["anomalies"][:] = 0
        h["dtw_row"][:] = np.inf
        for b, (scan, vp) in enumerate(zip(scans, start_viewpoints)):
            G, start, dist = int(h["gt_len"][b]), g.node_id(scan, vp), g.dist_host[scan]
            gt = h["gt"][b, :G]
            h["cur"][b] = h["path"][b, 0] = start
            h["goal"][b] = gt[-1]
            h["dtw_row"][b, 1:G + 1] = np.cumsum(dist[start, gt])          # (cal_dtw's first row: only `left` is finite)
            h["last_dist"][b] = dist[start, gt[-1]]
            h["last_ndtw"][b] = np.exp(-h["dtw_row"][b, G] / (3.0 * G))

    def _upload(self):
        self.arena.copy_(self._host, non_blocking=True)
        self._event.record()
        return self

    def state_tensors(self):
        """everything a step mutates (graph.GraphedInference's `state`)"""
        return tuple(getattr(self, k) for k in self.MUTATED)


class GoalSetEpisodes(NavEpisodes):
    """Episodes whose goal is a SET of viewpoints (CVDN's `end_panos`, REVERIE's viewpoints the object is visible from): NavEpisodes'
    fields, then goals int32 [B, E_max] and goal_len int32 [B].  `last_dist` is the fp32 minimum over the set (cvdn/agent.py:52-55), 0
    for an empty set; there is no nDTW term, so `dtw_row` / `last_ndtw` only keep their initial values.  Advanced by
    `ops.nav_advance_goals`.  `max_goals` <= 256 (HAMT_NAV_MAX_GOALS)."""

    FIELDS = NavEpisodes.FIELDS + (("goals", np.int32, "BE"), ("goal_len", np.int32, "B"))
    MUTATED = ("cur", "path", "path_len", "last_dist", "anomalies")
    KIND = "goals"

    def __init__(self, graphs: NavGraphs, max_steps: int, batch_size: int, max_gt: int = 64, max_goals: int = 64):
        super().__init__(graphs, max_steps, batch_size, max_gt=max_gt, max_goals=max_goals)

    def reset(self, scans, start_viewpoints, gt_paths, goal_sets):
        """`gt_paths[b]` feeds the teacher of `ops.nav_observe` (the host picks it: the shortest path to a drawn end_pano, or the player's
        path); `goal_sets[b]` is the list of goal viewpoints, possibly empty, duplicates allowed."""
        assert len(goal_sets) == self.B, (len(goal_sets), self.B)
        if max((len(e) for e in goal_sets), default=0) > self.E_max:
            raise ops.L.HamtError(f"GoalSetEpisodes.reset: a goal set larger than max_goals = {self.E_max}")
        self._fill(scans, start_viewpoints, gt_paths)
        g, h = self.graphs, self._np
        _, h["goals"][:], h["goal_len"][:] = g.pack(scans, goal_sets, self.E_max)
        for b, scan in enumerate(scans):
            E = int(h["goal_len"][b])
            h["last_dist"][b] = g.dist_host[scan][h["cur"][b], h["goals"][b, :E]].min() if E else 0.0
        return self._upload()


class ReturnEpisodes(NavEpisodes):
    """Return trips (R2R-Back): the ground-truth path leads to `midstop` and on to its end.  NavEpisodes' fields, then midstop int32 [B]
    (the ground truth's), midstop_at int32 [B] (where the agent made its first STOP, -1 = not yet) and first_ended uint8 [B].
    `last_dist` starts as the distance to the mid-stop (agent_r2rback.py:106-107).  Advanced by `ops.nav_advance_back`."""

    FIELDS = NavEpisodes.FIELDS + (("midstop", np.int32, "B"), ("midstop_at", np.int32, "B"), ("first_ended", np.uint8, "B"))
    MUTATED = NavEpisodes.MUTATED + ("first_ended", "midstop_at")
    KIND = "back"

    def reset(self, scans, start_viewpoints, gt_paths, midstops):
        assert len(midstops) == self.B, (len(midstops), self.B)
        self._fill(scans, start_viewpoints, gt_paths)
        g, h = self.graphs, self._np
        h["midstop_at"][:] = -1
        h["first_ended"][:] = 0
        for b, (scan, vp) in enumerate(zip(scans, midstops)):
            h["midstop"][b] = g.node_id(scan, vp)
            h["last_dist"][b] = g.dist_host[scan][h["cur"][b], h["midstop"][b]]
        self._scans = list(scans)
        return self._upload()

    def midstops(self):
        """traj['midstop'] of every episode: the viewpoint of its first STOP, or None (one blocking read of midstop_at)"""
        return [None if v < 0 else self.graphs.viewpoint(s, v) for s, v in zip(self._scans, self.midstop_at.cpu().tolist())]
