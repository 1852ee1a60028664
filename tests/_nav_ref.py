"""A numpy restatement of csrc/nav.hip and of RolloutRecorder's `nav=` step (what include/hamt.h says of hamt_nav_observe /
hamt_nav_advance / hamt_nav_eval), serial and fp64: tests/test_nav_graph.py holds it to the reference's own statements
(tests/golden/nav_reward.npz), the GPU tests use it for the shapes the golden does not hold."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONNECTIVITY = [os.path.join(GOLDEN, "r2r_tiny"), os.path.join(GOLDEN, "nav_tiny")]         # scanA, scanB, scanC: the golden's scan order
MODES = ("path_step", "path_index", "shortest")
COLS = ("nav_error", "oracle_error", "trajectory_steps", "trajectory_lengths", "success", "spl", "oracle_success", "DTW", "nDTW", "SDTW", "CLS")
f32 = np.float32

# the bounds of the issue: fp32 `dist` exact; ndtw two fp32 ulps at 1; reward one rounding of an fp64 result (|reward| <= 4);
# metrics under ~1e3 fp64 operations in any order
TOL_NDTW, TOL_REWARD, TOL_METRIC = 2.4e-7, 1e-6, 1e-12


def golden_tables(store):
    """[(dist fp64 [n, n], nxt int32 [n, n])] per scan, from the golden's networkx tables"""
    return [(store[f"graph/{s}/dist"], store[f"graph/{s}/next"].astype(np.int32)) for s in store["meta/scans"]]


def host_tables(graphs):
    return [(graphs.dist_host[s], graphs.nxt_host[s]) for s in graphs.scans]


def dtw_row(above, cost):
    """the next row of cal_dtw's matrix: above [G + 1] (above[0] = 0 for the first row, inf after), cost [G]"""
    row = np.full(len(cost) + 1, np.inf)
    for j in range(1, len(cost) + 1):
        row[j] = cost[j - 1] + min(above[j], row[j - 1], above[j - 1])
    return row


class EpisodesRef:
    """NavEpisodes on the host: `tables` per scan, episode b in scan[b] standing on start[b], scored against gt[b][:gt_len[b]]"""

    def __init__(self, tables, scan, start, gt, gt_len):
        self.tables, self.scan, self.B = tables, [int(s) for s in scan], len(scan)
        self.gt = [[int(v) for v in gt[b][:gt_len[b]]] for b in range(self.B)]
        self.cur = [int(v) for v in start]
        self.path = [[c] for c in self.cur]
        self.anomalies = [0, 0]
        self.row, self.last_dist, self.last_ndtw = [], np.zeros(self.B, f32), np.zeros(self.B, f32)
        for b in range(self.B):
            dist = self.tables[self.scan[b]][0]
            first = np.full(len(self.gt[b]) + 1, np.inf)
            first[0] = 0.0
            self.row.append(dtw_row(first, dist[self.cur[b], self.gt[b]]))
            self.last_dist[b] = dist[self.cur[b], self.gt[b][-1]]
            self.last_ndtw[b] = self.ndtw(b)

    def ndtw(self, b):
        G = len(self.gt[b])
        return f32(np.exp(-self.row[b][G] / (3.0 * G)))

    def observe(self, t, cand_node, cand_len, ended, mode, ignoreid=-100):
        """-> (target int64 [B], bt_mask uint8 [B, V]); counts anomalies[0]"""
        B, V = cand_node.shape
        target, bt = np.full(B, ignoreid, np.int64), np.zeros((B, V), np.uint8)
        for b in range(B):
            here, gt, nav = self.cur[b], self.gt[b], [int(v) for v in cand_node[b, :max(int(cand_len[b]) - 1, 0)]]
            for c, node in enumerate(nav):
                bt[b, c] = node >= 0 and node in self.path[b]
            if ended[b]:
                continue
            if mode == "path_step":
                tv = gt[t + 1] if t < len(gt) - 1 else here
            elif mode == "path_index":
                tv = None if here not in gt else (here if gt.index(here) == len(gt) - 1 else gt[gt.index(here) + 1])
            else:
                tv = int(self.tables[self.scan[b]][1][here, gt[-1]])
            if tv is not None and tv in nav:
                target[b] = nav.index(tv)
            elif tv == here:
                target[b] = int(cand_len[b]) - 1
            else:
                self.anomalies[0] += 1
        return target, bt

    def advance(self, cand_node, env_action, mask):
        """-> (reward, dist, ndtw) fp32 [B]; moves the episodes"""
        B = self.B
        reward, dist_, ndtw_ = np.zeros(B, f32), np.zeros(B, f32), np.zeros(B, f32)
        for b in range(B):
            dist, a = self.tables[self.scan[b]][0], int(env_action[b])
            if a >= 0:
                self.cur[b] = int(cand_node[b, a])
                self.path[b].append(self.cur[b])
                above = self.row[b]
                self.row[b] = dtw_row(above, dist[self.cur[b], self.gt[b]])
            d, nd, ld, ln = f32(dist[self.cur[b], self.gt[b][-1]]), self.ndtw(b), self.last_dist[b], self.last_ndtw[b]
            r = f32(0.0)
            if mask[b] != 0:
                if a < 0:
                    r = f32(2.0) + nd * f32(2.0) if d < f32(3.0) else f32(-2.0)
                else:
                    gain, shaped = -(d - ld), nd - ln
                    if gain > 0:
                        r = f32(1.0) + shaped
                    elif gain < 0:
                        r = f32(-1.0) + shaped
                    else:
                        r = shaped
                        self.anomalies[1] += 1
                    if ld <= f32(1.0) and d - ld > 0:
                        r = r - (f32(1.0) - ld) * f32(2.0)
            reward[b], dist_[b], ndtw_[b] = r, d, nd
            self.last_dist[b], self.last_ndtw[b] = d, nd
        return reward, dist_, ndtw_


def eval_ref(dist, path, gt):
    """env.py::_eval_item's eleven scores of one trajectory (node ids) in COLS order"""
    path, gt = [int(v) for v in path], [int(v) for v in gt]
    goal = gt[-1]
    nav_error = dist[path[-1], goal]
    oracle_error = min(dist[v, goal] for v in path)
    plen = float(np.sum([dist[a, b] for a, b in zip(path[:-1], path[1:])]))
    glen = float(np.sum([dist[a, b] for a, b in zip(gt[:-1], gt[1:])]))
    success = float(nav_error < 3.0)
    row = np.full(len(gt) + 1, np.inf)
    row[0] = 0.0
    for v in path:
        row = dtw_row(row, dist[v, gt])
    dtw = row[len(gt)]
    ndtw = np.exp(-dtw / (3.0 * len(gt)))
    cover = np.mean([np.exp(-min(dist[u, v] for v in path) / 3.0) for u in gt])
    expected = cover * glen
    with np.errstate(invalid="ignore"):
        score = np.float64(expected) / (expected + np.abs(expected - plen))
    return np.array([nav_error, oracle_error, len(path) - 1, plen, success, success * glen / max(plen, glen, 0.01), float(oracle_error < 3.0),
                     dtw, ndtw, success * ndtw, cover * score], np.float64)


def close_metrics(got, want, what=""):
    """`got` against `want` [N, 11]: NaNs in the same places, the rest within TOL_METRIC relative; returns the largest error seen"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want)))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    err[got[ok] == want[ok]] = 0.0
    worst = float(err.max()) if err.size else 0.0
    print(f"[{what}] metrics: max relative error {worst:.3e}")
    assert worst <= TOL_METRIC, (what, worst)
    return worst


def random_walk(rng, nbrs, start, n, revisit=0.3):
    p = [int(start)]
    while len(p) < n:
        nb = nbrs[p[-1]]
        fresh = [v for v in nb if v not in p]
        pool = fresh if fresh and rng.random() > revisit else nb
        p.append(int(pool[int(rng.integers(len(pool)))]))
    return p


def neighbours(graphs, scan):
    """local neighbour lists of `scan` (a NavGraphs): x's neighbours are the y with nxt[x, y] == y, y != x ... and an edge"""
    d, nx_ = graphs.dist_host[scan], graphs.nxt_host[scan]
    n = d.shape[0]
    return [[y for y in range(n) if y != x and nx_[x, y] == y] for x in range(n)]
