"""A numpy restatement of the goal-set and return-trip kernels of csrc/nav.hip (what include/hamt.h says of hamt_nav_advance_goals /
hamt_nav_advance_back / hamt_nav_eval_goals / hamt_nav_eval_back), serial and fp64: tests/test_nav_tasks.py holds it to the reference's
own statements (tests/golden/nav_tasks.npz), the GPU tests use it for the shapes the golden does not hold.  The bounds are those of
tests/_nav_ref.py."""
import numpy as np

from _nav_ref import EpisodesRef, dtw_row, f32

GOALS_COLS = ("trajectory_steps", "trajectory_lengths", "success", "oracle_success", "spl", "gp", "spl_ratio")
BACK_COLS = ("nav_error", "trajectory_steps", "trajectory_lengths", "success", "spl", "DTW", "nDTW", "SDTW", "CLS")


class GoalSetRef(EpisodesRef):
    """GoalSetEpisodes on the host: EpisodesRef (its `observe` is the teacher's) with a goal list per episode"""

    def __init__(self, tables, scan, start, gt, gt_len, goals, goal_len):
        super().__init__(tables, scan, start, gt, gt_len)
        self.goals = [[int(v) for v in goals[b][:goal_len[b]]] for b in range(self.B)]
        for b in range(self.B):
            self.last_dist[b] = self.nearest(b)

    def nearest(self, b):
        """the fp32 of the fp64 minimum over the set; 0 for an empty set"""
        dist = self.tables[self.scan[b]][0]
        return f32(min(dist[self.cur[b], e] for e in self.goals[b])) if self.goals[b] else f32(0.0)

    def advance(self, cand_node, env_action, mask):
        """-> (reward, dist) fp32 [B]; moves the episodes"""
        reward, dist_ = np.zeros(self.B, f32), np.zeros(self.B, f32)
        for b in range(self.B):
            a = int(env_action[b])
            if a >= 0:
                self.cur[b] = int(cand_node[b, a])
                self.path[b].append(self.cur[b])
            d, ld = self.nearest(b), self.last_dist[b]
            r = f32(0.0)
            if mask[b] != 0:
                if a < 0:
                    r = f32(2.0) if d == 0 else f32(-2.0)
                else:
                    gain = -(d - ld)
                    r = f32(1.0) if gain > 0 else f32(-1.0) if gain < 0 else f32(0.0)
            reward[b], dist_[b] = r, d
            self.last_dist[b] = d
        return reward, dist_


class ReturnRef(EpisodesRef):
    """ReturnEpisodes on the host.  `ended` is the recorder's: `advance` is handed it as the policy step left it (ended before the
    step, or a stop) and returns what the kernel leaves."""

    def __init__(self, tables, scan, start, gt, gt_len, midstop):
        super().__init__(tables, scan, start, gt, gt_len)
        self.midstop = [int(v) for v in midstop]
        self.first_ended, self.midstop_at = np.zeros(self.B, bool), np.full(self.B, -1, np.int32)
        for b in range(self.B):
            self.last_dist[b] = self.tables[self.scan[b]][0][self.cur[b], self.midstop[b]]

    def advance(self, cand_node, env_action, mask, ended, end_on_miss=True):
        """-> (reward, dist, ndtw) fp32 [B], ended bool [B]; moves the episodes"""
        B = self.B
        reward, dist_, ndtw_, ended = np.zeros(B, f32), np.zeros(B, f32), np.zeros(B, f32), np.array(ended, bool)
        for b in range(B):
            dist, a = self.tables[self.scan[b]][0], int(env_action[b])
            if a >= 0:
                self.cur[b] = int(cand_node[b, a])
                self.path[b].append(self.cur[b])
                self.row[b] = dtw_row(self.row[b], dist[self.cur[b], self.gt[b]])
            d0, d1 = f32(dist[self.cur[b], self.midstop[b]]), f32(dist[self.cur[b], self.gt[b][-1]])
            second = bool(self.first_ended[b])
            d, nd, ld, ln = (d1 if second else d0), self.ndtw(b), self.last_dist[b], self.last_ndtw[b]
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
            new_ld = d
            if mask[b] != 0 and a < 0 and not second:
                self.midstop_at[b], self.first_ended[b], new_ld = self.cur[b], True, d1
                ended[b] = bool(end_on_miss) and not d < f32(3.0)
            elif mask[b] == 0:
                self.first_ended[b] = True
            reward[b], dist_[b], ndtw_[b] = r, d, nd
            self.last_dist[b], self.last_ndtw[b] = new_ld, nd
        return reward, dist_, ndtw_, ended


def _length(dist, nodes):
    return float(np.sum([dist[a, b] for a, b in zip(nodes[:-1], nodes[1:])]))


def eval_goals_ref(dist, path, goals, gt=None):
    """the seven scores of one trajectory against a goal set in GOALS_COLS order"""
    path, goals = [int(v) for v in path], [int(v) for v in goals]
    plen = _length(dist, path)
    gtl = _length(dist, [int(v) for v in gt]) if gt is not None else min(dist[path[0], e] for e in goals)
    success, oracle = float(path[-1] in goals), float(any(x in goals for x in path))
    ratio = gtl / max(plen, gtl, 0.01)
    return np.array([len(path) - 1, plen, success, oracle, success * ratio, gtl - min(dist[path[-1], e] for e in goals), ratio], np.float64)


def eval_back_ref(dist, path, gt, midstop, gt_midstop):
    """R2RBackBatch._eval_item's nine scores in BACK_COLS order; midstop -1 = None"""
    from _nav_ref import eval_ref
    r2r = eval_ref(dist, path, gt)                       # nav_error 0, steps 2, lengths 3, DTW 7, nDTW 8, CLS 10
    glen = _length(dist, [int(v) for v in gt])
    success = float(midstop >= 0 and dist[int(midstop), int(gt_midstop)] <= 3.0 and r2r[0] <= 3.0)
    return np.array([r2r[0], r2r[2], r2r[3], success, success * glen / max(r2r[3], glen, 0.01), r2r[7], r2r[8], success * r2r[8], r2r[10]], np.float64)
