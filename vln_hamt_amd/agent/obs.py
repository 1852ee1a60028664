"""The observations of a rollout step on the device: a viewpoint store and the per-rollout view state over it.

The reference builds them on the host at every step: `R2RBatch._get_obs` (finetune_src/r2r/env.py:270-305) looks every candidate of the
current viewpoint up in `buffered_state_dict` (`make_candidate`, :182-252) and the agent re-stacks them, STOP and the remaining views in
numpy and uploads the result (`_cand_pano_feature_variable`, agent_cmt.py:104-151; `_candidate_variable`, :153-171;
`_history_variable`, :173-190).  None of that needs the simulator: with discretised viewing angles an observation is a pure function of
(scan, viewpoint, view index), a move in the Matterport graph is deterministic, and after a move the view index is the chosen
candidate's `pointId` (`make_equiv_action`, :213-246).

`ObsStore` holds that function as device tables over every viewpoint of a `NavGraphs`, in its arena order (row = vp_base[scan] + local
node).  `ObsEpisodes` owns the view index of every episode of a `NavEpisodes` and the static output buffers; `observe()` is one launch
(`ops.obs_gather`), `turn()` one more (`ops.obs_turn`), and nothing crosses to the host.

Candidate angle features follow `make_candidate`'s CACHED branch (:239-252): `angle_feature(normalized_heading - (view % 12) * 30 deg,
elevation)` in Python doubles, rounded once to float32.  The first-visit branch (:189-228) forms the same heading as
`(state.heading - base) + rel_heading`, which associates the sum differently and can differ in the last bit; from the second visit of a
viewpoint on the reference itself serves the cached form, and this store serves it always.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from .. import ops
from ..data.r2r_data import _view_angles, angle_feature, get_all_point_angle_feature

VIEWS, HEADINGS = ops.OBS_VIEWS, 12
Observation = namedtuple("Observation", "ob_img ob_ang ob_nav ob_mask ob_len cand_len cand_nodes cand_points hist_img hist_pano_img hist_pano_ang")
TABLES = ("feat", "ang36", "cand_cnt", "cand_point", "cand_node", "cand_ang", "vp_base", "scan_n")


def build_tables(graphs, features, candidates, image_feat_size=768, angle_feat_size=4, angle_table=None):
    """The host side of `ObsStore`: {name: numpy array} for TABLES plus 'max_cands' and 'max_ob_len'.  `graphs` needs `scans`,
    `nodes[scan]`, `scan_n_host` and `node_id(scan, viewpoint)` (an agent.NavGraphs, with or without a device)."""
    F, A = int(image_feat_size), int(angle_feat_size)
    scan_n = np.asarray(graphs.scan_n_host, np.int32)
    vp_base = np.concatenate([[0], np.cumsum(scan_n.astype(np.int64))[:-1]]).astype(np.int64)
    NV = int(scan_n.sum())
    missing = [f"{s}_{vp}" for s in graphs.scans for vp in graphs.nodes[s] if f"{s}_{vp}" not in candidates]
    if missing:
        raise ops.L.HamtError(f"ObsStore: no candidate list for {len(missing)} viewpoints ({', '.join(missing[:4])}, ...)")
    C = max(1, max(len(candidates[f"{s}_{vp}"]) for s in graphs.scans for vp in graphs.nodes[s]))
    if C > ops.OBS_MAX_CAND:
        raise ops.L.HamtError(f"ObsStore: a viewpoint with {C} candidates, above the supported {ops.OBS_MAX_CAND}")
    feat = np.zeros((NV, VIEWS, F), np.float32)
    cnt, point, node = np.zeros(NV, np.int32), np.full((NV, C), -1, np.int32), np.full((NV, C), -1, np.int32)
    ang = np.zeros((NV, C, HEADINGS, A), np.float32)
    step = math.radians(30)
    for si, scan in enumerate(graphs.scans):
        for li, vp in enumerate(graphs.nodes[scan]):
            row = int(vp_base[si]) + li
            fts = np.asarray(features.get_image_feature(scan, vp))
            if fts.shape[0] != VIEWS or fts.shape[1] < F:
                raise ops.L.HamtError(f"ObsStore: features of {scan}_{vp} are {fts.shape}, need [36, >= {F}]")
            feat[row] = fts[:, :F]
            cands = candidates[f"{scan}_{vp}"]
            cnt[row] = len(cands)
            for c, cc in enumerate(cands):
                if not 0 <= int(cc["pointId"]) < VIEWS:
                    raise ops.L.HamtError(f"ObsStore: candidate {c} of {scan}_{vp} has pointId {cc['pointId']}")
                point[row, c], node[row, c] = int(cc["pointId"]), graphs.node_id(scan, cc["viewpointId"])
                for h in range(HEADINGS):          # (make_candidate's cached branch, env.py:239-252: base_heading = (viewId % 12) * radians(30))
                    ang[row, c, h] = angle_feature(cc["normalized_heading"] - h * step, cc["elevation"], A)
    ang36 = np.stack(get_all_point_angle_feature(A), 0) if angle_table is None else np.stack([np.asarray(a, np.float32) for a in angle_table], 0)
    taken = np.zeros((NV, VIEWS), bool)
    for c in range(C):
        ok = c < cnt
        taken[np.flatnonzero(ok), point[ok, c]] = True
    return {"feat": feat, "ang36": ang36.astype(np.float32), "cand_cnt": cnt, "cand_point": point, "cand_node": node, "cand_ang": ang,
            "vp_base": vp_base, "scan_n": scan_n, "max_cands": int(cnt.max(initial=0)), "max_ob_len": int((cnt + 1 + VIEWS - taken.sum(1)).max(initial=1))}


class ObsStore:
    """Device tables over the NV viewpoints of `graphs` (an agent.NavGraphs on a device), row = vp_base[scan] + local node:
      feat fp32 [NV, 36, F]; ang36 fp32 [36, 36, A] (base view, view); cand_cnt int32 [NV]; cand_point / cand_node int32 [NV, C] (each
      candidate's view index / local node, -1 = padding); cand_ang fp32 [NV, C, 12, A] (its angle feature per base heading).
    `features`: anything with `get_image_feature(scan, viewpoint) -> [36, >= image_feat_size]` (data.r2r_data.ViewFeatureStore,
    MultiStepNavData); the first `image_feat_size` columns are kept.  `candidates`: {"scan_viewpoint": [{'viewpointId', 'pointId',
    'normalized_heading', 'elevation', ...}, ...]}, the reference's own `buffered_state_dict`; list order is slot order
    (`candidates_from_scanvp` converts the pretraining `scanvp_cands.json`).  `angle_table` [36, 36, A]: the view angle features,
    default the table data.r2r_data builds; pass the simulator's `env.angle_feature` for byte agreement with it.
    `max_cands` / `max_ob_len`: the largest candidate count, and the longest panorama observation (candidates + STOP + the views no
    candidate points to), read off the table."""

    def __init__(self, graphs, features, candidates, image_feat_size=768, angle_feat_size=4, angle_table=None, device=None):
        device = graphs.device if device is None else torch.device(device)
        if device is None:
            raise ops.L.HamtError("ObsStore: no device (the graphs are on none either); there is no CPU path")
        t = build_tables(graphs, features, candidates, image_feat_size, angle_feat_size, angle_table)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self._set(*(up(t[k]) for k in TABLES))
        self.max_cands, self.max_ob_len, self.graphs = t["max_cands"], t["max_ob_len"], graphs

    def _set(self, feat, ang36, cand_cnt, cand_point, cand_node, cand_ang, vp_base, scan_n):
        NV, V, F = feat.shape
        A, C = ang36.shape[-1], cand_point.shape[1] if cand_point.dim() == 2 else -1
        dev = feat.device
        if not feat.is_cuda:
            raise ops.L.HamtError(f"ObsStore: the tables are on {dev}; the gather runs on the GPU only (no CPU path)")
        if not 0 < C <= ops.OBS_MAX_CAND:
            raise ops.L.HamtError(f"ObsStore: cand_point must be [NV, C] with 0 < C <= {ops.OBS_MAX_CAND}, got {tuple(cand_point.shape)}")
        for name, t_, dt, shape in (("feat", feat, torch.float32, (NV, VIEWS, F)), ("ang36", ang36, torch.float32, (VIEWS, VIEWS, A)),
                                    ("cand_cnt", cand_cnt, torch.int32, (NV,)), ("cand_point", cand_point, torch.int32, (NV, C)),
                                    ("cand_node", cand_node, torch.int32, (NV, C)), ("cand_ang", cand_ang, torch.float32, (NV, C, HEADINGS, A)),
                                    ("vp_base", vp_base, torch.int64, tuple(scan_n.shape)), ("scan_n", scan_n, torch.int32, tuple(scan_n.shape))):
            ops._nav_arg("ObsStore: " + name, t_, dt, shape, dev)
        self.feat, self.ang36, self.cand_cnt, self.cand_point, self.cand_node, self.cand_ang = feat, ang36, cand_cnt, cand_point, cand_node, cand_ang
        self.vp_base, self.scan_n = vp_base, scan_n
        self.NV, self.F, self.A, self.C, self.device, self.graphs = NV, F, A, C, dev, None

    @classmethod
    def from_tensors(cls, feat, ang36, cand_cnt, cand_point, cand_node, cand_ang, vp_base, scan_n):
        """A store over ready device tensors (shapes and dtypes as in the class docstring; vp_base int64 and scan_n int32, one entry per
        scan).  `max_cands` / `max_ob_len` are read off the table: one pass over it and one blocking read."""
        self = cls.__new__(cls)
        self._set(feat, ang36, cand_cnt, cand_point, cand_node, cand_ang, vp_base, scan_n)
        live = torch.arange(self.C, device=self.device)[None] < cand_cnt[:, None]
        hits = torch.zeros(self.NV, VIEWS, dtype=torch.int32, device=self.device)
        hits.scatter_add_(1, cand_point.clamp(0, VIEWS - 1).long(), live.to(torch.int32))
        n = cand_cnt.clamp(0, self.C)
        self.max_cands = int(n.max()) if self.NV else 0
        self.max_ob_len = int((n + 1 + VIEWS - (hits > 0).sum(1)).max()) if self.NV else 1
        return self

    @staticmethod
    def candidates_from_scanvp(scanvp_cands):
        """The pretraining `scanvp_cands.json` ({"scan_vp": {next_vp: [view index, distance, heading offset, elevation offset]}}) in the
        form of `buffered_state_dict`, file order kept: normalized_heading = the view's heading + the heading offset, elevation = the
        view's elevation + the elevation offset (the view angles of data.r2r_data._view_angles)."""
        views = _view_angles()
        out = {}
        for key, cands in scanvp_cands.items():
            scan = key.rsplit("_", 1)[0]
            out[key] = [{"normalized_heading": views[int(v[0])][0] + v[2], "elevation": views[int(v[0])][1] + v[3], "scanId": scan,
                         "viewpointId": vp, "pointId": int(v[0]), "idx": j + 1} for j, (vp, v) in enumerate(cands.items())]
        return out


class ObsEpisodes:
    """The view index of each of `nav`'s B episodes (an agent.NavEpisodes, which owns their scan and current node) and the static
    buffers one step's observation is gathered into.

        obs = ObsEpisodes(store, nav).reset(view_indices)
        for t in range(T):
            o = obs.observe()
            logit = model('visual', ..., ob_img_feats=o.ob_img, ob_ang_feats=o.ob_ang, ob_nav_types=o.ob_nav, ob_masks=o.ob_mask)
            a_t, env_action, prev = rec.step(t, logit, cand_lens=o.cand_len, ob_ang_feats=o.ob_ang, sync=False, nav=nav, cand_nodes=o.cand_nodes)
            obs.turn(env_action, t)
            hist.append(model('history', hist_img_feats=o.hist_img, hist_ang_feats=prev, hist_pano_img_feats=o.hist_pano_img, ...))

    `width`: the slots per episode, default `store.max_ob_len` ('pano') or `store.max_cands + 1` ('cand'); a smaller one is refused.
    `observe()` returns views of the SAME buffers every time (valid until the next call), `ob_mask` as bool, `ob_nav` int64, `ob_len`
    and `cand_len` int32 on the device.  `anomalies` int32 [1] counts the episodes found outside their scan or their 36 views."""

    def __init__(self, store: ObsStore, nav, width=None, layout="pano", hist_pano=True):
        if layout not in ops.OBS_LAYOUTS:
            raise ValueError(f"ObsEpisodes: layout {layout!r}, expected one of {sorted(ops.OBS_LAYOUTS)}")
        need = store.max_ob_len if layout == "pano" else store.max_cands + 1
        W = need if width is None else int(width)
        if W < need:
            raise ValueError(f"ObsEpisodes: width {W} below the {need} slots the store's longest '{layout}' observation takes")
        self.store, self.nav, self.layout, self.W, self.B = store, nav, layout, W, int(nav.B)
        dev, B, F, A = store.device, self.B, store.F, store.A
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        self.ob_img, self.ob_ang, self.ob_nav, self.ob_mask = z(B, W, F), z(B, W, A), z(B, W, dtype=torch.int64), z(B, W, dtype=torch.uint8)
        self.ob_len, self.cand_len = z(B, dtype=torch.int32), z(B, dtype=torch.int32)
        self.cand_nodes, self.cand_points = z(B, W, dtype=torch.int32), z(B, W, dtype=torch.int32)
        self.hist_img = z(B, F)
        self.hist_pano_img, self.hist_pano_ang = (z(B, VIEWS, F), z(B, VIEWS, A)) if hist_pano else (None, None)
        self.view, self.anomalies = z(B, dtype=torch.int32), z(1, dtype=torch.int32)
        self.view_log = torch.full((int(getattr(nav, "T_max", 0)) + 1, B), -1, dtype=torch.int32, device=dev)
        self._obs = Observation(self.ob_img, self.ob_ang, self.ob_nav, self.ob_mask.view(torch.bool), self.ob_len, self.cand_len, self.cand_nodes,
                                self.cand_points, self.hist_img, self.hist_pano_img, self.hist_pano_ang)

    def reset(self, view_indices):
        """New rollout: episode b looks at view `view_indices[b]` (the simulator's viewIndex after newEpisode)."""
        v = np.asarray(view_indices, dtype=np.int32).reshape(-1)
        if v.shape[0] != self.B or v.min(initial=0) < 0 or v.max(initial=0) >= VIEWS:
            raise ValueError(f"ObsEpisodes.reset: need {self.B} view indices in [0, {VIEWS})")
        self.view.copy_(torch.from_numpy(v))
        self.anomalies.zero_()
        self.view_log.fill_(-1)
        self.view_log[0].copy_(self.view)
        return self

    def observe(self) -> Observation:
        ops.obs_gather(self.store, self.nav.scan, self.nav.cur, self.view, self, self.anomalies, layout=self.layout)
        return self._obs

    def turn(self, env_action, t=None):
        """After the policy step: the episodes that move (`env_action` int32 [B] >= 0, what `RolloutRecorder.step` returned on the
        device) look where their candidate was; with `t`, the resulting views become row t + 1 of the view log.  It reads what `observe`
        wrote, so it may run before or after the recorder's `nav_advance`."""
        row = None
        if t is not None:
            if not 0 <= int(t) < self.view_log.shape[0] - 1:
                raise ValueError(f"ObsEpisodes.turn: step {t} outside the {self.view_log.shape[0] - 1} steps of the episodes")
            row = self.view_log[int(t) + 1]
        ops.obs_turn(self.cand_points, env_action, self.view, row)
        return self.view

    def state_tensors(self):
        """what a step mutates beyond its outputs (graph.GraphedInference's `state`, next to the recorder's and the episodes')"""
        return (self.view, self.view_log, self.anomalies)

    def views(self):
        """int32 [T_max + 1, B] on the device: row 0 the views of `reset`, row t + 1 those after `turn(..., t)`, -1 = not recorded"""
        return self.view_log
