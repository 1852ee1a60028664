"""The pretraining pipeline's view store on the device: the twin of `agent.ObsStore` for the six proxy tasks.

What `MultiStepNavData.get_input` stacks per sample is a pure function of (trajectory, step): the view features of the viewpoints of the
path, the angle tables of the views looked at, the candidates of the viewpoint stood on, the action and progress targets.  `PretrainStore`
holds all of it in HBM once; a batch is then built by ONE `hamt_pretrain_gather` launch (csrc/pretrain_gather.hip) from a 32-byte record
per sample (data/device_tasks.py draws the records, data/device_collate.py ships them), and nothing but the instruction tokens and those
records crosses PCIe.

Every table entry is computed on the host by the very expression the host pipeline evaluates per sample (`build_pretrain_tables` calls
`MultiStepNavData`'s own methods where there is one), so the two pipelines agree bit for bit by construction
(tests/test_device_batches.py, tests/test_gpu_device_batches.py).

Row order.  Viewpoint tables: one row per `"{scan}_{viewpoint}"` key in the order of FIRST VISIT, walking `nav_db.traj_data` in file order
and each (truncated) path front to back.  Step tables: one row per (trajectory, t), t < min(len(path), max_act_len - 1), the trajectories
of `nav_db.traj_data` back to back; `traj_base[i]` is trajectory i's first row (`pretrain_index`).
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from .. import _lib as L
from .r2r_data import angle_feature, softmax
from .r2r_tasks import _standardize_radians, sprel_target_table

VIEWS, HEADINGS = 36, 12
RECORD_WORDS, MAX_HIST, MAX_CAND = 8, 32, 64                   # HAMT_PRETRAIN_RECORD / _MAX_HIST / _MAX_CAND
KILL_V, KILL_A = 1, 2                                           # HAMT_PRETRAIN_KILL_*
LAYOUTS = {"views36": 0, "cands_first": 1}                      # HAMT_PRETRAIN_VIEWS36 / _CANDS_FIRST
REC_BASE, REC_T, REC_FLAGS, REC_MRC, REC_ANCHOR, REC_OB_LEN = range(6)       # the words of a record (6, 7: unused)
TABLES = ("feat", "prob", "ang36", "cand_cnt", "cand_view", "cand_ang", "step_idx", "step_val", "sp_targets")

_STORES: Dict[int, "PretrainStore"] = {}
_next_id = [1]                                                  # ids are never reused: a stale id must not find another store


def _f32(x):
    """a host value -> float32 the way the collate functions convert a per-sample field (collate._pack: torch.as_tensor(...).to(float32))"""
    return torch.as_tensor(np.asarray([np.asarray(x)])).to(torch.float32).numpy()[0]


def pretrain_index(nav_db):
    """The host index the index-only datasets and the tables share: {'traj_base': int64 [n_traj + 1], prefix sum of the steps each
    trajectory of `nav_db.traj_data` owns (min(len(path), max_act_len - 1)); 'ob_len': int32 [NS, 2], the observation length at every
    step in the 36-view layout (37) and in the candidates-first layout (candidates + STOP + the views no candidate points to)}.
    Reads no feature."""
    steps = [min(len(td["path"]), nav_db.max_act_len - 1) for td in nav_db.traj_data]
    too_long = [i for i, n in enumerate(steps) if n > MAX_HIST]
    if too_long:
        raise L.HamtError(f"PretrainStore: trajectory {too_long[0]} has {steps[too_long[0]]} history steps, above the {MAX_HIST} the MRC mask carries")
    traj_base = np.zeros(len(steps) + 1, np.int64)
    np.cumsum(steps, out=traj_base[1:])
    ob_len = np.full((int(traj_base[-1]), 2), VIEWS + 1, np.int32)
    for i, td in enumerate(nav_db.traj_data):
        for t in range(steps[i]):
            cands = nav_db.scanvp_cands.get(f"{td['scan']}_{td['path'][t]}")
            if cands is None:
                raise L.HamtError(f"PretrainStore: no candidate list for {td['scan']}_{td['path'][t]} (step {t} of trajectory {i})")
            ob_len[traj_base[i] + t, 1] = len(cands) + 1 + VIEWS - len({int(v[0]) for v in cands.values()})
    return {"traj_base": traj_base, "ob_len": ob_len}


def build_pretrain_tables(nav_db, with_probs=True):
    """The host side of `PretrainStore`: {name: numpy array} for TABLES (prob None without `with_probs`), plus 'keys' (the viewpoint rows'
    "{scan}_{viewpoint}" in row order), 'traj_base' and 'ob_len' (`pretrain_index`).  `nav_db`: a MultiStepNavData."""
    F, A, P = int(nav_db.image_feat_size), int(nav_db.angle_feat_size), int(nav_db.image_prob_size)
    index = pretrain_index(nav_db)
    traj_base, NS = index["traj_base"], int(index["traj_base"][-1])
    # ---- viewpoint rows, in order of first visit
    rows: Dict[str, int] = {}
    for i, td in enumerate(nav_db.traj_data):
        for vp in td["path"][:int(traj_base[i + 1] - traj_base[i])]:
            rows.setdefault(f"{td['scan']}_{vp}", len(rows))
    keys = list(rows)
    NV = len(keys)
    missing = [k for k in keys if k not in nav_db.features]
    if missing:
        raise L.HamtError(f"PretrainStore: no view features for {len(missing)} viewpoints ({', '.join(missing[:4])}, ...)")
    C = max([1] + [len(nav_db.scanvp_cands[k]) for k in keys])
    if C > MAX_CAND:
        raise L.HamtError(f"PretrainStore: a viewpoint with {C} candidates, above the supported {MAX_CAND}")
    feat = np.zeros((NV, VIEWS, F), np.float32)
    prob = np.zeros((NV, VIEWS, P), np.float32) if with_probs else None
    cand_cnt, cand_view = np.zeros(NV, np.int32), np.full((NV, C), -1, np.int32)
    cand_ang = np.zeros((NV, C, HEADINGS, A), np.float32)
    for key, row in rows.items():
        fts = nav_db.features.get(key)
        if fts.shape[0] != VIEWS or fts.shape[1] < F + (P if with_probs else 0):
            raise L.HamtError(f"PretrainStore: features of {key} are {fts.shape}, need [36, >= {F + (P if with_probs else 0)}]")
        feat[row] = fts[:, :F]
        if with_probs:
            prob[row] = softmax(np.ascontiguousarray(fts[:, F:F + P]))                  # (get_history_feature: softmax(blocks[steps, vidx, F:]))
        cands = nav_db.scanvp_cands[key]
        cand_cnt[row] = len(cands)
        for c, v in enumerate(cands.values()):
            if not 0 <= int(v[0]) < VIEWS:
                raise L.HamtError(f"PretrainStore: candidate {c} of {key} points to view {v[0]}")
            cand_view[row, c] = int(v[0])
            for h in range(HEADINGS):                # (get_ob_cand_pano_view's own expression, rel = rel_angles[path_viewindex]: a function of view % 12)
                rel = nav_db.rel_angles[h]
                cand_ang[row, c, h] = angle_feature(rel[v[0]][0] + v[2], rel[v[0]][1] + v[3], A)
    # ---- step rows
    step_idx = np.zeros((NS, 4), np.int32)
    step_val = np.zeros((NS, A + 5), np.float32)
    for i, td in enumerate(nav_db.traj_data):
        scan, path = td["scan"], td["path"][:nav_db.max_act_len - 1]
        views, act_views, rel_act = td["path_viewindex"], td["action_viewindex"], td["rel_act_angles"]
        goal = td["guide_path"][-1] if "guide_path" in td else path[-1]
        for t in range(len(path)):
            s = int(traj_base[i]) + t
            if not 0 <= int(views[t]) < VIEWS:
                raise L.HamtError(f"PretrainStore: step {t} of trajectory {i} looks at view {views[t]}")
            step_idx[s, 0], step_idx[s, 1] = rows[f"{scan}_{path[t]}"], int(views[t])
            step_val[s, :A] = np.zeros((A,), np.float32) if t == len(path) - 1 else angle_feature(rel_act[t][0], rel_act[t][1], A)
            for lay, build in enumerate((nav_db.get_ob_pano_view, nav_db.get_ob_cand_pano_view)):
                *_, gt_label, gt_angle = build(scan, path, views, act_views, rel_act, t)
                step_idx[s, 2 + lay] = int(gt_label)
                step_val[s, A + 2 * lay:A + 2 * lay + 2] = _f32(_standardize_radians(gt_angle))
            step_val[s, A + 4] = _f32(nav_db.get_progress(scan, path[0], path[t], goal))
    return {"feat": feat, "prob": prob, "ang36": np.ascontiguousarray(nav_db._angle_table, np.float32), "cand_cnt": cand_cnt,
            "cand_view": cand_view, "cand_ang": cand_ang, "step_idx": step_idx, "step_val": step_val,
            "sp_targets": torch.as_tensor(sprel_target_table()).to(torch.float32).numpy(), "keys": keys, **index}


class PretrainStore:
    """Device tables of a MultiStepNavData (module docstring for the row order; include/hamt.h: hamt_pretrain_gather for the layout):
      feat fp32 [NV, 36, F]; prob fp32 [NV, 36, P] or None; ang36 fp32 [36, 36, A]; cand_cnt int32 [NV]; cand_view int32 [NV, C];
      cand_ang fp32 [NV, C, 12, A]; step_idx int32 [NS, 4]; step_val fp32 [NS, A + 5]; sp_targets fp32 [36, 36, 2].
    Building one registers it under `store.id` and marks `nav_db.device_store_id` with it: the index-only datasets over that `nav_db` stamp
    their items with the id and `IndexedBatch.to_device` finds the store through `get_store` -- no device tensor sits in a dataset or a batch.
    `anomalies` int32 [1] counts the samples whose record pointed outside the tables (they come out as zeros); `check()` reads it, once per
    epoch or on request.  `nbytes`: the HBM footprint.  There is no CPU path."""

    def __init__(self, nav_db, device, with_probs=True):
        device = None if device is None else torch.device(device)
        if device is None or device.type != "cuda":
            raise L.HamtError(f"PretrainStore: device is {device}; the gather runs on the GPU only (no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = build_pretrain_tables(nav_db, with_probs)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self._set(*(up(t[k]) for k in TABLES))
        self.keys, self.traj_base, self.ob_len = t["keys"], t["traj_base"], t["ob_len"]
        nav_db.device_store_id = self.id

    def _set(self, feat, prob, ang36, cand_cnt, cand_view, cand_ang, step_idx, step_val, sp_targets):
        if not feat.is_cuda:
            raise L.HamtError(f"PretrainStore: the tables are on {feat.device}; the gather runs on the GPU only (no CPU path)")
        if feat.dim() != 3 or ang36.dim() != 3 or cand_view.dim() != 2 or not 0 < cand_view.shape[1] <= MAX_CAND:
            raise L.HamtError(f"PretrainStore: need feat [NV, 36, F], ang36 [36, 36, A] and cand_view [NV, C] with 0 < C <= {MAX_CAND}")
        (NV, _, F), A, C, NS, dev = feat.shape, ang36.shape[-1], cand_view.shape[1], step_idx.shape[0], feat.device
        P = 0 if prob is None else prob.shape[-1]
        for name, t_, dt, shape in (("feat", feat, torch.float32, (NV, VIEWS, F)), ("prob", prob, torch.float32, (NV, VIEWS, P)),
                                    ("ang36", ang36, torch.float32, (VIEWS, VIEWS, A)), ("cand_cnt", cand_cnt, torch.int32, (NV,)),
                                    ("cand_view", cand_view, torch.int32, (NV, C)), ("cand_ang", cand_ang, torch.float32, (NV, C, HEADINGS, A)),
                                    ("step_idx", step_idx, torch.int32, (NS, 4)), ("step_val", step_val, torch.float32, (NS, A + 5)),
                                    ("sp_targets", sp_targets, torch.float32, (VIEWS, VIEWS, 2))):
            if t_ is not None and (t_.dtype != dt or tuple(t_.shape) != shape or not t_.is_contiguous() or t_.device != dev):
                raise L.HamtError(f"PretrainStore: {name} must be a contiguous {dt} tensor of shape {shape} on {dev}, got {t_.dtype} "
                                  f"{tuple(t_.shape)} on {t_.device}")
        self.feat, self.prob, self.ang36, self.cand_cnt, self.cand_view, self.cand_ang = feat, prob, ang36, cand_cnt, cand_view, cand_ang
        self.step_idx, self.step_val, self.sp_targets = step_idx, step_val, sp_targets
        self.NV, self.NS, self.F, self.A, self.P, self.C, self.device = NV, NS, F, A, P, C, dev
        self.anomalies = torch.zeros(1, dtype=torch.int32, device=dev)
        self.keys = self.traj_base = self.ob_len = None
        self.id, _next_id[0] = _next_id[0], _next_id[0] + 1
        _STORES[self.id] = self

    @classmethod
    def from_tensors(cls, feat, prob, ang36, cand_cnt, cand_view, cand_ang, step_idx, step_val, sp_targets):
        """A store over ready device tensors (shapes and dtypes as in the class docstring; `prob` may be None).  It is registered like any
        other; its records come from the caller, word REC_OB_LEN carrying each sample's observation length."""
        self = cls.__new__(cls)
        self._set(feat, prob, ang36, cand_cnt, cand_view, cand_ang, step_idx, step_val, sp_targets)
        return self

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (getattr(self, k) for k in TABLES) if t is not None)

    def check(self, reset=True) -> int:
        """The number of samples gathered as zeros since the last reset (one blocking read): call it once per epoch, not per batch."""
        torch.cuda.synchronize(self.device)          # (the gathers may run on a copy stream: PrefetchLoader)
        n = int(self.anomalies.item())
        if reset:
            self.anomalies.zero_()
        return n

    def close(self):
        """Take the store out of the registry (its tensors go when the last reference does)."""
        _STORES.pop(self.id, None)


def get_store(store_id) -> PretrainStore:
    store = _STORES.get(int(store_id)) if store_id is not None else None
    if store is None:
        raise L.HamtError(f"no PretrainStore with id {store_id} in this process: build PretrainStore(nav_db, device) before the index-only "
                          "batches are moved to the device (there is no CPU path and no host substitute)")
    return store
