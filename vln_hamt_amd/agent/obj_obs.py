"""REVERIE's candidate objects of a rollout step on the device: an object store next to the viewpoint store, and the static buffers
one step's object block is gathered into.

The reference builds the block on the host at every step: `ReverieNavRefBatch._get_obs` (finetune_src/reverie/env.py:181-215) looks the
current viewpoint up in the object database, joins each object's feature with the angle feature of the view it was seen in
(`angle_feature[viewIndex][viewindexs[k]]`, the view index NOT reduced mod 12), forms the normalised boxes (`get_obj_local_pos`,
reverie/data_utils.py:25-31) and keeps the first `max_objects`; the agent's `_object_variable` (reverie/agent.py:125-139) pads the batch
with zeros and uploads it.  Like the panorama, it is a pure function of (scan, viewpoint, view index).

`ObjStore` holds that function as CSR tables over the rows of an `ObsStore` (row = vp_base[scan] + local node), sharing its `ang36`,
`vp_base` and `scan_n`.  `ObjEpisodes` owns the output buffers of the B episodes of an `ObsEpisodes`; `observe()` is one launch
(`ops.obj_gather`) and nothing crosses to the host.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import ops

VIEWS = ops.OBS_VIEWS
ObjObservation = namedtuple("ObjObservation", "obj_feats obj_angles obj_poses obj_masks obj_lens obj_ids")
OBJ_TABLES = ("obj_off", "obj_feat", "obj_view", "obj_pos", "obj_id")


def _obj_id(raw, where):
    if isinstance(raw, bytes):
        raw = raw.decode()
    try:
        oid = int(str(raw))
    except ValueError:
        oid = -1
    if not 0 <= oid < 2 ** 31:
        raise ops.L.HamtError(f"ObjStore: object id {raw!r} of {where} is not a non-negative integer below 2^31")
    return oid


def build_obj_tables(graphs, obj_db, obj_feat_size, max_objects=20):
    """The host side of `ObjStore`: {name: numpy array} for OBJ_TABLES plus 'max_objs' (the largest count kept).  `graphs` needs `scans`,
    `nodes[scan]` and `scan_n_host` (an agent.NavGraphs, with or without a device); `obj_db` is the reference's own dict,
    {"scan_viewpoint": {'obj_ids', 'fts' [n, >= obj_feat_size], 'bboxes' [n, 4] (x1, y1, w, h), 'viewindexs' [n]}} (what
    reverie.data_utils.load_obj_database returns).  A viewpoint that is not in it has no objects; the first `max_objects` are kept, in
    file order.  The boxes become [x1/640, y1/480, (x1+w)/640, (y1+h)/480, w*h/(640*480)] in numpy AT THE DTYPE THE DATABASE GIVES and
    are then rounded to float32, as the reference's float32 batch array rounds them."""
    Fo, M = int(obj_feat_size), int(max_objects)
    if not 0 < M <= ops.OBJ_MAX_WIDTH:
        raise ops.L.HamtError(f"ObjStore: max_objects {M} outside the supported (0, {ops.OBJ_MAX_WIDTH}]")
    NV = int(np.asarray(graphs.scan_n_host, np.int64).sum())
    off, feat, view, pos, ids = np.zeros(NV + 1, np.int64), [], [], [], []
    row = 0
    for scan in graphs.scans:
        for vp in graphs.nodes[scan]:
            key = f"{scan}_{vp}"
            n = 0
            if key in obj_db:
                e = obj_db[key]
                fts, boxes, vidx = np.asarray(e["fts"]), np.asarray(e["bboxes"]), np.asarray(e["viewindexs"])
                n_all = len(e["obj_ids"])
                if fts.ndim != 2 or fts.shape[0] != n_all or fts.shape[1] < Fo:
                    raise ops.L.HamtError(f"ObjStore: fts of {key} are {fts.shape}, need [{n_all}, >= {Fo}]")
                if boxes.shape != (n_all, 4) or vidx.shape != (n_all,):
                    raise ops.L.HamtError(f"ObjStore: {key} has {n_all} ids, bboxes {boxes.shape} and viewindexs {vidx.shape}")
                n = min(n_all, M)
                if n and (vidx[:n].min() < 0 or vidx[:n].max() >= VIEWS or not np.array_equal(vidx[:n], vidx[:n].astype(np.int64))):
                    raise ops.L.HamtError(f"ObjStore: viewindexs of {key} outside [0, {VIEWS}): {vidx[:n].tolist()}")
                if n:
                    x1, y1, w, h = boxes[:n, 0], boxes[:n, 1], boxes[:n, 2], boxes[:n, 3]
                    feat.append(fts[:n, :Fo].astype(np.float32))
                    view.append(vidx[:n].astype(np.int32))
                    pos.append(np.stack([x1 / 640, y1 / 480, (x1 + w) / 640, (y1 + h) / 480, w * h / (640 * 480)], 1).astype(np.float32))
                    ids.append(np.array([_obj_id(i, key) for i in list(e["obj_ids"])[:n]], np.int32))
            off[row + 1] = off[row] + n
            row += 1
    cat = lambda parts, shape, dt: np.concatenate(parts, 0) if parts else np.zeros(shape, dt)
    return {"obj_off": off, "obj_feat": cat(feat, (0, Fo), np.float32), "obj_view": cat(view, (0,), np.int32),
            "obj_pos": cat(pos, (0, 5), np.float32), "obj_id": cat(ids, (0,), np.int32), "max_objs": int(np.diff(off).max(initial=0))}


class ObjStore:
    """Device tables over the objects of the NV viewpoints of `obs_store` (an agent.ObsStore), CSR over its rows:
      obj_off int64 [NV + 1]; obj_feat fp32 [NObj, Fo]; obj_view int32 [NObj] (the view each object was seen in); obj_pos fp32 [NObj, 5];
      obj_id int32 [NObj].
    `obj_db`: the reference's object database as a dict (`build_obj_tables`); the first `obj_feat_size` columns of its features and the
    first `max_objects` objects of a viewpoint are kept.  `ang36`, `vp_base` and `scan_n` are the viewpoint store's own tensors.
    `max_objs`: the largest count of a viewpoint, read off the table."""

    def __init__(self, obs_store, obj_db, obj_feat_size=2048, max_objects=20):
        if getattr(obs_store, "graphs", None) is None:
            raise ops.L.HamtError("ObjStore: the viewpoint store carries no graphs (built by from_tensors); use ObjStore.from_tensors")
        t = build_obj_tables(obs_store.graphs, obj_db, obj_feat_size, max_objects)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(obs_store.device)
        self._set(obs_store, *(up(t[k]) for k in OBJ_TABLES))
        self.max_objs = t["max_objs"]

    def _set(self, obs_store, obj_off, obj_feat, obj_view, obj_pos, obj_id):
        dev, NV = obs_store.device, obs_store.NV
        if not obj_feat.is_cuda:
            raise ops.L.HamtError(f"ObjStore: the tables are on {obj_feat.device}; the gather runs on the GPU only (no CPU path)")
        if obj_feat.dim() != 2 or obj_feat.shape[1] < 1:
            raise ops.L.HamtError(f"ObjStore: obj_feat must be [NObj, Fo], got {tuple(obj_feat.shape)}")
        NObj, Fo = obj_feat.shape
        for name, t_, dt, shape in (("obj_off", obj_off, torch.int64, (NV + 1,)), ("obj_feat", obj_feat, torch.float32, (NObj, Fo)),
                                    ("obj_view", obj_view, torch.int32, (NObj,)), ("obj_pos", obj_pos, torch.float32, (NObj, 5)),
                                    ("obj_id", obj_id, torch.int32, (NObj,))):
            ops._nav_arg("ObjStore: " + name, t_, dt, shape, dev)
        self.obs_store, self.obj_off, self.obj_feat, self.obj_view, self.obj_pos, self.obj_id = obs_store, obj_off, obj_feat, obj_view, obj_pos, obj_id
        self.ang36, self.vp_base, self.scan_n = obs_store.ang36, obs_store.vp_base, obs_store.scan_n
        self.NV, self.NObj, self.Fo, self.A, self.device = NV, NObj, Fo, obs_store.A, dev

    @classmethod
    def from_tensors(cls, obs_store, obj_off, obj_feat, obj_view, obj_pos, obj_id):
        """A store over ready device tensors (shapes and dtypes as in the class docstring).  The offsets are checked and `max_objs` is
        read off them: one pass and one blocking read."""
        self = cls.__new__(cls)
        self._set(obs_store, obj_off, obj_feat, obj_view, obj_pos, obj_id)
        cnt = obj_off[1:] - obj_off[:-1]
        first, last, lo, hi = (int(v) for v in torch.stack([obj_off[0], obj_off[-1], cnt.min(), cnt.max()]).tolist())
        if first != 0 or last != self.NObj or lo < 0 or hi > ops.OBJ_MAX_WIDTH:
            raise ops.L.HamtError(f"ObjStore: obj_off must ascend from 0 to NObj = {self.NObj} in steps of at most {ops.OBJ_MAX_WIDTH}")
        self.max_objs = hi
        return self


class ObjEpisodes:
    """The object block of each of the B episodes of `obs_episodes` (an agent.ObsEpisodes, which owns their view index; its NavEpisodes
    owns their scan and current node), gathered into static buffers.

        objs = ObjEpisodes(obj_store, obs).reset()
        goal = goal_objects(batch).to(device)
        for t in range(T):
            o, j = obs.observe(), objs.observe()              # BEFORE obs.turn: the objects are seen from the view of this step
            outs = model('visual', ..., obj_feats=j.obj_feats, obj_angles=j.obj_angles, obj_poses=j.obj_poses, obj_masks=j.obj_masks)
            a_t, env_action, prev = rec.step(t, outs[0], outs[1], j.obj_lens, cand_lens=o.cand_len, ..., obj_ids=j.obj_ids, goal_obj=goal)
            obs.turn(env_action, t)

    `width`: the object slots per episode, default max(store.max_objs, 1); a smaller one is refused, and so is one above 256 (the
    step's limit on O).  `observe()` reads `obs_episodes.view`, so it must be called before `obs_episodes.turn` moves the view on.  It
    returns views of the SAME buffers every time (valid until the next call): `obj_masks` as bool with ONE live slot at a viewpoint
    without objects, as the reference's `max(len, 1)` gives the model; `obj_lens` int32 the TRUE count, as the recorder wants it;
    `obj_ids` int32, -1 at padding.  `anomalies` int32 [1] counts the episodes found outside their scan or their 36 views."""

    def __init__(self, obj_store, obs_episodes, width=None):
        need = max(int(obj_store.max_objs), 1)
        Ow = need if width is None else int(width)
        if Ow < need:
            raise ValueError(f"ObjEpisodes: width {Ow} below the {need} objects of the store's fullest viewpoint")
        if Ow > ops.OBJ_MAX_WIDTH:
            raise ValueError(f"ObjEpisodes: width {Ow} above the {ops.OBJ_MAX_WIDTH} object slots a rollout step takes")
        if obs_episodes.store is not obj_store.obs_store:
            raise ValueError("ObjEpisodes: the episodes run over another viewpoint store than the object store's")
        self.store, self.obs, self.nav, self.Ow, self.B = obj_store, obs_episodes, obs_episodes.nav, Ow, int(obs_episodes.B)
        dev, B, Fo, A = obj_store.device, self.B, obj_store.Fo, obj_store.A
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        self.obj_feats, self.obj_angles, self.obj_poses = z(B, Ow, Fo), z(B, Ow, A), z(B, Ow, 5)
        self.obj_masks, self.obj_lens = z(B, Ow, dtype=torch.uint8), z(B, dtype=torch.int32)
        self.obj_ids = torch.full((B, Ow), -1, dtype=torch.int32, device=dev)
        self.anomalies = z(1, dtype=torch.int32)
        self._obs = ObjObservation(self.obj_feats, self.obj_angles, self.obj_poses, self.obj_masks.view(torch.bool), self.obj_lens, self.obj_ids)

    def reset(self):
        """New rollout: the anomaly count starts again (the positions and views are the NavEpisodes' and the ObsEpisodes')."""
        self.anomalies.zero_()
        return self

    def observe(self) -> ObjObservation:
        ops.obj_gather(self.store, self.nav.scan, self.nav.cur, self.obs.view, self, self.anomalies)
        return self._obs

    def state_tensors(self):
        """what a step mutates beyond its outputs (graph.GraphedInference's `state`)"""
        return (self.anomalies,)


def goal_objects(items):
    """int32 [B] (a host tensor) of the episodes' goal object, `item['objId']` of each instruction item; None becomes -1, an id no object
    of a store can have, so the step's object target is then ignored."""
    return torch.tensor([-1 if it.get("objId") is None else _obj_id(it["objId"], "an episode") for it in items], dtype=torch.int32)
