"""Shared by tests/test_device_batches.py (CPU) and tests/test_gpu_device_batches.py: the tiny dataset's databases and datasets for both
pipelines, the cases, a numpy restatement of `hamt_pretrain_gather` (plain loops over the records: no code shared with the kernel or
with data/device_collate.py), and a numpy reader of the PackedBatch layout (what the unpack kernels do to a host batch)."""
import os
import random
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "tests", "golden", "r2r_tiny")
DIMS = dict(image_feat_size=16, image_prob_size=10, angle_feat_size=4)
TOK = types.SimpleNamespace(cls_token_id=101, sep_token_id=102, mask_token_id=103, pad_token_id=0)
TASKS = ("mlm", "mrc", "itm", "sap", "sar", "sprel")
OB_TASKS = ("sap", "sar", "sprel")
KILL_V, KILL_A, MRC_PROB = 0.3, 0.43, 0.5
HIST_FIELDS = ("hist_img_fts", "hist_ang_fts", "hist_pano_img_fts", "hist_pano_ang_fts")
# (task, dataset indices, seed).  The tiny dataset: 6 (trajectory, instruction) pairs (index 2 = the 6-step path cut to 5 by
# max_act_len = 6), 24 (trajectory, instruction, step) triples, step 0 at indices 0, 4, 8, 13, 17, 21.
CASES = [("mlm", [3], 11), ("mlm", [0, 2, 5, 1, 4], 12), ("mrc", [2], 88), ("mrc", [1, 3, 4, 2, 0], 22), ("itm", [5], 31), ("itm", [4, 0, 2, 3, 1], 32),
         ("sap", [13], 41), ("sap", [0, 4, 8, 17, 21], 42), ("sap", [0, 3, 7, 12, 14], 43), ("sar", [9], 51), ("sar", [1, 2, 12, 13, 23], 52),
         ("sprel", [8], 61), ("sprel", [0, 5, 11, 12, 20], 62), ("sprel", [4, 6, 10, 16, 22], 63)]
CONFIGS = [(pano, cand) for pano in (True, False) for cand in (False, True)]          # (hist_enc_pano, ob_cand_pano_view)

_dbs = {}


def nav_db(pano=True, cand=False):
    """one MultiStepNavData per configuration and process (host index only: the feature file is read lazily)"""
    from vln_hamt_amd.data.r2r_data import MultiStepNavData
    if (pano, cand) not in _dbs:
        _dbs[pano, cand] = MultiStepNavData(
            traj_files=[os.path.join(TINY, "traj.jsonl"), os.path.join(TINY, "traj2.jsonl")], img_ft_file=os.path.join(TINY, "img_fts.npz"),
            scanvp_cands_file=os.path.join(TINY, "scanvp_cands.json"), connectivity_dir=TINY, max_txt_len=12, max_act_len=6,
            hist_enc_pano=pano, ob_cand_pano_view=cand, in_memory=True, **DIMS)
    return _dbs[pano, cand]


def datasets(db, task):
    """-> (the host dataset, its index-only twin) of `task` over `db`, same constructor arguments"""
    from vln_hamt_amd import data as D
    args = {"mlm": (), "itm": (), "mrc": (MRC_PROB,)}.get(task, (KILL_V, KILL_A))
    host = {"mlm": D.MlmDataset, "mrc": D.MrcDataset, "itm": D.ItmDataset, "sap": D.SapDataset, "sar": D.SarDataset, "sprel": D.SprelDataset}[task]
    return host(db, TOK, *args), D.INDEX_DATASETS[task](db, TOK, *args)


def draw(ds, idxs, seed):
    """the items of one batch under one seed of python's and numpy's streams -> (items, the streams' end states)"""
    random.seed(seed)
    np.random.seed(seed)
    items = [ds[i] for i in idxs]
    return items, (random.getstate(), np.random.get_state())


def same_state(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def numpy_unpack(pb):
    """the collated batch of a PackedBatch, read off its host buffer: rows padded per family, masks and lengths, per-sample fields"""
    raw = pb.buf.numpy()
    out = dict(pb.lists)
    pre = {f: raw[o:o + 4 * (pb.B + 1)].view(np.int32) for f, o in pb.prefix_off.items()}
    for name, (off, row_shape, dtype, fam, pad) in pb.fields.items():
        if pb.hist_none and name in HIST_FIELDS:
            out[name] = None
            continue
        npdt = torch.empty((), dtype=dtype).numpy().dtype
        rows, maxlen, n_row = int(pre[fam][-1]), max(pb.lens[fam]), int(np.prod(row_shape, dtype=np.int64))
        src = raw[off:off + rows * n_row * npdt.itemsize].view(npdt).reshape((rows,) + tuple(row_shape))
        dst = np.frombuffer(bytes([pad]) * (pb.B * maxlen * n_row * npdt.itemsize), dtype=npdt).reshape((pb.B, maxlen) + tuple(row_shape)).copy()
        for b in range(pb.B):
            dst[b, :pb.lens[fam][b]] = src[pre[fam][b]:pre[fam][b + 1]]
        out[name] = dst
    for fam, add in (("txt", 0), ("hist", 1), ("ob", 0)):
        if fam in pb.lens:
            lens = np.asarray(pb.lens[fam], dtype=np.int64) + add
            out[f"{fam}_masks"], out[f"{fam}_lens"] = np.arange(lens.max())[None] < lens[:, None], lens
    for name, (off, shape, dtype) in pb.per_sample.items():
        npdt = torch.empty((), dtype=dtype).numpy().dtype
        out[name] = raw[off:off + int(np.prod(shape)) * npdt.itemsize].view(npdt).reshape(shape).copy()
    return out


def gather_ref(tb, recs, task, layout, hist_pano, Hmax=None, Omax=None, hist_none=None, has_ob=None):
    """`hamt_pretrain_gather` restated: `tb` = {name: numpy table} (build_pretrain_tables' names), `recs` int32 [B, 8] -> (the batch's
    fields beyond the text, the number of refused records).  Hmax / Omax / hist_none: as IndexedBatch derives them, from the records.
    `has_ob`: whether the launch carries observation outputs (then a record also reaches its observed step), default by `task`."""
    recs = np.asarray(recs)
    B, (NV, _, F), A, NS = recs.shape[0], tb["feat"].shape, tb["ang36"].shape[-1], tb["step_idx"].shape[0]
    C = tb["cand_view"].shape[1]
    P = 0 if tb.get("prob") is None else tb["prob"].shape[-1]
    reach_ob = task in OB_TASKS if has_ob is None else has_ob
    has_ob = task in OB_TASKS
    if hist_none is None:
        hist_none = has_ob and int(recs[:, 1].max()) == 0
    Hmax = (0 if hist_none else int(recs[:, 1].max())) if Hmax is None else Hmax
    Omax = (int(recs[:, 5].max()) if has_ob else 0) if Omax is None else Omax
    o = {}
    if not hist_none:
        o["hist_img_fts"], o["hist_ang_fts"] = np.zeros((B, Hmax, F), np.float32), np.zeros((B, Hmax, A), np.float32)
        if hist_pano:
            o["hist_pano_img_fts"], o["hist_pano_ang_fts"] = np.zeros((B, Hmax, 36, F), np.float32), np.zeros((B, Hmax, 36, A), np.float32)
    else:
        o.update({k: None for k in HIST_FIELDS if hist_pano or "pano" not in k})
    if task == "mrc":
        o["hist_img_probs"], o["hist_mrc_masks"] = np.zeros((B, Hmax, P), np.float32), np.zeros((B, Hmax), bool)
    o["hist_masks"], o["hist_lens"] = np.zeros((B, Hmax + 1), bool), np.zeros(B, np.int64)
    if has_ob:
        o.update(ob_img_fts=np.zeros((B, Omax, F), np.float32), ob_ang_fts=np.zeros((B, Omax, A), np.float32), ob_nav_types=np.zeros((B, Omax), np.int64),
                 ob_masks=np.zeros((B, Omax), bool), ob_lens=np.zeros(B, np.int64))
        if task == "sap":
            o["ob_action_viewindex"] = np.zeros(B, np.int64)
        elif task == "sar":
            o["ob_action_angles"], o["ob_progress"] = np.zeros((B, 2), np.float32), np.zeros(B, np.float32)
        else:
            o["sp_anchor_idxs"], o["sp_targets"] = np.zeros(B, np.int64), np.zeros((B, 36, 2), np.float32)
    bad = 0
    for b in range(B):
        base, t, flags, mrc, anchor = (int(x) for x in recs[b, :5])
        steps = range(base, base + t + (1 if reach_ob else 0))
        ok = base >= 0 and 0 <= t <= min(Hmax, 32) and base + len(steps) <= NS and (task != "sprel" or 0 <= anchor < 36)
        ok = ok and all(0 <= tb["step_idx"][s, 0] < NV and 0 <= tb["step_idx"][s, 1] < 36 for s in steps)
        if not ok:
            bad += 1
            o["hist_masks"][b, 0], o["hist_lens"][b] = True, 1
            continue
        o["hist_masks"][b, :t + 1], o["hist_lens"][b] = True, t + 1
        for s in range(t):
            row, view = tb["step_idx"][base + s, :2]
            masked = bool((mrc >> s) & 1)
            o["hist_ang_fts"][b, s] = tb["step_val"][base + s, :A]
            if not masked:
                o["hist_img_fts"][b, s] = tb["feat"][row, view]
            if hist_pano:
                o["hist_pano_ang_fts"][b, s] = tb["ang36"][view]
                if not masked:
                    o["hist_pano_img_fts"][b, s] = tb["feat"][row]
            if task == "mrc":
                o["hist_img_probs"][b, s], o["hist_mrc_masks"][b, s] = tb["prob"][row, view], masked
        if not has_ob:
            continue
        cur = base + t
        row, view = tb["step_idx"][cur, :2]
        n = min(max(int(tb["cand_cnt"][row]), 0), C)
        cviews = [min(max(int(v), 0), 35) for v in tb["cand_view"][row, :n]]
        if layout == 0:                                   # the 36 views, then STOP
            img = [tb["feat"][row, v] for v in range(36)] + [np.zeros(F, np.float32)]
            ang = [tb["ang36"][view, v] for v in range(36)] + [np.zeros(A, np.float32)]
            nav = [1 if v in cviews else 0 for v in range(36)] + [2]
        else:                                             # candidates, STOP, the views no candidate points to
            rest = [v for v in range(36) if v not in cviews]
            img = [tb["feat"][row, v] for v in cviews] + [np.zeros(F, np.float32)] + [tb["feat"][row, v] for v in rest]
            ang = [tb["cand_ang"][row, c, view % 12] for c in range(n)] + [np.zeros(A, np.float32)] + [tb["ang36"][view, v] for v in rest]
            nav = [1] * n + [2] + [0] * len(rest)
        ln = min(len(nav), Omax)
        o["ob_lens"][b], o["ob_masks"][b, :ln], o["ob_nav_types"][b, :ln] = ln, True, nav[:ln]
        if not flags & 1:
            o["ob_img_fts"][b, :ln] = np.stack(img[:ln])
        if not flags & 2:
            o["ob_ang_fts"][b, :ln] = np.stack(ang[:ln])
        if task == "sap":
            o["ob_action_viewindex"][b] = tb["step_idx"][cur, 2 + layout]
        elif task == "sar":
            o["ob_action_angles"][b], o["ob_progress"][b] = tb["step_val"][cur, A + 2 * layout:A + 2 * layout + 2], tb["step_val"][cur, A + 4]
        else:
            o["sp_anchor_idxs"][b], o["sp_targets"][b] = anchor, tb["sp_targets"][anchor]
    return o, bad


def restate(tb, pb):
    """the whole batch an IndexedBatch stands for: its text read off the buffer, the rest restated from the tables and its records"""
    out = numpy_unpack(pb)
    rest, bad = gather_ref(tb, pb.host_records(), pb.task, pb.layout, pb.hist_pano, hist_none=pb.hist_none)
    assert bad == 0
    out.update(rest)
    return out


def assert_same_batch(got, want, what=""):
    """key for key: None-ness, dtype, shape, bits (`got` / `want`: numpy arrays or tensors)"""
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if w is None or isinstance(w, list):
            assert g == w if isinstance(w, list) else g is None, (what, k)
            continue
        g = np.ascontiguousarray(g.cpu().numpy() if torch.is_tensor(g) else g)
        w = np.ascontiguousarray(w.cpu().numpy() if torch.is_tensor(w) else w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint8) if g.dtype != bool else g, w.view(np.uint8) if w.dtype != bool else w), (what, k)
