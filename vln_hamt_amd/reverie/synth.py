"""Synthetic REVERIE decision inputs with the agent's conventions (finetune reverie/agent.py:77-139, 229), drawn from a numpy PCG64
stream so that the same call gives the same tensors on any host (the golden generator and the tests both rebuild them here):

* text: [CLS] ... [SEP] ids with ragged lengths, bool masks;
* history: `hist_steps` per-step image / angle / panorama features;
* observation: `n_views` candidate rows, navigable ones (nav type 1) first, the STOP row (type 2) after them, padding (type 0, mask
  False) at the end;
* objects: `obj_lens[i]` objects per viewpoint, n = max(max(obj_lens), 1) rows, a viewpoint without objects contributes ONE all-zero
  row whose mask is True (agent.py:126); the angles are the last 4 columns of one [B, n, obj_feat_size + 4] array, as the agent slices
  them (agent.py:136-137) -- row-strided views -- and the poses are [B, n, 5]."""
from __future__ import annotations

import numpy as np
import torch


def _angles(rng, shape):
    h = rng.uniform(-np.pi, np.pi, size=shape).astype(np.float32)
    e = rng.uniform(-np.pi / 6, np.pi / 6, size=shape).astype(np.float32)
    return np.stack([np.sin(h), np.cos(h), np.sin(e), np.cos(e)], -1).astype(np.float32)


def make_inputs(seed, B, txt_len, n_views, obj_lens, image_feat_size, obj_feat_size, hist_steps=3, vocab_size=1000, n_pano=36):
    rng = np.random.Generator(np.random.PCG64(seed))
    assert len(obj_lens) == B
    lens = rng.integers(max(2, txt_len // 2), txt_len + 1, size=B)
    lens[0] = txt_len
    ids = np.zeros((B, txt_len), dtype=np.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(1000 if vocab_size > 2000 else 3, vocab_size, size=n)
        ids[i, 0], ids[i, n - 1] = 101 % vocab_size, 102 % vocab_size
    txt_masks = np.arange(txt_len)[None] < lens[:, None]
    feat = lambda *s: np.maximum(rng.standard_normal(size=s, dtype=np.float32), 0.0).astype(np.float32)    # post-ReLU features
    hist = dict(img=feat(hist_steps, B, image_feat_size), ang=_angles(rng, (hist_steps, B)),
                pano_img=feat(hist_steps, B, n_pano, image_feat_size), pano_ang=_angles(rng, (hist_steps, B, n_pano)))
    ob_lens = rng.integers(2, n_views + 1, size=B)
    ob_lens[0] = n_views
    ob_img, ob_ang = feat(B, n_views, image_feat_size), _angles(rng, (B, n_views))
    nav = np.zeros((B, n_views), dtype=np.int64)
    for i, n in enumerate(ob_lens):
        ob_img[i, n:] = 0.0
        ob_ang[i, n:] = 0.0
        nav[i, :n - 1] = 1
        nav[i, n - 1] = 2                      # STOP (zero features, agent.py:110-114)
        ob_img[i, n - 1] = 0.0
        ob_ang[i, n - 1] = 0.0
    ob_masks = np.arange(n_views)[None] < ob_lens[:, None]
    n_obj = max(max(obj_lens), 1)
    obj_full = np.zeros((B, n_obj, obj_feat_size + 4), dtype=np.float32)
    obj_poses = np.zeros((B, n_obj, 5), dtype=np.float32)
    for i, n in enumerate(obj_lens):
        if n > 0:
            obj_full[i, :n, :obj_feat_size] = feat(n, obj_feat_size)
            obj_full[i, :n, obj_feat_size:] = _angles(rng, (n,))
            box = rng.uniform(0.0, 1.0, size=(n, 4)).astype(np.float32)
            obj_poses[i, :n, :4] = box
            obj_poses[i, :n, 4] = box[:, 2] * box[:, 3]
    obj_masks = np.arange(n_obj)[None] < np.maximum(np.asarray(obj_lens), 1)[:, None]
    full = torch.from_numpy(obj_full)
    t = torch.from_numpy
    return dict(txt_ids=t(ids), txt_masks=t(txt_masks), hist_img_feats=t(hist["img"]), hist_ang_feats=t(hist["ang"]),
                hist_pano_img_feats=t(hist["pano_img"]), hist_pano_ang_feats=t(hist["pano_ang"]),
                ob_img_feats=t(ob_img), ob_ang_feats=t(ob_ang), ob_nav_types=t(nav), ob_masks=t(ob_masks),
                obj_feats=full[..., :obj_feat_size], obj_angles=full[..., obj_feat_size:], obj_poses=t(obj_poses), obj_masks=t(obj_masks))


def targets(inp, seed):
    """(action target, object target) per sample as the agent's teacher gives them (agent.py:141-163): a navigable view or STOP,
    an object index -- or -100 (ignored); the viewpoint without objects always has the object target -100"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nav, om = inp["ob_nav_types"].numpy(), inp["obj_masks"].numpy()
    B = nav.shape[0]
    act = np.array([rng.choice(np.flatnonzero(nav[i] > 0)) for i in range(B)], dtype=np.int64)
    objs = inp["obj_feats"].abs().sum(-1).numpy() > 0
    ref = np.array([rng.choice(np.flatnonzero(objs[i])) if objs[i].any() else -100 for i in range(B)], dtype=np.int64)
    act[-1] = -100
    assert all(om[i, ref[i]] for i in range(B) if ref[i] >= 0)
    return torch.from_numpy(act), torch.from_numpy(ref)

