"""The six proxy-task datasets and `*_image_collate` functions of the image-input pipeline behind the reference's names
(pretrain_src/data/image_tasks.py).  The datasets are the feature-input ones (data/r2r_tasks.py) with the history / observation
builders swapped: the same text, angle, label keys from the same random draws in the same order, and per view a parameter record
instead of a feature row (data/image_data.py).  The collates return a `PackedImageBatch`: the usual packed ragged fields, then --
in the SAME pinned buffer -- the parameter table of every output slot and the uint8 panoramas the records point at; `to_device`
makes the one H2D copy, runs the unpack kernels and `hamt_image_prep` per image key, and yields the dict of the reference's collates:
`hist_images` (B, Tmax, 3, 224, 224), `hist_pano_images` (B, Tmax, 36, 3, 224, 224), `ob_images` (B, 36, 3, 224, 224) zero padded
(image_tasks.py:61-69), `ob_v_exists`, `None` history when every sample is at step 0 (and `hist_ang_fts`, which the reference
misspells there, :227).  With `image_layout="patches"` the three image keys are `PatchRows` holders: the rows of the patch-embedding
GEMM, the fp32 images are never written.
"""
from __future__ import annotations

import random
from typing import Dict, List

import numpy as np
import torch

from . import r2r_tasks as R
from .collate import _ALIGN, PackedBatch, _pack, _rup
from .image_data import N_VIEWS
from .image_prep import PATCH_K, PATCHES_PER_VIEW, image_prep
from .image_transform import IMGSIZE, VIEW_DTYPE

IMAGE_KEYS = ("hist_images", "hist_pano_images", "ob_images")


class _ImageInputs:
    """history / observation builders over `MultiStepNavImageData.get_input`; mixed in front of the feature-input datasets"""

    @staticmethod
    def _history(inputs, out):
        out["hist_images"] = inputs["hist_images"]
        out["hist_ang_fts"] = torch.from_numpy(inputs["hist_ang_fts"])
        out["hist_pano_images"] = inputs["hist_pano_images"]
        out["hist_pano_ang_fts"] = torch.from_numpy(inputs["hist_pano_ang_fts"])
        out["hist_lens"] = inputs["hist_lens"]
        out["image_views"] = inputs["image_views"]

    def _observation(self, inputs, out):
        """image_tasks.py:178-189: the views are killed with probability random_kill_v; only if they survive is the angle kill drawn"""
        out["ob_images"] = inputs["ob_images"].copy()
        v_exists = True
        if random.random() < self.random_kill_v:
            out["ob_images"]["zero"] = 1
            v_exists = False
        out["ob_v_exists"] = v_exists
        out["ob_ang_fts"] = torch.from_numpy(inputs["ob_ang_fts"])
        if v_exists and random.random() < self.random_kill_a:
            out["ob_ang_fts"][...] = 0
        out["ob_nav_types"] = torch.LongTensor(inputs["ob_nav_types"])
        out["ob_lens"] = out["ob_images"].shape[0] + 1          # STOP


class MlmImageDataset(_ImageInputs, R.MlmDataset):
    pass


class ItmImageDataset(_ImageInputs, R.ItmDataset):
    pass


class SapImageDataset(_ImageInputs, R.SapDataset):
    pass


class SarImageDataset(_ImageInputs, R.SarDataset):
    pass


class SprelImageDataset(_ImageInputs, R.SprelDataset):
    pass


class MrcImageDataset(_ImageInputs, R.MrcDataset):
    """image_tasks.py:81-117: the views are NOT masked here -- the model zero-fills the features of the masked steps after the
    backbone (image_vilmodel.py:84-86)"""

    def __getitem__(self, i):
        inputs, out = self._inputs(i), {}
        self._text(inputs, out)
        n = inputs["hist_img_probs"].shape[0]
        picked = [np.random.rand() < self.mask_prob for _ in range(n)]          # mrc.py `_get_img_mask`, as R.MrcDataset draws it
        if not any(picked):
            picked[np.random.randint(n)] = True
        out["hist_img_probs"] = torch.from_numpy(inputs["hist_img_probs"])
        out["hist_mrc_masks"] = torch.tensor(picked)
        self._history(inputs, out)
        return out


class PackedImageBatch(PackedBatch):
    """`image`: key -> (record offset, slots, leading shape); `views_off` / `n_src` / `view_hw`: the shipped uint8 views."""

    image: Dict[str, tuple] = {}
    views_off = n_src = 0
    view_hw = (0, 0)

    def host_records(self, key) -> np.ndarray:
        off, n, _ = self.image[key]
        return self.buf.numpy()[off:off + n * VIEW_DTYPE.itemsize].view(VIEW_DTYPE)

    def host_views(self) -> np.ndarray:
        H, W = self.view_hw
        return self.buf.numpy()[self.views_off:self.views_off + self.n_src * H * W * 3].reshape(self.n_src, H, W, 3)

    def _unpack_extra(self, dbuf, device, res, out, image_layout="nchw", patch_dtype=torch.float32):
        H, W = self.view_hw
        src = dbuf[self.views_off:self.views_off + self.n_src * H * W * 3].view(self.n_src, H, W, 3)
        for key, (off, n, lead) in self.image.items():
            if self.hist_none and key != "ob_images":
                res[key] = None
                continue
            recs_dev = dbuf[off:off + n * VIEW_DTYPE.itemsize]
            if image_layout == "patches":
                res[key] = image_prep(src, self.host_records(key), recs_dev, "patches", dtype=patch_dtype, ldy=PATCH_K,
                                      Rpad=_rup(n * PATCHES_PER_VIEW, 64), lead=lead)
                continue
            shape = tuple(lead) + (3, IMGSIZE, IMGSIZE)
            t = out.get(key) if out is not None else None
            if not (t is not None and tuple(t.shape) == shape and t.dtype == torch.float32 and t.device == device and t.is_contiguous()):
                t = torch.empty(shape, dtype=torch.float32, device=device)
            image_prep(src, self.host_records(key), recs_dev, "nchw", out=t)
            res[key] = t


def _pack_images(task: str, inputs: List[dict]) -> PackedImageBatch:
    B = len(inputs)
    hist = [int(x["hist_lens"]) for x in inputs]
    Tmax = max(hist)
    has_ob = "ob_images" in inputs[0]
    blocks0 = next((x["image_views"][0] for x in inputs if x["image_views"]), None)
    H, W = (blocks0.shape[1], blocks0.shape[2]) if blocks0 is not None else (1, 1)
    # which panoramas cross PCIe: every history block, the observation's unless it was killed
    base, n_src = [], 0                       # per sample: first shipped view index of each of its blocks (-1: not shipped)
    for x, T in zip(inputs, hist):
        b = []
        for j in range(len(x["image_views"])):
            ship = j < T or not bool(x["ob_images"]["zero"].all())
            b.append(n_src if ship else -1)
            n_src += N_VIEWS if ship else 0
        base.append(b)
    slots = {"hist_images": (B * Tmax, (B, Tmax)), "hist_pano_images": (B * Tmax * N_VIEWS, (B, Tmax, N_VIEWS))}
    if has_ob:
        slots["ob_images"] = (B * N_VIEWS, (B, N_VIEWS))
    rec_bytes = {k: _rup(n * VIEW_DTYPE.itemsize) for k, (n, _) in slots.items()}
    tail = sum(rec_bytes.values()) + _rup(n_src * H * W * 3) + _ALIGN
    pb = _pack(task, inputs, skip=IMAGE_KEYS + ("image_views",), tail_bytes=tail, cls=PackedImageBatch)
    raw = pb.buf.numpy()
    off, pb.image = pb.tail_off, {}
    for k, (n, lead) in slots.items():
        pb.image[k] = (off, n, lead)
        recs = raw[off:off + n * VIEW_DTYPE.itemsize].view(VIEW_DTYPE).reshape(lead)
        recs[...] = np.zeros((), VIEW_DTYPE)
        recs["src"], recs["zero"] = -1, 1                     # padded steps: written as 0.0
        for i, (x, T) in enumerate(zip(inputs, hist)):
            r = x[k]
            L_ = T if k != "ob_images" else N_VIEWS
            if L_ == 0:
                continue
            recs[i, :L_] = r
            blk = r["src"] // N_VIEWS                              # sample-local block -> index among the shipped views
            b = np.asarray(base[i], dtype=np.int64)[blk]
            recs[i, :L_]["src"] = np.where(b >= 0, b + r["src"] % N_VIEWS, -1)
        off += rec_bytes[k]
    pb.views_off, pb.n_src, pb.view_hw = off, n_src, (H, W)
    dst = raw[off:off + n_src * H * W * 3].reshape(n_src, H, W, 3)
    for x, b in zip(inputs, base):
        for blk, s in zip(x["image_views"], b):
            if s >= 0:
                dst[s:s + N_VIEWS] = blk                      # the one host copy of the payload (from the store's memory map)
    return pb


def mlm_image_collate(inputs):
    return _pack_images("mlm", inputs)


def mrc_image_collate(inputs):
    return _pack_images("mrc", inputs)


def itm_image_collate(inputs):
    return _pack_images("itm", inputs)


def sap_image_collate(inputs):
    return _pack_images("sap", inputs)


def sar_image_collate(inputs):
    return _pack_images("sar", inputs)


def sprel_image_collate(inputs):
    return _pack_images("sprel", inputs)


IMAGE_COLLATE = {"mlm": mlm_image_collate, "mrc": mrc_image_collate, "itm": itm_image_collate, "sap": sap_image_collate,
                 "sar": sar_image_collate, "sprel": sprel_image_collate}
