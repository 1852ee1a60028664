"""Collation of the index-only datasets (data/device_tasks.py): the `*_index_collate` functions return an `IndexedBatch`, a `PackedBatch`
whose byte buffer holds the instruction tokens (packed as ever: `txt_labels`' 0xFF pad and the `text_pack` plan included) and one 32-byte
record per sample -- a few KiB where the host pipeline ships tens of MiB.  `to_device` is the parent's: one H2D copy, the text unpack
kernels, and then, through the subclass hook, ONE `hamt_pretrain_gather` launch (ops.pretrain_gather) that writes every other field of
the batch from the `PretrainStore` the items name.  The result is the dict `PackedBatch.to_device` returns for the host pipeline's batch
of the same samples: same keys, shapes, dtypes and bits, `None` for the four history fields when every sample is at step 0.  `Hmax` and
`Omax` come from the records on the host; nothing is read back from the device.  `move_to_cuda`, `PrefetchLoader`, `MetaLoader` and
`build_dataloader` take these batches as they take any `PackedBatch`.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from .. import _lib as L
from .. import ops
from . import device_store as S
from .collate import HIST_FIELDS, PackedBatch, _pack, _rup

_ITEM_ONLY = ("record", "store", "layout", "hist_pano")
_OB_TASKS = ("sap", "sar", "sprel")
_LABELS = {"sap": ("ob_action_viewindex",), "sar": ("ob_action_angles", "ob_progress"), "sprel": ("sp_anchor_idxs", "sp_targets")}


class IndexedBatch(PackedBatch):
    """`records_off`: where the int32 [B, 8] records sit in the buffer; `store_id`, `layout`, `hist_pano`: which `PretrainStore` the batch is
    gathered from, the observation layout of its task (device_store.LAYOUTS) and whether the history carries whole panoramas;
    `hist_lens`: the samples' history lengths."""

    records_off = layout = 0
    store_id = None
    hist_pano = True
    hist_lens: List[int] = []

    def host_records(self) -> np.ndarray:
        n = self.B * S.RECORD_WORDS * 4
        return self.buf.numpy()[self.records_off:self.records_off + n].view(np.int32).reshape(self.B, S.RECORD_WORDS)

    def _unpack_extra(self, dbuf, device, res, out, **extra):
        if extra:
            raise TypeError(f"IndexedBatch.to_device: unexpected arguments {sorted(extra)}")
        store = S.get_store(self.store_id)
        if store.device != device:
            raise L.HamtError(f"IndexedBatch.to_device: the batch goes to {device}, its PretrainStore is on {store.device}")
        B, F, A, P, task = self.B, store.F, store.A, store.P, self.task
        recs = self.host_records()
        Hmax = 0 if self.hist_none else max(self.hist_lens)
        has_ob = task in _OB_TASKS
        Omax = int(recs[:, S.REC_OB_LEN].max()) if has_ob else 0
        shapes = {}
        if not self.hist_none:
            shapes["hist_img_fts"], shapes["hist_ang_fts"] = (torch.float32, (B, Hmax, F)), (torch.float32, (B, Hmax, A))
            if self.hist_pano:
                shapes["hist_pano_img_fts"], shapes["hist_pano_ang_fts"] = (torch.float32, (B, Hmax, S.VIEWS, F)), (torch.float32, (B, Hmax, S.VIEWS, A))
        if task == "mrc":
            shapes["hist_img_probs"], shapes["hist_mrc_masks"] = (torch.float32, (B, Hmax, P)), (torch.bool, (B, Hmax))
        shapes["hist_masks"], shapes["hist_lens"] = (torch.bool, (B, Hmax + 1)), (torch.int64, (B,))
        if has_ob:
            shapes.update(ob_img_fts=(torch.float32, (B, Omax, F)), ob_ang_fts=(torch.float32, (B, Omax, A)), ob_nav_types=(torch.int64, (B, Omax)),
                          ob_masks=(torch.bool, (B, Omax)), ob_lens=(torch.int64, (B,)))
            label = {"ob_action_viewindex": (torch.int64, (B,)), "ob_action_angles": (torch.float32, (B, 2)), "ob_progress": (torch.float32, (B,)),
                     "sp_anchor_idxs": (torch.int64, (B,)), "sp_targets": (torch.float32, (B, S.VIEWS, 2))}
            shapes.update({k: label[k] for k in _LABELS[task]})
        outs = {}
        for name, (dtype, shape) in shapes.items():
            t = out.get(name) if out is not None else None
            if not (t is not None and tuple(t.shape) == shape and t.dtype == dtype and t.device == device and t.is_contiguous()):
                t = torch.empty(shape, dtype=dtype, device=device)
            outs[name] = t
        n = B * S.RECORD_WORDS * 4
        ops.pretrain_gather(store, dbuf[self.records_off:self.records_off + n].view(torch.int32).view(B, S.RECORD_WORDS), outs, Hmax, Omax, self.layout)
        if self.hist_none:
            for name in HIST_FIELDS:
                if self.hist_pano or "pano" not in name:
                    res[name] = None
        res.update(outs)


def _index_pack(task: str, inputs: List[dict]) -> IndexedBatch:
    B = len(inputs)
    pb = _pack(task, inputs, skip=_ITEM_ONLY, tail_bytes=_rup(B * S.RECORD_WORDS * 4), cls=IndexedBatch)
    pb.hist_lens = pb.lens.pop("hist")              # the text alone goes through the parent's unpack; the gather writes hist_masks / hist_lens
    x0 = inputs[0]
    pb.records_off, pb.store_id, pb.layout, pb.hist_pano = pb.tail_off, x0["store"], int(x0["layout"]), bool(x0["hist_pano"])
    if any(x["store"] != pb.store_id for x in inputs):
        raise L.HamtError("index collate: the items of one batch name different stores")
    pb.host_records()[...] = np.stack([x["record"] for x in inputs], 0)
    return pb


def mlm_index_collate(inputs):
    return _index_pack("mlm", inputs)


def mrc_index_collate(inputs):
    return _index_pack("mrc", inputs)


def itm_index_collate(inputs):
    return _index_pack("itm", inputs)


def sap_index_collate(inputs):
    return _index_pack("sap", inputs)


def sar_index_collate(inputs):
    return _index_pack("sar", inputs)


def sprel_index_collate(inputs):
    return _index_pack("sprel", inputs)


INDEX_COLLATE = {"mlm": mlm_index_collate, "mrc": mrc_index_collate, "itm": itm_index_collate, "sap": sap_index_collate,
                 "sar": sar_index_collate, "sprel": sprel_index_collate}
