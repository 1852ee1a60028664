"""The six proxy-task datasets, index only: what `data/r2r_tasks.py`'s datasets decide per sample, without a feature read.

An item is the instruction (`txt_ids`, and `txt_labels` for MLM) plus ONE int32 record of `device_store.RECORD_WORDS` words -- the first
step row of the trajectory, the history length, the kill flags, the MRC mask, the SPREL anchor, the observation's length -- from which
`hamt_pretrain_gather` builds the sample on the device out of a `PretrainStore` (data/device_store.py).  Each class takes the constructor
arguments of its host twin and draws from python's `random` and numpy's global stream exactly what the twin draws, in the twin's order,
so equal seeds give equal batches (tests/test_device_batches.py pins the streams' end states against the host datasets):

  MLM    `random_word` over the instruction
  MRC    n x `np.random.rand()`, then `np.random.randint(n)` if no view was picked
  SAP / SAR / SPREL   `random.random()` for random_kill_v, then, if the views survive, `random.random()` for random_kill_a
  SPREL  then `np.random.randint(36)`

A dataset keeps host index tables only (`device_store.pretrain_index`): DataLoader workers never pickle a device tensor.  The store is
found at `to_device` time through the id `PretrainStore(nav_db, device)` left on `nav_db`.
"""
from __future__ import annotations

import random

import numpy as np
import torch
from torch.utils.data import Dataset

from . import device_store as S
from .r2r_tasks import random_word


class _IndexDataset(Dataset):
    task = ""
    per_step = has_ob = False

    def __init__(self, nav_db, tok):
        self.nav_db, self.tok = nav_db, tok
        self.cls_token_id, self.sep_token_id, self.pad_token_id = tok.cls_token_id, tok.sep_token_id, tok.pad_token_id
        index = S.pretrain_index(nav_db)
        self.traj_base, self.ob_len = index["traj_base"], index["ob_len"]

    def __len__(self):
        return len(self.nav_db.traj_step_refer if self.per_step else self.nav_db.traj_refer)

    def _layout(self):
        return int(bool(self.nav_db.ob_cand_pano_view))

    def _item(self, i):
        """-> (instruction tokens, item with its record: base, history length and observation length set, nothing drawn yet)"""
        n, j, t = (self.nav_db.traj_step_refer if self.per_step else self.nav_db.traj_refer)[i]
        rec = np.zeros(S.RECORD_WORDS, np.int32)
        rec[S.REC_BASE], rec[S.REC_T] = self.traj_base[n], t
        layout = self._layout() if self.has_ob else 0
        if self.has_ob:
            rec[S.REC_OB_LEN] = self.ob_len[self.traj_base[n] + t, layout]
        item = {"record": rec, "hist_lens": int(t), "layout": layout, "hist_pano": bool(self.nav_db.hist_enc_pano),
                "store": getattr(self.nav_db, "device_store_id", None)}
        return self.nav_db.traj_data[n]["instr_encodings"][j][:self.nav_db.max_txt_len], item

    @staticmethod
    def _text(tokens, item):
        item["txt_ids"] = torch.LongTensor(tokens)
        item["txt_lens"] = item["txt_ids"].size(0)

    def _kills(self, item):
        seen = True
        if random.random() < self.random_kill_v:
            item["record"][S.REC_FLAGS] |= S.KILL_V
            seen = False
        if seen and random.random() < self.random_kill_a:
            item["record"][S.REC_FLAGS] |= S.KILL_A

    def __getitem__(self, i):
        tokens, item = self._item(i)
        self._text(tokens, item)
        return item


class MlmIndexDataset(_IndexDataset):
    task = "mlm"

    def __init__(self, nav_db, tok):
        super().__init__(nav_db, tok)
        self.vocab_range = [1996, 29611]
        self.mask_token_id = tok.mask_token_id

    def __getitem__(self, i):
        tokens, item = self._item(i)
        ids, labels = random_word(tokens, self.vocab_range, self.mask_token_id)
        item["txt_ids"], item["txt_labels"] = torch.LongTensor(ids), torch.LongTensor(labels)
        item["txt_lens"] = item["txt_ids"].size(0)
        return item


class MrcIndexDataset(_IndexDataset):
    task = "mrc"

    def __init__(self, nav_db, tok, mask_prob):
        super().__init__(nav_db, tok)
        self.mask_prob = mask_prob

    def __getitem__(self, i):
        tokens, item = self._item(i)
        self._text(tokens, item)
        n = item["hist_lens"]
        picked = [np.random.rand() < self.mask_prob for _ in range(n)]
        if not any(picked):
            picked[np.random.randint(n)] = True
        item["record"][S.REC_MRC] = np.array(sum(1 << s for s, p in enumerate(picked) if p), np.uint32).astype(np.int32)
        return item


class ItmIndexDataset(_IndexDataset):
    task = "itm"


class SapIndexDataset(_IndexDataset):
    task = "sap"
    per_step = has_ob = True

    def __init__(self, nav_db, tok, random_kill_v, random_kill_a):
        super().__init__(nav_db, tok)
        self.random_kill_v, self.random_kill_a = random_kill_v, random_kill_a

    def __getitem__(self, i):
        tokens, item = self._item(i)
        self._text(tokens, item)
        self._kills(item)
        return item


class SarIndexDataset(SapIndexDataset):
    task = "sar"


class SprelIndexDataset(SapIndexDataset):
    task = "sprel"

    def _layout(self):
        return 0                                    # always the 36 + STOP layout (SprelDataset: ob_cand_pano_view=False)

    def __getitem__(self, i):
        item = super().__getitem__(i)
        item["record"][S.REC_ANCHOR] = np.random.randint(36)
        return item


INDEX_DATASETS = {"mlm": MlmIndexDataset, "mrc": MrcIndexDataset, "itm": ItmIndexDataset, "sap": SapIndexDataset, "sar": SarIndexDataset,
                  "sprel": SprelIndexDataset}
