"""The validation half of the proxy-task pretraining loop (``pretrain_src/main_r2r.py:319-511``) behind the reference's names:

    from vln_hamt_amd.validate import validate
    validate(model, val_dataloaders, setname='_unseen')

Per batch there is one ``model(batch, task, compute_loss=False)`` under ``torch.no_grad()`` and one ``ops.eval_*`` call, which adds the
batch's loss sum and counts into accumulators on the device (csrc/eval.hip).  Nothing comes back to the host inside the loop -- no
``.item()``, no boolean indexing when the batch carries its index lists (``txt_label_idx``, ``hist_mrc_idx``) -- and the one read after the
last batch is the pass's only synchronisation; the throughput keys are timed across it.  The returned dicts carry the reference's keys
and normalisations.  Across ranks every rank's totals are gathered and summed in rank order, as ``sum(all_gather(x))`` does.
"""
from __future__ import annotations

import logging
import time

import torch

from . import ops

LOGGER = logging.getLogger(__name__)

__all__ = ["validate", "validate_mlm", "validate_sap", "validate_sar", "validate_sprel", "validate_mrc", "validate_itm",
           "compute_accuracy_for_soft_targets", "combine_totals"]


# ------------------------------------------------------------------------------------------ totals of one pass
def combine_totals(rank_totals):
    """`rank_totals`: one (sums, counts) pair per rank, in rank order -- lists of floats and of ints.  Returns their element-wise
    sums, added left to right from 0 as the reference's ``sum(all_gather(x))`` adds them (a pure function: no process group needed)."""
    rank_totals = list(rank_totals)
    if not rank_totals:
        raise ValueError("combine_totals: no rank totals")
    ns, nc = len(rank_totals[0][0]), len(rank_totals[0][1])
    sums, counts = [0.0] * ns, [0] * nc
    for s, c in rank_totals:
        if len(s) != ns or len(c) != nc:
            raise ValueError("combine_totals: ranks disagree on the number of totals")
        sums = [a + float(b) for a, b in zip(sums, s)]
        counts = [a + int(b) for a, b in zip(counts, c)]
    return sums, counts


def gather_totals(sums, counts, device=None):
    """this rank's totals -> the rank-ordered sum over all ranks (unchanged without an initialised process group of more than one rank).
    The exchange is one all_gather of a float64 and one of an int64 tensor: CPU tensors under gloo, device tensors under nccl."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return list(sums), list(counts)
    where = torch.device("cpu")
    if str(dist.get_backend()).lower() == "nccl":
        where = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    world = dist.get_world_size()
    mine = (torch.tensor(list(sums), dtype=torch.float64, device=where), torch.tensor(list(counts), dtype=torch.int64, device=where))
    got = []
    for t in mine:
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
        got.append([p.cpu().tolist() for p in parts])
    return combine_totals(list(zip(got[0], got[1])))


class _Pass:
    """the accumulator of one validate_* pass, made on the device of the first batch's scores, and the host-side row count"""

    def __init__(self):
        self.acc = None
        self.rows = 0                       # rows counted on the host from shapes (scores.size(0)): no synchronisation
        self.start = time.time()

    def on(self, device):
        if self.acc is None:
            self.acc = ops.EvalAccumulator(device)
        return self.acc

    def finish(self):
        """-> (sums, counts, rows, seconds): the one read of the pass, then the exchange between ranks"""
        if self.acc is None:
            sums, counts, dev = [0.0] * ops.EVAL_SLOTS, [0] * ops.EVAL_SLOTS, None
        else:
            (sums, counts), dev = self.acc.read(), self.acc.device
        sums, counts = gather_totals(sums, counts + [self.rows], dev)
        return sums, counts[:-1], counts[-1], time.time() - self.start


def _rows(x):
    """scores / targets as the eval kernels read them: detached fp32 with a contiguous last dimension (no copy when they already are)"""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    return x if (x.dim() < 1 or x.shape[-1] <= 1 or x.stride(-1) == 1) else x.contiguous()


def _labels(x):
    x = x.detach()
    if x.dtype != torch.int64:
        x = x.long()
    return x.contiguous()


def _ce_log(sums, counts, tot_time):
    val_loss, n_correct, n = sums[0], counts[0], counts[1]
    acc = n_correct / n
    LOGGER.info(f"validation finished in {int(tot_time)} seconds, acc: {acc*100:.2f}")
    return {'loss': val_loss / n, 'acc': acc, 'tok_per_s': n / tot_time}


# ------------------------------------------------------------------------------------------ the six passes
@torch.no_grad()
def validate_mlm(model, val_loader):
    LOGGER.info("start running MLM validation...")
    p = _Pass()
    for batch in val_loader:
        scores = _rows(model(batch, task='mlm', compute_loss=False))
        txt_labels = batch['txt_labels']
        idx = batch.get('txt_label_idx') if hasattr(batch, 'get') else None
        if idx is None:                     # (the reference's boolean indexing: a synchronisation, taken only without the index list)
            idx = (txt_labels != -1).reshape(-1).nonzero(as_tuple=False).squeeze(1)
        labels = txt_labels.reshape(-1).index_select(0, idx)          # as forward_mlm takes them
        ops.eval_ce(scores, _labels(labels), p.on(scores.device))
    sums, counts, _, tot_time = p.finish()
    return _ce_log(sums, counts, tot_time)


@torch.no_grad()
def validate_sap(model, val_loader):
    LOGGER.info("start running SAP validation...")
    p = _Pass()
    for batch in val_loader:
        scores = _rows(model(batch, task='sap', compute_loss=False))
        ops.eval_ce(scores, _labels(batch['ob_action_viewindex']), p.on(scores.device))
    sums, counts, _, tot_time = p.finish()
    return _ce_log(sums, counts, tot_time)


@torch.no_grad()
def validate_itm(model, val_loader):
    LOGGER.info("start running ITM validation...")
    p = _Pass()
    for batch in val_loader:
        scores, labels = model(batch, task='itm', compute_loss=False)
        scores = _rows(scores)
        ops.eval_ce(scores, _labels(labels), p.on(scores.device))
    sums, counts, _, tot_time = p.finish()
    return _ce_log(sums, counts, tot_time)


@torch.no_grad()
def validate_sar(model, val_loader):
    LOGGER.info("start running SAR validation...")
    p = _Pass()
    for batch in val_loader:
        scores = _rows(model(batch, task='sar', compute_loss=False))                       # [B, 3]: heading, elevation, progress
        targets = torch.cat([batch['ob_action_angles'][:, :2].float(), batch['ob_progress'].float().unsqueeze(1)], dim=1)
        ops.eval_mse_cols(scores[:, :3], targets, p.on(scores.device))
        p.rows += scores.size(0)
    sums, _, n_data, tot_time = p.finish()
    val_log = {'heading_loss': sums[0] / n_data, 'elevation_loss': sums[1] / n_data, 'progress_loss': sums[2] / n_data,
               'tok_per_s': n_data / tot_time}
    LOGGER.info(f"validation finished in {int(tot_time)} seconds, heading_loss: {val_log['heading_loss']:.4f}, "
                f"elevation_loss: {val_log['elevation_loss']:.4f}, progress_loss: {val_log['progress_loss']:.4f}")
    return val_log


@torch.no_grad()
def validate_sprel(model, val_loader):
    """The reference's statements are ``F.mse_loss(scores[:, j], batch['sp_targets'][:, j], reduction='sum')`` for j = 0 ('heading') and
    j = 1 ('elevation'), over ``n_data += scores.size(0)``.  On [R, 2] scores these are the two columns.  The model's own output is
    [B, 36, 2] (pretrain_cmt.py:216), where the same statements take VIEW j of every sample, both of its components: that is what they
    give here too -- the four numbers (view 0 / 1) x (component 0 / 1) are four columns of the [B, 72] rows, read in place."""
    LOGGER.info("start running SPREL validation...")
    p = _Pass()
    wide = False
    for batch in val_loader:
        scores = _rows(model(batch, task='sprel', compute_loss=False))
        targets = _rows(batch['sp_targets'])
        if scores.dim() == 3:
            wide = True
            B = scores.size(0)
            if scores.size(1) < 2 or scores.size(2) != 2 or targets.shape != scores.shape:
                raise ValueError(f"validate_sprel: scores {tuple(scores.shape)} / sp_targets {tuple(targets.shape)}: expected [B, >= 2, 2]")
            W = 2 * scores.size(1)
            ops.eval_mse_cols(scores.reshape(B, W)[:, :4], targets.reshape(B, W)[:, :4], p.on(scores.device))
        else:
            ops.eval_mse_cols(scores[:, :2], targets[:, :2], p.on(scores.device))
        p.rows += scores.size(0)
    sums, _, n_data, tot_time = p.finish()
    heading, elevation = (sums[0] + sums[1], sums[2] + sums[3]) if wide else (sums[0], sums[1])
    val_log = {'heading_loss': heading / n_data, 'elevation_loss': elevation / n_data, 'tok_per_s': n_data / tot_time}
    LOGGER.info(f"validation finished in {int(tot_time)} seconds, heading_loss: {val_log['heading_loss']:.4f}, "
                f"elevation_loss: {val_log['elevation_loss']:.4f}")
    return val_log


def compute_accuracy_for_soft_targets(out, labels):
    """number of rows whose arg-max agrees between `out` and `labels` (lowest index on ties), as a Python int: one read"""
    out, labels = _rows(out), _rows(labels)
    acc = ops.eval_kl(out.reshape(-1, out.shape[-1]), labels.reshape(-1, labels.shape[-1]), ops.EvalAccumulator(out.device))
    return int(acc.read()[1][0])


@torch.no_grad()
def validate_mrc(model, val_loader):
    """n_feat is the device's count of rows, which is ``hist_mrc_masks.sum()``: one row of scores per masked step"""
    LOGGER.info("start running MRC validation...")
    p = _Pass()
    for batch in val_loader:
        prediction_soft_label, img_target_probs = model(batch, task='mrc', compute_loss=False)
        prediction_soft_label = _rows(prediction_soft_label)
        ops.eval_kl(prediction_soft_label, _rows(img_target_probs), p.on(prediction_soft_label.device))
    sums, counts, _, tot_time = p.finish()
    val_loss, tot_score, n_feat = sums[0], counts[0], counts[1]
    val_acc = tot_score / n_feat
    LOGGER.info(f"validation finished in {int(tot_time)} seconds, score: {val_acc*100:.2f}")
    return {'loss': val_loss / n_feat, 'acc': val_acc, 'feat_per_s': n_feat / tot_time}


_VALIDATORS = (('mlm', validate_mlm), ('sap', validate_sap), ('sar', validate_sar), ('sprel', validate_sprel), ('mrc', validate_mrc),
               ('itm', validate_itm))


def validate(model, val_dataloaders, setname='', log_fn=None):
    """main_r2r.py:319-341.  Returns {f'val{setname}_{task}_{k}': v} over all tasks; `log_fn`, when given, is handed
    {f'valid{setname}_{task}/{k}': v} per task (where the reference calls TB_LOGGER.log_scalar_dict).  The model is put in eval mode
    for the pass and back in training mode after it, as the reference does."""
    model.eval()
    out = {}
    for task, loader in val_dataloaders.items():
        LOGGER.info(f"validate val{setname} on {task} task")
        fn = next((f for prefix, f in _VALIDATORS if task.startswith(prefix)), None)
        if fn is None:
            raise ValueError(f'Undefined task {task}')
        val_log = {f'val{setname}_{task}_{k}': v for k, v in fn(model, loader).items()}
        if log_fn is not None:
            log_fn({f'valid{setname}_{task}/{k}': v for k, v in val_log.items()})
        out.update(val_log)
    model.train()
    return out
