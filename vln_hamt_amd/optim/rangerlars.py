"""RangerLars = Ralamb (RAdam with a LARS-style per-tensor trust ratio, pretrain_src/optim/ralamb.py) wrapped in Lookahead
(lookahead.py; rangerlars.py:12-14), as HIP kernels over the flat fp32 arenas of optim.AdamW.

The arena machinery (re-homed parameters, bf16 shadow, gradient packing, the deferred global-norm clip, the static launch
sequence that graph.GraphedTrainStep captures) is AdamW's; the update is three launches of ``hamt_ralamb_table``: moments and
per-item partial sums of squares, the per-parameter trust ratio, the update with the Lookahead sync.  The host keeps:
  * the AdamW table layout {lr, s*lr, weight_decay, active} (s: the RAdam step size, float64 like the reference's Python
    scalars) -- the gradient-norm kernels and parallel.py read its column 3;
  * a second table {N_sma >= 5, Lookahead action (0 none, 1 create, 2 interpolate), alpha, -weight_decay*lr};
  * a static item table (each item inside one parameter, at most 4096 elements, in arena order) with one partial slot per item;
  * one more fp32 arena for the slow weights (RangerLars only).

The reference's quirks are kept: the step count advances only for parameters with a gradient (ralamb.py:24, 51), weight decay is
applied before the norms (:70-71), weight_norm is clamped at 10 (:82), the Lookahead counter advances on EVERY step() (also one
without gradients, lookahead.py:48-52), a slow buffer is created lazily at the first sync where its parameter has a gradient (:29-35).
One divergence: ``state_dict()['slow_state']`` is keyed by parameter index like 'state' (the reference keys it by id(), which no
other process can map back).
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch
from torch.optim import Optimizer

from .. import _lib as L
from ..ops import _p, _stream
from .adamw import AdamW

ITEM4 = 1024        # float4 per item (256 threads x 4): the kernels' chunk
NONE, CREATE, INTERPOLATE = 0.0, 1.0, 2.0


def ralamb_coef(step: int, beta1: float, beta2: float):
    """(N_sma >= 5, RAdam step size) of step `step`: ralamb.py:57-68, statement for statement in float64."""
    beta2_t = beta2 ** step
    N_sma_max = 2 / (1 - beta2) - 1
    N_sma = N_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if N_sma >= 5:
        return True, math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (1 - beta1 ** step)
    return False, 1.0 / (1 - beta1 ** step)


def item_table(ends: np.ndarray, n: int) -> np.ndarray:
    """The static item table of hamt_ralamb_table (include/hamt.h) for parameters ending at `ends` (elements, exclusive)."""
    ends4 = np.asarray(ends, dtype=np.int64) // 4
    begins4 = np.concatenate([[0], ends4[:-1]])
    counts = -(-(ends4 - begins4) // ITEM4)
    first = np.concatenate([[0], np.cumsum(counts)])
    nitems = int(first[-1])
    param = np.repeat(np.arange(len(ends4)), counts)
    starts = begins4[param] + (np.arange(nitems) - first[param]) * ITEM4
    tab = np.concatenate([starts, [n // 4], param, first]).astype(np.int64)
    assert tab.max() < 2 ** 31
    return tab.astype(np.int32), nitems


class Ralamb(AdamW):
    """The reference's Ralamb (ralamb.py) on the arenas: RangerLars without the Lookahead wrapper."""

    _lookahead = False
    owned_slice_update = False      # every parameter's trust ratio needs its whole norm

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        Optimizer.__init__(self, params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._init_host_state()
        self._la_pending = None     # (actions, created) of the counted step: zero_grad() of a dropped pass takes them back

    # ---------------------------------------------------------------- arenas
    def _build(self):
        super()._build()
        n, dev, np_ = self._n, self._flat_p.device, len(self._params)
        ends = self._ends.cpu().numpy()
        tab, self._nitems = item_table(ends, n)
        self._items = torch.from_numpy(tab).to(dev)
        self._partials = torch.zeros(2 * self._nitems, dtype=torch.float32, device=dev)
        self._stats = torch.zeros(np_, 4, dtype=torch.float32, device=dev)     # {weight_norm, adam_norm, trust_ratio, 0}
        # both tables in one device block (one H2D copy per step); _hyp keeps AdamW's [nparams, 4] layout
        self._tables = torch.zeros(2, np_, 4, dtype=torch.float32, device=dev)
        self._hyp, self._rl = self._tables[0], self._tables[1]
        self._hyp_ring = [torch.zeros(2, np_, 4, dtype=torch.float32).pin_memory() for _ in range(4)]
        self._hyp_events = [None] * 4
        self._flat_slow = torch.zeros_like(self._flat_p) if self._lookahead else None
        self._has_slow = np.zeros(np_, dtype=bool)

    def attach(self, model, chunk_elems: int = 8 << 20):
        raise L.HamtError(f"{type(self).__name__}: the update cannot run chunk by chunk next to the next forward pass (attach / "
                          "overlap_update): every parameter's trust ratio needs its whole norm first")

    def update_bytes(self, active=None, sync=False) -> float:
        """algorithmic HBM bytes of one update: pass 1 reads p, g, m, v and writes m, v (24 per element, + 4 where the gradient slot
        is zeroed), pass 3 reads p, m, v and writes p and the bf16 shadow (18), + 8 (slow weights read and written) on a Lookahead
        sync (`sync`)"""
        self.materialize()
        sizes = np.diff(np.concatenate([[0], self._ends.cpu().numpy()])).astype(np.float64)
        per = sizes * (np.where(self._keep == 2.0, 42.0, 46.0) + (8.0 if sync and self._lookahead else 0.0))
        if active is not None:
            per = per * np.asarray(active, dtype=np.float64)
        return float(per.sum())

    # ---------------------------------------------------------------- host part of a step
    def _advance_lookahead(self, act: np.ndarray):
        """lookahead.py:48-52: every group's counter advances; at a multiple of k the parameters with a gradient sync"""
        actions = np.zeros(len(self._params), dtype=np.float32)
        if self._lookahead:
            for gi, g in enumerate(self.param_groups):
                g["lookahead_step"] += 1
                if g["lookahead_step"] % g["lookahead_k"] == 0:
                    sel = (self._gidx_np == gi) & act
                    actions[sel] = np.where(self._has_slow[sel], INTERPOLATE, CREATE)
        created = actions == CREATE
        self._has_slow |= created
        return actions, created

    def host_table(self, active: Optional[List[bool]] = None, advance: bool = True) -> np.ndarray:
        """AdamW.host_table's contract; the result is [2, nparams, 4]: the AdamW-layout table {lr, s*lr, weight_decay, active} and
        the RangerLars table {N_sma >= 5, Lookahead action, alpha, -weight_decay*lr}."""
        self.materialize()
        flags = self.table_flags(active)
        act = flags != 0
        if advance:
            self._steps[act] += 1
            self._counted = act.copy()
            self._la_pending = self._advance_lookahead(act)
        actions = self._la_pending[0] if self._la_pending is not None else np.zeros(len(self._params), dtype=np.float32)
        b1, b2 = self.param_groups[0]["betas"]
        coefs = {t: ralamb_coef(t, b1, b2) for t in set(np.maximum(self._steps, 1).tolist())}
        rect = np.array([coefs[max(int(t), 1)][0] for t in self._steps], dtype=np.float32)
        s = np.array([coefs[max(int(t), 1)][1] for t in self._steps], dtype=np.float64)
        lr = np.array([g["lr"] for g in self.param_groups], dtype=np.float64)[self._gidx_np]
        wd = np.array([g["weight_decay"] for g in self.param_groups], dtype=np.float64)[self._gidx_np]
        alpha = np.array([g.get("lookahead_alpha", 0.0) for g in self.param_groups], dtype=np.float64)[self._gidx_np]
        h = np.zeros((2, len(self._params), 4), dtype=np.float32)
        h[0, :, 0], h[0, :, 1], h[0, :, 2], h[0, :, 3] = lr, s * lr, wd, flags
        h[1, :, 0], h[1, :, 1], h[1, :, 2], h[1, :, 3] = rect, actions, alpha, -wd * lr
        self._table_active = flags
        return h

    def upload_table(self, table: Optional[np.ndarray]):
        """both device tables in one async copy from the pinned ring (None: nothing active, the launches touch nothing)"""
        self.materialize()
        k = self._hyp_slot
        self._hyp_slot = (k + 1) % len(self._hyp_ring)
        if self._hyp_events[k] is not None:
            self._hyp_events[k].synchronize()
        h = self._hyp_ring[k].numpy()
        if table is None:
            h[:] = 0.0
        else:
            h[:] = table
        self._tables.copy_(self._hyp_ring[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hyp_events[k] = ev

    def launch_step(self, zero_grad_arena: bool = True):
        """Device side of a step: hamt_ralamb_table's three launches (static; capturable)."""
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        gn, max_norm = self._pending_clip if self._pending_clip is not None else (None, 0.0)
        self._counted = None
        if zero_grad_arena:
            self._flat_g._hamt_dirty = False
        slow = self._flat_slow
        L.check(L.load().hamt_ralamb_table(_p(self._flat_p), _p(self._flat_g), _p(self._flat_m), _p(self._flat_v), _p(self._flat_p16),
                                           _p(slow) if slow is not None else None, _p(self._items), self._nitems, _p(self._hyp),
                                           _p(self._rl), len(self._params), _p(self._partials), _p(self._stats), _p(gn), float(max_norm),
                                           b1, b2, 1 - b1, 1 - b2, g0["eps"], int(zero_grad_arena), _stream()), "hamt_ralamb_table")

    def zero_grad(self, set_to_none: bool = True):
        counted = self._built and self._counted is not None
        super().zero_grad(set_to_none=set_to_none)
        if counted and self._la_pending is not None:
            # the dropped pass was counted: take its Lookahead step back as well (the reference counts inside step() only)
            actions, created = self._la_pending
            if self._lookahead:
                for g in self.param_groups:
                    g["lookahead_step"] -= 1
            self._has_slow[created] = False
            self._la_pending = None

    # ---------------------------------------------------------------- checkpointing
    def _torch_index(self):
        """parameter -> the index torch's Optimizer.state_dict gives it (position in the groups' parameter lists)"""
        out, i = {}, 0
        for g in self.param_groups:
            for p in g["params"]:
                out[id(p)] = i
                i += 1
        return out

    def state_dict(self):
        """Ralamb's per-parameter state {'step', 'exp_avg', 'exp_avg_sq', 'weight_norm', 'adam_norm', 'trust_ratio'} (ralamb.py:39-41,
        88-90) + param_groups; RangerLars adds 'slow_state' {index: {'slow_buffer'}} (lookahead.py:54-66, keyed by index)."""
        if not self._built:
            sd = Optimizer.state_dict(self)
        else:
            self.wait_update()
            stats = self._stats.clone()
            self.state.clear()
            for i, (p, o) in enumerate(zip(self._params, self._offs)):
                if self._steps[i] > 0:
                    n = p.numel()
                    self.state[p] = {"step": int(self._steps[i]), "exp_avg": self._flat_m[o:o + n].view(p.shape).clone(),
                                     "exp_avg_sq": self._flat_v[o:o + n].view(p.shape).clone(), "weight_norm": stats[i, 0].clone(),
                                     "adam_norm": stats[i, 1].clone(), "trust_ratio": stats[i, 2].clone()}
            try:
                sd = Optimizer.state_dict(self)
            finally:
                self.state.clear()
        if not self._lookahead:
            return sd
        slow = {}
        if self._built:
            tidx = self._torch_index()
            for i, (p, o) in enumerate(zip(self._params, self._offs)):
                if self._has_slow[i]:
                    slow[tidx[id(p)]] = {"slow_buffer": self._flat_slow[o:o + p.numel()].view(p.shape).clone()}
        return {"state": sd["state"], "slow_state": slow, "param_groups": sd["param_groups"]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Restore moments, step counts, norms and (RangerLars) the slow weights; a dict without 'slow_state' starts the slow weights
        fresh, as the reference does (lookahead.py:75-80)."""
        Optimizer.load_state_dict(self, {"state": state_dict["state"], "param_groups": state_dict["param_groups"]})
        if self._lookahead:
            for name, default in self.defaults.items():
                for g in self.param_groups:
                    g.setdefault(name, default)
        self.materialize()
        self.wait_update()
        self._flat_m.zero_()
        self._flat_v.zero_()
        self._stats.zero_()
        self._steps[:] = 0
        for i, (p, o) in enumerate(zip(self._params, self._offs)):
            st = self.state.get(p)
            if st:
                n = p.numel()
                self._flat_m[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self._flat_v[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                self._steps[i] = int(st["step"])
                for c, key in enumerate(("weight_norm", "adam_norm", "trust_ratio")):
                    if key in st:
                        self._stats[i, c] = torch.as_tensor(st[key], dtype=torch.float32)
        self.state.clear()
        self._has_slow[:] = False
        if self._lookahead:
            self._flat_slow.zero_()
            slow = state_dict.get("slow_state") or {}
            arena_of = {t: self._index_of[pid] for pid, t in self._torch_index().items()}
            for k, ent in slow.items():
                if k not in arena_of:
                    raise ValueError(f"{type(self).__name__}.load_state_dict: slow_state key {k!r} is no parameter index (a reference "
                                     "checkpoint keys it by id() of a tensor of another process: load it without 'slow_state')")
                if "slow_buffer" in ent:
                    i = arena_of[k]
                    o, p = self._offs[i], self._params[i]
                    self._flat_slow[o:o + p.numel()].copy_(ent["slow_buffer"].reshape(-1))
                    self._has_slow[i] = True
        self._counted = None
        self._la_pending = None
        self.refresh_shadow()


class RangerLars(Ralamb):
    """RangerLars(params, alpha=0.5, k=6, *args, **kwargs) of rangerlars.py:12-14: Ralamb(params, *args, **kwargs) under Lookahead(alpha, k).
    param_groups carry lookahead_alpha / lookahead_k / lookahead_step like the reference's."""

    _lookahead = True

    def __init__(self, params, alpha=0.5, k=6, *args, **kwargs):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f'Invalid slow update rate: {alpha}')
        if not 1 <= k:
            raise ValueError(f'Invalid lookahead steps: {k}')
        super().__init__(params, *args, **kwargs)
        defaults = dict(lookahead_alpha=alpha, lookahead_k=k, lookahead_step=0)
        self.defaults.update(defaults)                  # (lookahead.py:17-25)
        for name, default in defaults.items():
            for group in self.param_groups:
                group.setdefault(name, default)
