"""RangerLars = Ralamb (RAdam with a LARS-style per-tensor trust ratio, pretrain_src/optim/ralamb.py) wrapped in Lookahead
(lookahead.py; rangerlars.py:12-14), as HIP kernels over the flat fp32 arenas of optim.arena.

The arena machinery (re-homed parameters, bf16 shadow, gradient packing, the deferred global-norm clip, the static launch
sequence that graph.GraphedTrainStep captures) is optim.arena.ArenaOptimizer's; the update is three launches of
``hamt_ralamb_table``: moments and per-item partial sums of squares, the per-parameter trust ratio, the update with the Lookahead
sync.  The host keeps:
  * the arena's first table {lr, s*lr, weight_decay, active} (s: the RAdam step size, float64 like the reference's Python
    scalars) -- the gradient-norm kernels and parallel.py read its column 3;
  * a second table {N_sma >= 5, Lookahead action (0 none, 1 create, 2 interpolate), alpha, -weight_decay*lr};
  * a static item table (each item inside one parameter, at most 4096 elements, in arena order) with one partial slot per item
    (`set_item_cuts`: also inside one owner's share of a sharded update -- parallel.ShardedItemSync runs passes 1 and 3 over the
    items a rank owns, sums the partial slots over the ranks and runs pass 2 everywhere);
  * one more fp32 arena for the slow weights (RangerLars only).

The reference's quirks are kept: the step count advances only for parameters with a gradient (ralamb.py:24, 51), weight decay is
applied before the norms (:70-71), weight_norm is clamped at 10 (:82), the Lookahead counter advances on EVERY step() (also one
without gradients, lookahead.py:48-52), a slow buffer is created lazily at the first sync where its parameter has a gradient (:29-35).
One divergence: ``state_dict()['slow_state']`` is keyed by parameter index like 'state' (the reference keys it by id(), which no
other process can map back).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib as L
from ..ops import _p, _stream
from .arena import ArenaOptimizer, check_adam_args

ITEM4 = 1024        # float4 per item (256 threads x 4): the kernels' chunk
NONE, CREATE, INTERPOLATE = 0.0, 1.0, 2.0
STAT_KEYS = ("weight_norm", "adam_norm", "trust_ratio")     # state keys of the columns of _stats


def ralamb_coef(step: int, beta1: float, beta2: float):
    """(N_sma >= 5, RAdam step size) of step `step`: ralamb.py:57-68, statement for statement in float64."""
    beta2_t = beta2 ** step
    N_sma_max = 2 / (1 - beta2) - 1
    N_sma = N_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if N_sma >= 5:
        return True, math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (1 - beta1 ** step)
    return False, 1.0 / (1 - beta1 ** step)


def item_table(ends: np.ndarray, n: int, cuts=()) -> np.ndarray:
    """The static item table of hamt_ralamb_table (include/hamt.h) for parameters ending at `ends` (elements, exclusive).  `cuts`:
    element offsets (multiples of 8) that no item may straddle -- the boundaries between the owners of a sharded update
    (parallel.ShardedItemSync): an item that would straddle one ends there and the next begins there."""
    ends4 = np.asarray(ends, dtype=np.int64) // 4
    cuts = np.asarray(sorted(set(int(c) for c in cuts)), dtype=np.int64)
    if cuts.size and ((cuts % 8).any() or cuts[0] < 0 or cuts[-1] > n):
        raise ValueError(f"item_table: cuts must be multiples of 8 inside [0, {n}]")
    # segments: the stretches between neighbouring breaks (parameter ends and cuts); each lies inside one parameter and one cut interval
    breaks = np.unique(np.concatenate([[0], ends4, cuts // 4]))
    lo4, hi4 = breaks[:-1], breaks[1:]
    seg_param = np.searchsorted(ends4, lo4, side="right")             # the parameter q with begin(q) <= lo < end(q)
    counts = -(-(hi4 - lo4) // ITEM4)
    seg_first = np.concatenate([[0], np.cumsum(counts)])
    nitems = int(seg_first[-1])
    seg = np.repeat(np.arange(len(lo4)), counts)
    starts = lo4[seg] + (np.arange(nitems) - seg_first[seg]) * ITEM4
    param = seg_param[seg]
    first = np.concatenate([[0], np.cumsum(np.bincount(param, minlength=len(ends4)))])
    tab = np.concatenate([starts, [n // 4], param, first]).astype(np.int64)
    assert tab.max() < 2 ** 31
    return tab.astype(np.int32), nitems


def owned_item_runs(tab: np.ndarray, nitems: int, segments) -> list:
    """[(item_first, item_count)]: the maximal runs of consecutive items of the table `tab` that lie inside the element segments
    [(first, count)] (in arena order, as parallel.ShardedGradSync.owned() gives them).  Every segment boundary must be an item
    boundary (a cut the table was built with): an item that straddles one has no single owner."""
    starts = np.asarray(tab[:nitems + 1], dtype=np.int64)
    runs = []
    for f, c in segments:
        if f % 4 or c % 4:
            raise ValueError(f"owned_item_runs: segment ({f}, {c}) is not made of whole float4")
        i0, i1 = int(np.searchsorted(starts, f // 4)), int(np.searchsorted(starts, (f + c) // 4))
        if i1 > nitems or starts[i0] != f // 4 or starts[i1] != (f + c) // 4:
            raise ValueError(f"owned_item_runs: an item straddles a boundary of the segment ({f}, {c}): build the item table with that cut")
        if i1 == i0:
            continue
        if runs and runs[-1][0] + runs[-1][1] == i0:
            runs[-1] = (runs[-1][0], runs[-1][1] + i1 - i0)
        else:
            runs.append((i0, i1 - i0))
    return runs


class Ralamb(ArenaOptimizer):
    """The reference's Ralamb (ralamb.py) on the arenas: RangerLars without the Lookahead wrapper."""

    _lookahead = False
    n_tables = 2                    # the arena's {lr, s*lr, weight_decay, active} and _rl
    no_range_reason = "every parameter's trust ratio needs its whole norm first"
    item_slice_update = True        # the three passes run over item ranges (hamt_ralamb_*_items): parallel.ShardedItemSync asks for this

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        check_adam_args(lr, betas, eps)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._la_pending = None     # (actions, created) of the counted step: zero_grad() of a dropped pass takes them back

    # ---------------------------------------------------------------- arenas
    def _build(self):
        super()._build()
        n, dev, np_ = self._n, self._flat_p.device, len(self._params)
        self._item_cuts = ()
        self._build_items()
        self._stats = torch.zeros(np_, 4, dtype=torch.float32, device=dev)     # {weight_norm, adam_norm, trust_ratio, 0}
        self._rl = self._tables[1]
        self._flat_slow = torch.zeros_like(self._flat_p) if self._lookahead else None
        self._has_slow = np.zeros(np_, dtype=bool)

    def _build_items(self):
        tab, self._nitems = item_table(self._ends.cpu().numpy(), self._n, self._item_cuts)
        self._items_np = tab
        self._items = torch.from_numpy(tab).to(self._flat_p.device)
        self._partials = torch.zeros(2 * self._nitems, dtype=torch.float32, device=self._flat_p.device)

    def set_item_cuts(self, cuts):
        """Rebuild the item table (and its partial slots) so that no item straddles one of `cuts` (element offsets, multiples of 8):
        what a sharded update needs at the boundaries between its owners.  Before the first step only: afterwards the table is
        part of what the run computes (a parameter's norms are summed item by item), and changing it mid-run would change them."""
        self.materialize()
        cuts = tuple(sorted(set(int(c) for c in cuts)))
        if cuts == self._item_cuts:
            return
        if self._steps.any() or self._counted is not None:
            raise L.HamtError(f"{type(self).__name__}.set_item_cuts: the optimiser has stepped (or loaded a stepped state) with another item table; "
                              "choose the exchange (parallel.make_grad_sync) before the first step and before load_state_dict")
        self._item_cuts = cuts
        self._build_items()

    def item_runs(self, segments):
        """the maximal runs of consecutive items inside the element segments [(first, count)]: `owned_item_runs` on this table"""
        return owned_item_runs(self._items_np, self._nitems, segments)

    def _bytes_per_element(self, sync=False):
        """pass 1 reads p, g, m, v and writes m, v (24 per element), pass 3 reads p, m, v and writes p and the bf16 shadow (18),
        + 8 (slow weights read and written) on a Lookahead sync (`sync`)"""
        return 42.0 + (8.0 if sync and self._lookahead else 0.0)

    # ---------------------------------------------------------------- host part of a step
    def _advanced(self, act: np.ndarray):
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
        self._la_pending = actions, created

    def _fill_table(self, h, t, lr, wd):
        """column 1 of the first table: s*lr; the RangerLars table {N_sma >= 5, Lookahead action, alpha, -weight_decay*lr}"""
        actions = self._la_pending[0] if self._la_pending is not None else np.zeros(len(self._params), dtype=np.float32)
        b1, b2 = self.param_groups[0]["betas"]
        coefs = {k: ralamb_coef(k, b1, b2) for k in set(t.astype(np.int64).tolist())}
        rect = np.array([coefs[int(k)][0] for k in t], dtype=np.float32)
        s = np.array([coefs[int(k)][1] for k in t], dtype=np.float64)
        alpha = np.array([g.get("lookahead_alpha", 0.0) for g in self.param_groups], dtype=np.float64)[self._gidx_np]
        h[0, :, 1] = s * lr
        h[1, :, 0], h[1, :, 1], h[1, :, 2], h[1, :, 3] = rect, actions, alpha, -wd * lr

    def _launch(self, gn, max_norm, zero_grad_arena):
        """hamt_ralamb_table's three launches"""
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        slow = self._flat_slow
        L.check(L.load().hamt_ralamb_table(_p(self._flat_p), _p(self._flat_g), _p(self._flat_m), _p(self._flat_v), _p(self._flat_p16),
                                           _p(slow) if slow is not None else None, _p(self._items), self._nitems, _p(self._hyp),
                                           _p(self._rl), len(self._params), _p(self._partials), _p(self._stats), gn, max_norm,
                                           b1, b2, 1 - b1, 1 - b2, g0["eps"], zero_grad_arena, _stream()), "hamt_ralamb_table")

    # the three passes on their own, passes 1 and 3 over item runs [(item_first, item_count)]: the owned-item update of
    # parallel.ShardedItemSync (static launches, capturable)
    def launch_moments_items(self, runs, gn, max_norm, zero_grad_arena=True):
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        lib = L.load()
        for f, c in runs:
            L.check(lib.hamt_ralamb_moments_items(_p(self._flat_p), _p(self._flat_g), _p(self._flat_m), _p(self._flat_v), _p(self._items),
                                                  self._nitems, f, c, _p(self._hyp), _p(self._rl), len(self._params), _p(self._partials),
                                                  _p(gn), float(max_norm), b1, b2, 1 - b1, 1 - b2, g0["eps"], int(zero_grad_arena),
                                                  _stream()), "hamt_ralamb_moments_items")

    def launch_trust(self):
        L.check(L.load().hamt_ralamb_trust(_p(self._items), self._nitems, _p(self._hyp), len(self._params), _p(self._partials),
                                           _p(self._stats), _stream()), "hamt_ralamb_trust")

    def launch_apply_items(self, runs):
        slow, lib = self._flat_slow, L.load()
        for f, c in runs:
            L.check(lib.hamt_ralamb_apply_items(_p(self._flat_p), _p(self._flat_m), _p(self._flat_v), _p(self._flat_p16),
                                                _p(slow) if slow is not None else None, _p(self._items), self._nitems, f, c, _p(self._hyp),
                                                _p(self._rl), len(self._params), _p(self._stats), self.param_groups[0]["eps"], _stream()),
                    "hamt_ralamb_apply_items")

    def _taken_back(self):
        if self._la_pending is not None:
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
        sd = super().state_dict()
        if not self._lookahead:
            return sd
        slow = {}
        if self._built:
            tidx = self._torch_index()
            for i, (p, o) in enumerate(zip(self._params, self._offs)):
                if self._has_slow[i]:
                    slow[tidx[id(p)]] = {"slow_buffer": self._flat_slow[o:o + p.numel()].view(p.shape).clone()}
        return {"state": sd["state"], "slow_state": slow, "param_groups": sd["param_groups"]}

    def _state_of(self, i, p, o):
        st = super()._state_of(i, p, o)
        for c, key in enumerate(STAT_KEYS):
            st[key] = self._stats[i, c].clone()
        return st

    def _groups_loaded(self):
        if self._lookahead:
            for name, default in self.defaults.items():
                for g in self.param_groups:
                    g.setdefault(name, default)

    def _reset_state(self):
        super()._reset_state()
        self._stats.zero_()
        self._has_slow[:] = False
        self._la_pending = None
        if self._lookahead:
            self._flat_slow.zero_()

    def _restore(self, i, p, o, st):
        super()._restore(i, p, o, st)
        for c, key in enumerate(STAT_KEYS):
            if key in st:
                self._stats[i, c] = torch.as_tensor(st[key], dtype=torch.float32)

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Restore moments, step counts, norms and (RangerLars) the slow weights; a dict without 'slow_state' starts the slow weights
        fresh, as the reference does (lookahead.py:75-80)."""
        super().load_state_dict({"state": state_dict["state"], "param_groups": state_dict["param_groups"]})
        if self._lookahead:
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
