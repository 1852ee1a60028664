"""HF-style AdamW (pretrain_src/optim/adamw.py:13-112) as HIP kernels over the flat fp32 arenas of optim.arena.

The update is one launch of ``hamt_adamw_table``: per-parameter {lr, bias-corrected step size, weight decay, active} come from the
device table the host refreshes each step.  Parameters whose ``grad is None`` are skipped like the reference's ``continue``
(:70-71) and keep their own step count for the bias correction (:93-97).  It is the one rule whose kernel has a range form
(``hamt_adamw_table_range``), so it alone can run chunk by chunk next to the following forward pass (`attach`) and on the owned
slices of parallel.ShardedGradSync.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from .. import streams
from ..ops import _p, _stream
from .arena import ArenaOptimizer, _Overlap, check_adam_args, clip_grad_norm_, shadow_only  # noqa: F401  (the last two: imported from here)


class AdamW(ArenaOptimizer):
    owned_slice_update = True       # the update has a range form (hamt_adamw_table_range): attach() and parallel.ShardedGradSync use it

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True):
        check_adam_args(lr, betas, eps)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))

    def _bytes_per_element(self):
        """read p, g, m, v + write p, m, v + bf16 shadow"""
        return 30.0

    def _fill_table(self, h, t, lr, wd):
        """column 1: the bias-corrected step size (optim/adamw.py:93-97)"""
        b1, b2 = self.param_groups[0]["betas"]
        cb = np.array([bool(g["correct_bias"]) for g in self.param_groups])[self._gidx_np]
        h[0, :, 1] = np.where(cb, lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), lr)

    def _launch(self, gn, max_norm, zero_grad_arena):
        b1, b2 = self.param_groups[0]["betas"]
        L.check(L.load().hamt_adamw_table(self._n, _p(self._flat_p), _p(self._flat_g), _p(self._flat_m), _p(self._flat_v),
                                          _p(self._flat_p16), _p(self._ends), _p(self._hyp), len(self._params), gn,
                                          max_norm, b1, b2, self.param_groups[0]["eps"], zero_grad_arena, _stream()),
                "hamt_adamw_table")

    # ---------------------------------------------------------------- update next to the following forward pass
    def attach(self, model: torch.nn.Module, chunk_elems: int = 8 << 20):
        """Let `step()` (and graph.GraphedTrainStep) run the update on a stream of its own, chunk by chunk in the order the
        forward pass reads the parameters, while the NEXT forward pass of `model` already runs: the update streams 34 bytes
        per parameter through HBM and no matrix core, the forward pass is the opposite.  Forward pre-hooks on the modules of
        `model` make the stream a module runs on wait for the chunk(s) holding the parameters of that module's subtree --
        except for classes that declare `_hamt_container = True` (their forward reads parameters only through child modules'
        __call__, or behind an explicit streams.gate(...)): without such declarations the root waits for everything and
        nothing overlaps, which is slow but never wrong.  A forward hook on `model` itself waits for the whole update, so everything behind a forward pass (backward, gradient norm,
        the next update) is ordered as before.  Anything else that reads parameters or the arenas directly must call
        `wait_update()` first (state_dict / load_state_dict / refresh_shadow / gradient packing in optim.arena do)."""
        self.materialize()
        self._ov = _Overlap(self, model, chunk_elems)
        # (graph.GraphedTrainStep replays the update of step t at the head of step t+1: the device table then describes the
        # PREVIOUS step while this step's norm is reduced -> zero every slot and reduce the whole arena, as before)
        self._keep[:] = 1.0
        self._publish_grad_slots()
        return self

    def detach(self):
        if self._ov is not None:
            self.wait_update()
            self._ov.remove()
            self._ov = None

    def launch_step_overlapped(self, gnorm_sq=None, max_norm: float = 0.0):
        """launch_step on the update stream, one launch + one event per chunk (capturable: a fork of the capturing stream that
        the forward hooks join again)."""
        ov = self._ov
        b1, b2 = self.param_groups[0]["betas"]
        if gnorm_sq is None and self._pending_clip is not None:
            gnorm_sq, max_norm = self._pending_clip
        self._flat_g._hamt_dirty = False
        self._counted = None
        lib = L.load()
        ov.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(ov.stream):
            for i, (f, c) in enumerate(ov.chunks):
                L.check(lib.hamt_adamw_table_range(f, c, _p(self._flat_p[f:f + c]), _p(self._flat_g[f:f + c]), _p(self._flat_m[f:f + c]),
                                                   _p(self._flat_v[f:f + c]), _p(self._flat_p16[f:f + c]), _p(self._ends), _p(self._hyp),
                                                   len(self._params), _p(gnorm_sq), float(max_norm), b1, b2, self.param_groups[0]["eps"], 1,
                                                   _stream()), "hamt_adamw_table_range")
                ov.events[i].record(ov.stream)
        ov.pending = True
        ov.waited.clear()
        streams.pending_updates.add(self)
