"""torch.optim's AdamW / Adam / RMSprop / SGD -- the four choices of the finetune agents' ``--optim`` (finetune_src/r2r/agent_cmt.py:62-77;
every finetune recipe runs ``adamW``) -- as one HIP launch over the flat fp32 arenas of optim.arena.

The arena machinery (re-homed parameters, bf16 shadow, gradient packing, the deferred global-norm clip, the pinned table ring, the
prepare_step / launch_step contract that graph.GraphedTrainStep captures) is optim.arena.ArenaOptimizer's; the update is
``hamt_optim_table`` with the rule as its first argument.  torch's rules are not the pretraining AdamW's (optim/adamw.py of the reference,
HF style) with other hyper-parameters: torch decays BEFORE the update and on every parameter, and adds eps AFTER dividing sqrt(v) by
sqrt(1 - beta2^t).

The host keeps two [nparams, 4] tables in one device block (one H2D copy per step), every entry formed in float64 and rounded once, as
torch does with its Python scalars:
  * hyp {lr, lr / (1 - beta1^t), weight_decay, active}: the arena's first table (the gradient-norm kernels and parallel.py read column 3);
  * aux {1 / sqrt(1 - beta2^t), 1 - lr * weight_decay, 0, 0}.
t is the parameter's own step count; it advances only where there is a gradient, as torch's does.  A rule's unused moment arenas are
not allocated (RMSprop: no exp_avg; SGD: neither).  ``state_dict()`` / ``load_state_dict()`` speak torch's layout, so a checkpoint moves
between these classes and torch.optim in both directions (``--resume_optimizer``).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from ..ops import _p, _stream
from .arena import ArenaOptimizer


def _refuse(name: str, **options):
    """options of torch's constructor whose non-default value the kernel does not implement"""
    for k, (v, default) in options.items():
        if v != default:
            raise ValueError(f"{name}: {k}={v!r} is not implemented by hamt_optim_table (only {k}={default!r})")


class _TorchRule(ArenaOptimizer):
    rule = None                     # hamt_opt_rule
    torch_class = None              # its defaults (and its checks of lr / betas / eps / weight_decay) are taken from the installed torch
    moment_keys = ()                # torch's state keys of the m / v arenas this rule owns
    n_tables = 2                    # hyp and _aux
    no_range_reason = "hamt_optim_table has no range form"      # (attach() refuses, parallel.py takes the all-reduce exchange)

    def _init(self, params, **given):
        params = list(params)
        defaults = dict(self.torch_class([torch.nn.Parameter(torch.zeros(1))], **given).defaults)    # raises torch's own ValueErrors
        super().__init__(params, defaults)

    # ---------------------------------------------------------------- arenas
    def _check_groups(self):
        for g in self.param_groups:
            if self._launch_scalars(g) != self._launch_scalars(self.param_groups[0]):
                raise ValueError(f"{type(self).__name__}: betas / alpha / eps must be the same in every group (one launch takes one set)")
            for k in ("amsgrad", "maximize", "centered", "nesterov"):
                if g.get(k, False):
                    raise ValueError(f"{type(self).__name__}: {k}=True is not implemented by hamt_optim_table")
            for k in ("momentum", "dampening"):
                if g.get(k, 0) != 0:
                    raise ValueError(f"{type(self).__name__}: {k}={g[k]!r} is not implemented by hamt_optim_table")

    def _launch_scalars(self, g):
        """(beta1, beta2, eps) of the launch"""
        b1, b2 = g["betas"]
        return float(b1), float(b2), float(g["eps"])

    def _build(self):
        super()._build()
        self._aux = self._tables[1]

    def _bytes_per_element(self, moments=None):
        """p and g read, p and the bf16 shadow written (14 per element), 8 more per moment arena the rule owns (`moments`: of another
        rule over the same arena): with the 4 of a zeroed gradient slot 34 / 34 / 26 / 18 for AdamW / Adam / RMSprop / SGD"""
        return 14.0 + 8.0 * (len(self.moment_keys) if moments is None else moments)

    # ---------------------------------------------------------------- host part of a step
    def _columns(self, t, lr, wd):
        """(hyp column 1, aux column 0, aux column 1) in float64 for step counts t >= 1.  The bias corrections use the betas AS THE
        KERNEL RECEIVES THEM (floats): its moments are then exactly Adam's with those betas, bias-corrected for those betas -- which
        differs from Adam with the double betas by ~1e-7 of the update.  With the double betas here, 1 - float(0.999) (1.29e-5 below
        0.001) in the kernel against 1 - 0.999^t in the table would leave the first updates 6.4e-6 of themselves off (in the fp32
        emulation of the tests' five-step schedule: 5.8e-7 of max|p| after the first step instead of 7.5e-8)."""
        b1, b2 = (float(np.float32(b)) for b in self._launch_scalars(self.param_groups[0])[:2])
        return lr / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t), 1.0 - lr * wd

    def _fill_table(self, h, t, lr, wd):
        h[0, :, 1], h[1, :, 0], h[1, :, 1] = self._columns(t, lr, wd)

    def _launch(self, gn, max_norm, zero_grad_arena):
        b1, b2, eps = self._launch_scalars(self.param_groups[0])
        L.check(L.load().hamt_optim_table(self.rule, self._n, _p(self._flat_p), _p(self._flat_g), _p(self._flat_m), _p(self._flat_v),
                                          _p(self._flat_p16), _p(self._ends), _p(self._hyp), _p(self._aux), len(self._params), gn,
                                          max_norm, b1, b2, eps, zero_grad_arena, _stream()), "hamt_optim_table")

    # ---------------------------------------------------------------- checkpointing (agent_cmt.py:607-644 saves optimizer.state_dict())
    def _state_of(self, i, p, o):
        """torch's layout: {'step' (0-dim float32 CPU tensor), the rule's moments under torch's names}"""
        st = super()._state_of(i, p, o)
        st["step"] = torch.tensor(float(self._steps[i]), dtype=torch.float32)
        return st

    def _groups_loaded(self):
        for name, default in self.defaults.items():          # (a checkpoint of another torch version may lack newer keys)
            for g in self.param_groups:
                g.setdefault(name, default)
        self.materialize()
        self._check_groups()

    def _restore(self, i, p, o, st):
        """'step' is a tensor or, as older torch wrote it, an int; a stepped parameter of SGD has none"""
        super()._restore(i, p, o, dict(st, step=round(float(st.get("step", 0)))))


class TorchAdamW(_TorchRule):
    """torch.optim.AdamW: p *= 1 - lr*wd, then Adam's update with eps outside the bias-corrected root."""
    rule, torch_class, moment_keys = L.OPT_ADAMW, torch.optim.AdamW, ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False):
        _refuse("TorchAdamW", amsgrad=(amsgrad, False), maximize=(maximize, False))
        self._init(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class TorchAdam(_TorchRule):
    """torch.optim.Adam: weight decay as an L2 term of the gradient."""
    rule, torch_class, moment_keys = L.OPT_ADAM, torch.optim.Adam, ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        _refuse("TorchAdam", amsgrad=(amsgrad, False), maximize=(maximize, False))
        self._init(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class TorchRMSprop(_TorchRule):
    """torch.optim.RMSprop with momentum 0, not centered (the parser's default --optim rms)."""
    rule, torch_class, moment_keys = L.OPT_RMSPROP, torch.optim.RMSprop, ("square_avg",)

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, maximize=False):
        _refuse("TorchRMSprop", momentum=(momentum, 0), centered=(centered, False), maximize=(maximize, False))
        self._init(params, lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay)

    def _launch_scalars(self, g):
        return 0.0, float(g["alpha"]), float(g["eps"])        # (alpha travels in hamt_optim_table's beta2)

    def _columns(self, t, lr, wd):
        return lr, np.ones_like(lr), 1.0 - lr * wd


class TorchSGD(_TorchRule):
    """torch.optim.SGD with momentum 0."""
    rule, torch_class, moment_keys = L.OPT_SGD, torch.optim.SGD, ()

    def __init__(self, params, lr, weight_decay=0, momentum=0, dampening=0, nesterov=False, maximize=False):
        _refuse("TorchSGD", momentum=(momentum, 0), dampening=(dampening, 0), nesterov=(nesterov, False), maximize=(maximize, False))
        self._init(params, lr=lr, weight_decay=weight_decay)

    def _launch_scalars(self, g):
        return 0.0, 0.0, 0.0

    def _columns(self, t, lr, wd):
        return lr, np.ones_like(lr), 1.0 - lr * wd

    def _state_of(self, i, p, o):
        return {"momentum_buffer": None}                      # what torch's SGD keeps for a stepped parameter without momentum
