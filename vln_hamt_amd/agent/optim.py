"""The finetune agents' optimiser pair (finetune_src/r2r/agent_cmt.py:62-77, 561-567, 597-602, 607-644) on the flat arenas: one
torch-rule optimiser for `vln_bert` and one for `critic`, the global-norm clip at 40 over `vln_bert`'s gradients only, and the
reference's checkpoint layout.  Per iteration: the sum of squares over vln_bert's arena, one `hamt_optim_table` launch and one table
upload per optimiser -- no per-tensor launch, and the bf16 weight shadows come out of the update."""
from __future__ import annotations

from ..optim.adamw import clip_grad_norm_
from ..optim.torch_rules import TorchAdam, TorchAdamW, TorchRMSprop, TorchSGD

OPTIMIZERS = {"rms": TorchRMSprop, "adam": TorchAdam, "adamW": TorchAdamW, "sgd": TorchSGD}      # agent_cmt.py:62-69
_DDP_PREFIX = "module."
MAX_GRAD_NORM = 40.0                                                                             # agent_cmt.py:564, 599


def optimizer_class(name: str):
    """args.optim -> class, as agent_cmt.py:62-71 maps it (anything else: its `assert False`)"""
    if name not in OPTIMIZERS:
        raise AssertionError(f"--optim {name!r}: the agents know 'rms', 'adam', 'adamW' and 'sgd' (agent_cmt.py:62-71)")
    return OPTIMIZERS[name]


class AgentOptimizers:
    def __init__(self, vln_bert, critic, vln_bert_optimizer, critic_optimizer):
        self.vln_bert, self.critic = vln_bert, critic
        self.vln_bert_optimizer, self.critic_optimizer = vln_bert_optimizer, critic_optimizer
        self.optimizers = (vln_bert_optimizer, critic_optimizer)

    def _pairs(self):
        return [("vln_bert", self.vln_bert, self.vln_bert_optimizer), ("critic", self.critic, self.critic_optimizer)]

    def zero_grad(self):
        for o in self.optimizers:
            o.zero_grad()

    def optim_step(self, loss=None):
        """agent_cmt.py:561-567: backward, clip_grad_norm_(vln_bert.parameters(), 40.), both steps.  The clip is deferred into
        vln_bert's update; the critic's gradients are not part of the norm and are not scaled.  Returns vln_bert's gradient norm
        (device scalar, no host synchronisation)."""
        if loss is not None:
            loss.backward()
        norm = clip_grad_norm_(self.vln_bert.parameters(), MAX_GRAD_NORM, optimizer=self.vln_bert_optimizer.materialize())
        self.critic_optimizer._pending_clip = None           # (max_norm = 0 in its launch)
        self.vln_bert_optimizer.step()
        self.critic_optimizer.step()
        return norm

    # ---------------------------------------------------------------- agent_cmt.py:607-644
    def state(self, name, epoch, model=None):
        """one entry of the reference's checkpoint: {'epoch', 'state_dict', 'optimizer'} of 'vln_bert' or 'critic'"""
        models = {n: (m, o) for n, m, o in self._pairs()}
        held, opt = models[name]
        return {"epoch": epoch + 1, "state_dict": (held if model is None else model).state_dict(), "optimizer": opt.state_dict()}

    def states(self, epoch):
        """what the reference's save() writes: torch.save(optimizers.states(epoch), path)"""
        return {name: self.state(name, epoch) for name, _, _ in self._pairs()}

    def load(self, states, resume_optimizer=False):
        """A checkpoint in that layout (already read) into the two models and, with `resume_optimizer`, the two optimisers; returns the
        epoch to resume at.  Entries the checkpoint lacks keep the model's values.  A checkpoint saved from DDP-wrapped models names
        every tensor 'module.<name>': when this model is not wrapped, that prefix is taken off (agent_cmt.py:624-645 is the behaviour
        this reproduces)."""
        for name, model, opt in self._pairs():
            saved = states[name]["state_dict"]
            own = model.state_dict()
            wrapped_here = all(k.startswith(_DDP_PREFIX) for k in own)
            if saved and not wrapped_here and all(k.startswith(_DDP_PREFIX) for k in saved):
                saved = {k[len(_DDP_PREFIX):]: v for k, v in saved.items()}
            model.load_state_dict({**own, **saved})
            if resume_optimizer:
                opt.load_state_dict(states[name]["optimizer"])      # (re-derives the bf16 shadow as well)
            elif opt._built:
                opt.refresh_shadow()                                # the masters changed in place: one cast launch over the arena
        return states["vln_bert"]["epoch"] - 1


def build_agent_optimizers(args, vln_bert, critic) -> AgentOptimizers:
    """agent_cmt.py:62-77: optimizer(model.parameters(), lr=args.lr) for each of the two models, everything else the class default."""
    cls = optimizer_class(args.optim)
    return AgentOptimizers(vln_bert, critic, cls(vln_bert.parameters(), lr=args.lr), cls(critic.parameters(), lr=args.lr))
