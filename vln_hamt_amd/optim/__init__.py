"""Mirror of ``pretrain_src/optim``: HF-style AdamW, RangerLars (Ralamb + Lookahead), warmup/linear schedule, name-based decay groups --
and torch.optim's AdamW / Adam / RMSprop / SGD, the finetune agents' choices (torch_rules) --
with the update, the global-norm clip and the bf16-shadow refresh running as HIP kernels over flat arenas (arena.ArenaOptimizer)."""
from .sched import warmup_linear, get_lr_sched
from .arena import ArenaOptimizer, clip_grad_norm_
from .adamw import AdamW
from .rangerlars import Ralamb, RangerLars
from .torch_rules import TorchAdam, TorchAdamW, TorchRMSprop, TorchSGD
from .misc import build_optimizer
