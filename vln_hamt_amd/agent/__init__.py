"""The part of a finetune rollout every agent of the reference shares (R2R, R2R-back, CVDN, REVERIE's action side): the per-step action
choice and losses on the device.  The agents themselves (simulator, teacher lookup, reward shaping, metrics) are out of scope."""
from .recorder import RolloutRecorder

__all__ = ["RolloutRecorder"]
