"""`ReverieRolloutRecorder`: `RolloutRecorder` for REVERIE's agent (finetune_src/reverie/agent.py:250-307, :448-451).

What REVERIE's loop does differently from the other three agents, per step: the best object (`torch.max(obj_logits, 1)`) is appended to
the action logits as column V = ob_img_max_len, which is STOP (`next_id >= ob_img_max_len`, no `cand_len - 1` rule); the imitation
cross-entropy is taken after the back-track mask; a second cross-entropy grounds the goal object (`ref_loss`); and a step that stops,
or the last one, records the predicted object.  Here that is `ops.policy_ref_step`, one launch per step (one more in the backward),
and the step's one transfer to the host is still the int32 environment action; the predicted objects cross once, after the rollout.
"""
from __future__ import annotations

import torch

from .. import ops
from .recorder import RolloutRecorder, _alias


class ReverieRolloutRecorder(RolloutRecorder):
    """`RolloutRecorder` plus the [T_max, B] fp32 array `ref` (the object cross-entropy per step and episode) and the int32 [B] vectors
    `pred_obj` (the predicted object's slot) / `pred_obj_id` (its id, when the steps get `obj_ids`), -1 = none, reset to -1.

        rec.reset(B)
        for t in range(T):
            outs = model('visual', ..., return_states=True)
            a_t, env_action, prev_angle = rec.step(t, outs['act_logits'], outs['obj_logits'], obj_lens, target, cand_lens, bt_mask,
                                                   ob_ang_feats, feedback, ref_target=ref_target)
            ...
        loss, logs = rec.loss(critic, hidden_states, last_h, train_ml=0.2)       # + ref.sum() / B, logs['REF_loss']
        slots, ids = rec.predicted_objects()
    """

    def _alloc(self, B):
        super()._alloc(B)
        self.ref = torch.zeros(self.T_max, B, dtype=torch.float32, device=self.device)
        self._pred = torch.full((2, B), -1, dtype=torch.int32, device=self.device)       # one array: one copy at the end of the rollout
        self.pred_obj, self.pred_obj_id = _alias(self._pred, 0, (B,)), _alias(self._pred, B, (B,))
        self._rows["ref"] = []

    def reset(self, batch_size=None, fresh_draws=True):
        super().reset(batch_size, fresh_draws)
        self._rows["ref"] = []
        self._pred.fill_(-1)
        return self

    def step(self, t, act_logit, obj_logit, obj_lens, target=None, cand_lens=None, bt_mask=None, ob_ang_feats=None, feedback="sample",
             forced_action=None, uniform=None, sync=True, nav=None, cand_nodes=None, teacher_mode="path_step", stop_logit="index",
             ref_target=None, obj_ids=None, goal_obj=None):
        """Step t on `act_logit` [B, V] and `obj_logit` [B, O]; `obj_lens` int32 [B] is each viewpoint's TRUE object count (0 allowed; a
        host list is uploaded, like `cand_lens` = navigable candidates + 1).  Returns what RolloutRecorder.step returns.  `stop_logit`:
        'index' (the reference's column V) or 'value' (ops.policy_ref_step).  The object target is `ref_target` int64 [B], or comes from
        `obj_ids` int32 [B, O] and `goal_obj` int32 [B]; `obj_ids` also fills `pred_obj_id`.  `nav` (a GoalSetEpisodes) with
        `cand_nodes`: `ops.nav_observe` -> `ops.policy_ref_step` -> `ops.nav_advance_goals`, as the base class does.  The step is the
        rollout's last one, which predicts an object for every episode still running, when t == T_max - 1."""
        if nav is not None and getattr(nav, "KIND", "r2r") != "goals":
            raise ops.L.HamtError("ReverieRolloutRecorder.step: nav= must be a GoalSetEpisodes")
        cand_lens, target, bt_mask = self._begin_step(t, cand_lens, target, bt_mask, nav, cand_nodes, teacher_mode)
        ml, ref, logp, ent, a_t, env_action, prev_angle = ops.policy_ref_step(
            act_logit, obj_logit, self._upload_i32(obj_lens), cand_lens, self.ended, self._row(self.mask, t), mode=feedback,
            stop_logit=stop_logit, target=target, ref_target=ref_target, obj_id=obj_ids, goal_obj=goal_obj, bt_mask=bt_mask,
            ob_ang=ob_ang_feats, hist_len=self.hist_len, forced_action=forced_action, uniform=uniform, last_step=(t == self.T_max - 1),
            ignoreid=self.ignoreid, call_id=(self.call_id + t) & 0xFFFFFFFF, pred_obj=self.pred_obj,
            pred_obj_id=self.pred_obj_id if obj_ids is not None else None,
            out=tuple(self._row(b_, t) for b_ in (self.ml, self.ref, self.logp, self.ent)))
        return self._end_step(t, feedback, {"ml": ml, "ref": ref, "logp": logp, "ent": ent}, a_t, env_action, prev_angle, nav, cand_nodes,
                              sync, None)

    def predicted_objects(self):
        """(slot, id) int32 numpy [B] of every episode's predicted object, -1 = none (`predObjId` None, agent.py:193, :301): ONE
        device-to-host copy, at the end of the rollout."""
        host = self._pred.cpu().numpy()
        return host[0], host[1]

    def loss(self, critic=None, hidden_states=None, last_h=None, train_ml=None, gamma=0.9, entropy_weight=0.01, normalize="total",
             train_rl=True):
        """RolloutRecorder.loss plus, when `train_ml` is given, ref.sum() / B -- NOT scaled by train_ml (agent.py:449) -- logged as
        REF_loss (:451)."""
        loss, logs = super().loss(critic, hidden_states, last_h, train_ml=train_ml, gamma=gamma, entropy_weight=entropy_weight,
                                  normalize=normalize, train_rl=train_rl)
        if train_ml is not None:
            rl = self.stacked("ref").sum() * (1.0 / self.B)
            loss = loss + rl
            logs["REF_loss"] = rl.detach()
        return loss, logs
