"""`RolloutRecorder`: what the finetune agents do between two model calls of a rollout, and at its end, on the device.

The reference's agent loop (finetune_src/r2r/agent_cmt.py:336-401; the R2R-back, CVDN and REVERIE agents repeat it) runs, per step, an
imitation cross-entropy, the back-track mask, softmax / Categorical / entropy / sample / log_prob (or max / log_softmax / gather), a
blocking `.cpu()`, two Python loops over the batch and an upload, and keeps per-step lists that `torch.stack` joins for the A2C loss
(:476-522).  Here one step is `ops.policy_step` (one launch, one more for its backward) writing straight into row t of the [T_max, B]
arrays `ops.a2c_loss` reads, and the only thing that crosses to the host is the int32 environment action the simulator needs.

With `nav=` (agent.NavEpisodes: the episodes' place in the navigation graph, on the device) the step is `ops.nav_observe` -> `ops.policy_step`
-> `ops.nav_advance` (`ops.nav_advance_goals` for CVDN's / REVERIE's goal sets, `ops.nav_advance_back` for R2R-Back's return trips): the
teacher action lookup (`_teacher_action`, :199-211), the back-track mask (:342-349) and the reward shaping
(:407-445) run on the device too, and the reward lands in row t of `reward`.

What stays on the host: the simulator (and, without `nav=`, the teacher action lookup and the reward shaping, handed in by the caller;
the observations the model reads come from the host too unless an `agent.ObsEpisodes` gathers them on the device).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops


def _alias(buf: torch.Tensor, offset: int, shape) -> torch.Tensor:
    """a contiguous tensor over `buf`'s storage at element `offset` that autograd does not treat as a view of `buf`"""
    return torch.empty(0, dtype=buf.dtype, device=buf.device).set_(buf.untyped_storage(), buf.storage_offset() + offset, tuple(shape))


class _JoinRows(torch.autograd.Function):
    """The per-step rows a rollout wrote into one [T_max, B] array, as ONE [T, B] autograd tensor: no copy (the rows already lie
    there); the backward hands row t of the gradient to step t."""

    @staticmethod
    def forward(ctx, buf, T, *rows):
        assert len(rows) == T
        return _alias(buf, 0, (T, buf.shape[1]))

    @staticmethod
    def backward(ctx, g):
        return (None, None) + tuple(g[t] for t in range(g.shape[0]))


class RolloutRecorder:
    """Owns the [T_max, B] fp32 arrays `ml`, `logp`, `ent`, `mask`, `reward`, the device vectors `ended` (uint8) and `hist_len` (int32)
    and one pinned int32 [B] host buffer for the environment action.

        rec.reset(B)
        for t in range(T):
            logit, h_t = model('visual', ..., hist_lens=rec.hist_len, return_states=True)
            a_t, env_action, prev_angle = rec.step(t, logit, target, cand_lens, bt_mask, ob_ang_feats, feedback)
            hist.append(model('history', ..., hist_ang_feats=prev_angle, ob_step=t))
            ... simulator.make_equiv_action(env_action) ...
        rec.set_rewards(rewards)
        loss, logs = rec.loss(critic, hidden_states, last_h, train_ml=0.2)

    With the navigation graph on the device (`nav = NavEpisodes(graphs, T, B).reset(scans, starts, gt_paths)`), target, bt_mask and the
    rewards need no host: `rec.step(t, logit, cand_lens=..., nav=nav, cand_nodes=cand_nodes, teacher_mode='path_step')`, no `set_rewards`.

    Draws of 'sample': step t hashes (ops.rng_state's seed and epoch, a call id, the row).  `reset()` takes a FRESH block of T_max call
    ids from ops.next_call_id, as every dropout call does, so rollouts drawn eagerly differ from each other whether or not anything
    advances the epoch.  A captured step has its call id baked into the graph: it draws afresh on a replay only when the epoch has
    moved (ops.advance_rng_epoch between replays), and its recorder is reset with `reset(fresh_draws=False)` so that eager steps
    of the same recorder keep the id the graph holds.
    """

    def __init__(self, max_steps: int, batch_size: int, device="cuda", ignoreid: int = -100):
        self.T_max, self.ignoreid = int(max_steps), int(ignoreid)
        self.device = torch.device(device)
        self._take_call_ids()
        self._alloc(int(batch_size))

    def _take_call_ids(self):
        """step t draws with call id (call_id + t): a block of T_max ids nobody else gets"""
        self.call_id = ops.next_call_id()
        for _ in range(self.T_max - 1):
            ops.next_call_id()

    def _alloc(self, B):
        dev, T = self.device, self.T_max
        self.B = B
        self.ml, self.logp, self.ent, self.mask, self.reward = (torch.zeros(T, B, dtype=torch.float32, device=dev) for _ in range(5))
        self.ended = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.hist_len = torch.ones(B, dtype=torch.int32, device=dev)
        self.env_host = torch.empty(B, dtype=torch.int32).pin_memory()
        self.env_host_np = self.env_host.numpy()
        self._event = torch.cuda.Event()
        self._rows = {"ml": [], "logp": [], "ent": []}
        self.feedback = self.target = self.bt_mask = None

    def reset(self, batch_size=None, fresh_draws=True):
        """New rollout: nothing ended, history length 1 (the global [CLS] embedding, agent_cmt.py:305-306), no steps recorded, and
        (`fresh_draws`) a new block of call ids: this rollout's 'sample' draws differ from the last one's under the same RNG epoch.
        `fresh_draws=False` keeps the ids (a recorder whose step is captured in a graph: see the class docstring)."""
        if fresh_draws:
            self._take_call_ids()
        B = self.B if batch_size is None else int(batch_size)
        if B != self.B:
            self._alloc(B)
        else:
            self.ended.zero_()
            self.hist_len.fill_(1)
            self._rows = {"ml": [], "logp": [], "ent": []}
            self.feedback = None
        return self

    @property
    def steps(self) -> int:
        return len(self._rows["ml"])

    def step(self, t, logit, target=None, cand_lens=None, bt_mask=None, ob_ang_feats=None, feedback="sample", forced_action=None,
             uniform=None, sync=True, nav=None, cand_nodes=None, teacher_mode="path_step", end_on_miss=None):
        """Step t of the rollout on `logit` [B, V].  Returns (a_t, env_action, prev_act_angle): a_t int64 [B] on the device, the
        environment's action (int32, -1 = stop / ignored / ended) as a numpy view of the pinned host buffer -- the step's ONE
        device-to-host copy, followed by one event wait -- and the chosen candidate's angle feature [B, A] for `history`.
        sync=False returns the device tensor instead and copies nothing (the form used inside a captured graph).
        `cand_lens` is an int32 device tensor [B] (a host list is uploaded).
        `nav` (a NavEpisodes) with `cand_nodes` int32 [B, V] (each navigable candidate's node, -1 = padding): `target` and `bt_mask` left
        at None come from `ops.nav_observe` (`teacher_mode`: 'path_step', 'path_index' or 'shortest', env.py::_teacher_path_action;
        False = none, as a run without imitation loss / without the back-track mask), and `ops.nav_advance` moves the episodes and
        writes the step's reward into row t of `reward`.  The episodes' kind picks that launch: a GoalSetEpisodes (CVDN, REVERIE) takes
        `ops.nav_advance_goals`; a ReturnEpisodes (R2R-Back) takes `ops.nav_advance_back`, which also reads and writes `ended` (the first
        STOP does not end a return trip) -- `end_on_miss` (a missed mid-stop ends the episode, agent_r2rback.py:252, which sits under
        `if train_rl:`) defaults to feedback == 'sample'."""
        cand_lens, target, bt_mask = self._begin_step(t, cand_lens, target, bt_mask, nav, cand_nodes, teacher_mode)
        ml, logp, ent, a_t, env_action, prev_angle = ops.policy_step(
            logit, cand_lens, self.ended, self._row(self.mask, t), mode=feedback, target=target, bt_mask=bt_mask, ob_ang=ob_ang_feats,
            hist_len=self.hist_len, forced_action=forced_action, uniform=uniform, ignoreid=self.ignoreid,
            call_id=(self.call_id + t) & 0xFFFFFFFF, out=tuple(self._row(b_, t) for b_ in (self.ml, self.logp, self.ent)))
        return self._end_step(t, feedback, {"ml": ml, "logp": logp, "ent": ent}, a_t, env_action, prev_angle, nav, cand_nodes, sync, end_on_miss)

    def _row(self, buf, t):
        """row t of one of the [T_max, B] arrays, as a [B] tensor of its own (see _alias)"""
        return _alias(buf, t * self.B, (self.B,))

    def _upload_i32(self, v):
        """an int32 device tensor as it is; a host list uploaded"""
        return v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.int32)).to(self.device, non_blocking=True)

    def _begin_step(self, t, cand_lens, target, bt_mask, nav, cand_nodes, teacher_mode):
        """What precedes the policy launch of step t: the order check, dropping the rows of a step recorded again, the upload of a host
        `cand_lens`, and with `nav` the teacher's slot and the back-track mask of `ops.nav_observe` for whichever of `target` / `bt_mask`
        is None (False = none).  Returns (cand_lens, target, bt_mask) as the launch takes them."""
        me = type(self).__name__
        if t > self.steps or t >= self.T_max:
            raise ops.L.HamtError(f"{me}.step: step {t} after {self.steps} recorded steps (T_max {self.T_max})")
        for rows in self._rows.values():         # (a step recorded again -- the warm-up and the capture of a graphed step -- replaces its row)
            del rows[t:]
        cand_lens = self._upload_i32(cand_lens)
        if nav is not None:
            if cand_nodes is None:
                raise ops.L.HamtError(f"{me}.step: nav= needs cand_nodes (int32 [B, V], the node of every navigable candidate)")
            tgt, btm = ops.nav_observe(nav, t, cand_nodes, cand_lens, self.ended, mode=teacher_mode, ignoreid=self.ignoreid,
                                       target=target is None, bt_mask=bt_mask is None)
            target, bt_mask = (tgt if target is None else target), (btm if bt_mask is None else bt_mask)
        target, bt_mask = (None if target is False else target), (None if bt_mask is False else bt_mask)
        self.target, self.bt_mask = target, bt_mask          # (what this step used: device tensors, for the caller's logs)
        return cand_lens, target, bt_mask

    def _end_step(self, t, feedback, rows, a_t, env_action, prev_angle, nav, cand_nodes, sync, end_on_miss):
        """What follows the policy launch of step t: record its `rows` ({name: [B] autograd tensor}), with `nav` move the episodes and
        write the reward (the launch the episodes' kind asks for), and hand the environment action to the host unless sync=False."""
        for name, r in rows.items():
            self._rows[name].append(r)
        self.feedback = feedback
        if nav is not None:
            kind = getattr(nav, "KIND", "r2r")
            mask, reward = self._row(self.mask, t), self._row(self.reward, t)
            if kind == "r2r":
                ops.nav_advance(nav, cand_nodes, env_action, mask, reward)
            elif kind == "goals":
                ops.nav_advance_goals(nav, cand_nodes, env_action, mask, reward)
            else:
                ops.nav_advance_back(nav, cand_nodes, env_action, mask, reward, self.ended,
                                     end_on_miss=(feedback == "sample") if end_on_miss is None else end_on_miss)
        if not sync:
            return a_t, env_action, prev_angle
        return a_t, self.to_host(env_action), prev_angle

    def to_host(self, env_action):
        """The environment actions of a step (device int32 [B], what `step(..., sync=False)` or a captured step returned) as a numpy view
        of the pinned host buffer: one non-blocking copy, one event wait."""
        self.env_host.copy_(env_action, non_blocking=True)
        self._event.record()
        self._event.synchronize()
        return self.env_host_np

    def set_rewards(self, rewards):
        """The host-computed rewards of the rollout, [T, B] (agent_cmt.py:407-445), uploaded once."""
        r = torch.as_tensor(np.asarray(rewards, dtype=np.float32)) if not torch.is_tensor(rewards) else rewards.to(torch.float32)
        T = r.shape[0]
        assert T == self.steps and r.shape[1] == self.B, (tuple(r.shape), self.steps, self.B)
        self.reward[:T].copy_(r, non_blocking=True)

    def rows(self, t):
        """(ml, logp, ent) of recorded step t: [B] autograd tensors over row t of the recorder's arrays (ent is None unless 'sample')"""
        return self._rows["ml"][t], self._rows["logp"][t], self._rows["ent"][t]

    def stacked(self, name):
        """`ml`, `logp` or `ent` of the recorded steps as one [T, B] autograd tensor over the recorder's own array (no copy)"""
        rows = self._rows[name]
        return _JoinRows.apply(getattr(self, name), len(rows), *rows)

    def loss(self, critic=None, hidden_states=None, last_h=None, train_ml=None, gamma=0.9, entropy_weight=0.01, normalize="total",
             train_rl=True):
        """The rollout's loss (agent_cmt.py:453-522): the A2C loss (`ops.a2c_loss` on the recorder's own arrays) when `train_rl` and the
        feedback was 'sample', plus ml.sum() * train_ml / B when `train_ml` is given.  `hidden_states`: the T per-step states ([T, B, H]
        or a list of [B, H]) the critic values; `last_h` [B, H]: the state after the last step (its value seeds the return of the episodes
        that have not ended, :480-484).  Returns (loss, logs): logs holds device scalars IL_loss, RL_loss, policy, critic, entropy, total."""
        T, B = self.steps, self.B
        loss, logs = 0.0, {}
        if train_rl and self.feedback == "sample":             # (:256-257: teacher / argmax never train the RL loss)
            hs = hidden_states if torch.is_tensor(hidden_states) else torch.cat(list(hidden_states), 0)
            value = critic(hs.reshape(T * B, -1)).reshape(T, B)
            last_value = critic(last_h).detach().reshape(B) * (self.ended == 0).to(torch.float32)
            mask = _alias(self.mask, 0, (T, B))
            rl, parts = ops.a2c_loss(self.stacked("logp"), value, _alias(self.reward, 0, (T, B)), mask, last_value=last_value,
                                     entropy=self.stacked("ent"), gamma=gamma, entropy_weight=entropy_weight, normalize=normalize)
            loss = loss + rl
            logs.update(RL_loss=rl.detach(), total=mask.sum(), **parts)
        if train_ml is not None:
            il = self.stacked("ml").sum() * (float(train_ml) / B)
            loss = loss + il
            logs["IL_loss"] = il.detach()
        return loss, logs
