#!/usr/bin/env python3
"""Generate tests/golden/policy_step.npz by running the REFERENCE agent's own statements (finetune_src/r2r/agent_cmt.py) on scripted
rollouts, CPU, fp32.

Test infrastructure, like tools/gen_reverie_golden.py (needs the reference checkout, oracle.ref_shim.REF):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_policy_step_golden.py

The statements sit inline in `Seq2SeqCMTAgent.rollout`, a 280-line method that needs the Matterport simulator for everything around
them; as oracle/gen_goldens.py::_reference_a2c_block does for the A2C block, the blocks below are cut out of the reference FILE at
generation time (located by their first and last statement, not by line number) and compiled -- nothing of them is restated here:
  step    `if train_ml is not None:` ... `cpu_a_t[i] = -1` (:336-375): imitation loss, back-track mask, the three feedback modes,
          the environment action;
  angle   `prev_act_angle = np.zeros(...)` ... the candidate loop (:382-385);
  hist    the `hist_lens` loop (:399-401);     ended   `ended[:] = np.logical_or(...)` (:447);
  a2c     `rl_loss = 0.` ... `self.loss += rl_loss` (:476-517, oracle.gen_goldens._reference_a2c_block);
  il      `if train_ml is not None:` ... `self.logs['IL_loss'].append(...)` (:520-522).
What is scripted: the logits (B 6, T 5, V 9, ragged candidate counts, -inf at non-candidates), the observations (viewpoint names
whose re-visits make the back-track mask, candidate features), the teacher's answers, the rewards, the hidden states (through the
reference's Critic).  Cases: `sample_<normalize>` for the three normalize_loss settings (train_ml 0.2, RL on), `teacher` (train_ml 1)
and `argmax` (train_ml 0.5; the reference never trains on the argmax log-probabilities, so a scripted weight per (t, b) takes their
gradient: loss += sum w * log pi).  In `sample` the draw comes from torch's stream (seeded); three of them are scripted -- two STOPs
that end episodes early and one slot whose logit lies 40 below the row maximum (probability under FLT_EPSILON: the clamp of
Categorical(probs)) -- by answering `Categorical.sample` for those rows.  The recorded a_t goes into the tests as `forced_action`.
"""
import os
import sys
import textwrap
import types
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import ref_shim                                            # noqa: E402
from oracle.gen_goldens import _reference_a2c_block                    # noqa: E402
from oracle.hamt_oracle import make_state_dict                         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "policy_step.npz")
B, T, V, A, HS = 6, 5, 9, 4, 768
IGNORE = -100
CRITIC_SEED, HIDDEN_SEED = 12, 91
CAND_LEN = np.array([[5, 9, 3, 7, 2, 6], [4, 8, 6, 7, 3, 9], [6, 5, 9, 4, 2, 7], [3, 9, 5, 8, 4, 6], [7, 6, 4, 9, 5, 3]], np.int32)    # [T, B], STOP slot included


def _block(lines, first, last, start=0):
    lo = next(i for i, ln in enumerate(lines) if i >= start and ln.strip().startswith(first))
    hi = next(i for i, ln in enumerate(lines) if i >= lo and ln.strip().startswith(last))
    return textwrap.dedent("\n".join(lines[lo:hi + 1])), (lo + 1, hi + 1)


def reference_blocks():
    path = os.path.join(ref_shim.REF, "finetune_src", "r2r", "agent_cmt.py")
    lines = open(path).read().split("\n")
    loop = next(i for i, ln in enumerate(lines) if ln.strip() == "for t in range(self.args.max_action_len):")
    src, spans = {}, {}
    src["step"], spans["step"] = _block(lines, "if train_ml is not None:", "cpu_a_t[i] = -1", loop)
    src["angle"], spans["angle"] = _block(lines, "prev_act_angle = np.zeros(", "prev_act_angle[i] = obs[i]['candidate'][next_id]['feature']", loop)
    src["hist"], spans["hist"] = _block(lines, "for i, i_ended in enumerate(ended):", "hist_lens[i] += 1", loop)
    src["ended"], spans["ended"] = _block(lines, "ended[:] = np.logical_or(ended, (cpu_a_t == -1))", "ended[:] = np.logical_or(ended, (cpu_a_t == -1))", loop)
    tail = next(i for i, ln in enumerate(lines) if ln.strip() == "self.loss += rl_loss")
    src["il"], spans["il"] = _block(lines, "if train_ml is not None:", "self.logs['IL_loss'].append(", tail)
    assert "self.criterion(logit, target)" in src["step"] and "torch.distributions.Categorical(probs)" in src["step"] and "masked_fill_" in src["step"]
    assert "ml_loss * train_ml / batch_size" in src["il"], "agent_cmt.py changed"
    code = {k: compile(v, f"{path}:{spans[k][0]}-{spans[k][1]}", "exec") for k, v in src.items()}
    code["a2c"], spans["a2c"] = _reference_a2c_block()
    return code, spans


def script(seed=23):
    """the scripted rollout: logits, observations, teacher answers, scripted draws, rewards"""
    rng = np.random.Generator(np.random.PCG64(seed))
    logits = (rng.standard_normal((T, B, V)) * 2.0).astype(np.float32)
    feats = rng.standard_normal((T, B, V, 3 + A)).astype(np.float32)
    for t in range(T):
        for b in range(B):
            logits[t, b, CAND_LEN[t, b]:] = -np.inf
            feats[t, b, CAND_LEN[t, b] - 1:] = 0.0                   # (the STOP slot and the padding carry no candidate)
    logits[2, 1, CAND_LEN[2, 1] - 1] = 9.0                            # argmax feedback: episode 1 stops at t = 2
    logits[1, 4, CAND_LEN[1, 4] - 1] = 9.0                            # ... and episode 4 at t = 1
    corner = (2, 2, 3)                                                # (t, b, slot): 40 below the row maximum, taken as a scripted draw
    logits[2, 2, 3] = np.delete(logits[2, 2, :CAND_LEN[2, 2]], 3).max() - 40.0
    # observations: episode b stands at viewpoint "b.t" at step t; candidate j leads to "b.t.j" unless scripted as a re-visit
    revisit = {}
    for t in range(1, T):
        for b in range(B):
            row = logits[t, b, :CAND_LEN[t, b] - 1]                   # navigable slots only (never the STOP slot)
            if row.size and (t + b) % 2 == 0:
                j = int(row.argmax())                                 # the best navigable slot leads back to where the episode was
                revisit[(t, b, j)] = f"{b}.{t - 1}"
    obs_all = []
    for t in range(T):
        obs = []
        for b in range(B):
            cands = [{"viewpointId": revisit.get((t, b, j), f"{b}.{t}.{j}"), "feature": feats[t, b, j]} for j in range(CAND_LEN[t, b] - 1)]
            obs.append({"viewpoint": f"{b}.{t}", "candidate": cands})
        obs_all.append(obs)
    teacher = np.stack([rng.integers(0, np.maximum(CAND_LEN[t] - 1, 1)) for t in range(T)]).astype(np.int64)     # a navigable slot ...
    teacher[1, 0] = CAND_LEN[1, 0] - 1                                # ... or STOP: teacher feedback ends episode 0 at t = 1
    teacher[3, 3] = CAND_LEN[3, 3] - 1                                # and episode 3 at t = 3
    teacher[2, 5] = CAND_LEN[2, 5] - 1
    draws = {(1, 0): int(CAND_LEN[1, 0] - 1), (3, 3): int(CAND_LEN[3, 3] - 1), (0, 2): 0, (1, 2): 0, corner[:2]: corner[2]}    # sample feedback: scripted draws (episode 2 walks on to the corner)
    for t in range(T):                                                # episodes 1 and 5 never stop (their return is seeded by the critic): a navigable,
        for b in (1, 5):                                              # unmasked slot
            draws[(t, b)] = 1 if (t, b, 0) in revisit else 0
    rewards = (rng.standard_normal((T, B)) * 2.0).astype(np.float32)
    weights = rng.standard_normal((T, B)).astype(np.float32)
    return dict(logits=logits, ob_ang=np.ascontiguousarray(feats[..., -A:]), obs=obs_all, teacher=teacher, draws=draws, rewards=rewards,
                weights=weights)


def hidden_states(seed=HIDDEN_SEED):
    """the critic's inputs, rebuilt by the tests from the seed (not stored: 100 KB of noise)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((T, B, HS), dtype=np.float32) * 0.5, rng.standard_normal((B, HS), dtype=np.float32) * 0.5


def run_case(code, sc, critic, feedback, normalize, train_ml, backtrack):
    logit_leaf = torch.from_numpy(sc["logits"]).requires_grad_(True)
    hid, last_h = hidden_states()
    hidden = torch.from_numpy(hid).requires_grad_(True)
    critic.zero_grad(set_to_none=True)
    ended = np.array([False] * B)
    state = {"t": 0}

    def teacher_action(obs, ended_):
        a = sc["teacher"][state["t"]].copy()
        a[ended_] = IGNORE                                            # (_teacher_action: an ended episode has no target)
        return torch.from_numpy(a)

    me = types.SimpleNamespace(critic=critic, feedback=feedback, logs=defaultdict(list), loss=0,
                               criterion=torch.nn.CrossEntropyLoss(ignore_index=IGNORE, reduction="sum"),       # agent_cmt.py: size_average=False
                               _teacher_action=teacher_action,
                               args=types.SimpleNamespace(gamma=0.9, entropy_loss_weight=0.01, normalize_loss=normalize, ignoreid=IGNORE,
                                                          no_cand_backtrack=backtrack, angle_feat_size=A, max_action_len=T))
    orig_sample, orig_cpu = torch.distributions.Categorical.sample, torch.Tensor.cpu

    def scripted_sample(self_, *a, **k):
        s = orig_sample(self_, *a, **k)
        for (t_, b_), v in sc["draws"].items():
            if t_ == state["t"]:
                s[b_] = v
        return s

    ns = {"self": me, "np": np, "torch": torch, "F": F, "sys": sys, "train_ml": train_ml, "train_rl": feedback == "sample", "batch_size": B,
          "ended": ended, "ml_loss": 0., "visited": [set() for _ in range(B)], "policy_log_probs": [], "entropys": [], "hist_lens": [1] * B,
          "ob_nav_types": torch.zeros(B, V, dtype=torch.long), "rewards": [], "masks": [], "hidden_states": [hidden[t] for t in range(T)],
          "last_h_": torch.from_numpy(last_h)}
    per = defaultdict(list)
    torch.manual_seed(1234)
    torch.distributions.Categorical.sample = scripted_sample
    torch.Tensor.cpu = lambda t_, *a, **k: t_.detach().clone()      # (`a_t.cpu()` is a COPY on the reference's path: the -1 edits never reach a_t)
    try:
        with ref_shim.cuda_is_identity():
            for t in range(T):
                state["t"] = t
                ns.update(t=t, obs=sc["obs"][t], ob_cand_lens=[int(c) for c in CAND_LEN[t]], logit=logit_leaf[t].clone())
                n_lp, ml_before = len(ns["policy_log_probs"]), float(ns["ml_loss"])       # (a float: `ml_loss +=` is in place from t = 1 on)
                exec(code["step"], ns)
                exec(code["angle"], ns)
                exec(code["hist"], ns)
                mask = (~ns["ended"]).astype(np.float32)              # :418-420 (inside the simulator-bound reward loop: 0 where ended)
                ns["rewards"].append(sc["rewards"][t] * mask)
                ns["masks"].append(mask)
                per["mask"].append(mask)
                per["target"].append(ns["target"].numpy().copy() if train_ml is not None else np.full(B, IGNORE, np.int64))
                per["bt_mask"].append(ns["bt_masks"].numpy().astype(np.uint8) if backtrack else np.zeros((B, V), np.uint8))
                per["a_t"].append(ns["a_t"].numpy().astype(np.int64).copy())
                per["env_action"].append(ns["cpu_a_t"].astype(np.int32).copy())
                per["prev_angle"].append(ns["prev_act_angle"].copy())
                per["ml_sum"].append(np.float32(float(ns["ml_loss"].detach()) - ml_before) if train_ml is not None else np.float32(0))
                if len(ns["policy_log_probs"]) > n_lp:
                    per["logp"].append(ns["policy_log_probs"][-1].detach().reshape(B).numpy().copy())
                else:
                    per["logp"].append(np.zeros(B, np.float32))
                per["ent"].append(ns["entropys"][-1].detach().numpy().copy() if feedback == "sample" else np.zeros(B, np.float32))
                exec(code["ended"], ns)
                per["ended"].append(ns["ended"].copy())
                per["hist_len"].append(np.array(ns["hist_lens"], np.int32))
            if feedback == "sample":
                exec(code["a2c"], ns)
                rl_loss_value = float(me.loss.detach())               # (what :518 logs as RL_loss: the block ends one statement earlier)
            exec(code["il"], ns)
    finally:
        torch.distributions.Categorical.sample, torch.Tensor.cpu = orig_sample, orig_cpu
    loss = me.loss
    if feedback == "argmax":                                          # (see the module docstring)
        w = torch.from_numpy(sc["weights"])
        loss = loss + sum((w[t] * ns["policy_log_probs"][t].reshape(B)).sum() for t in range(T))
    loss.backward()
    out = {k: np.stack(v) for k, v in per.items()}
    out["loss"] = np.float64(loss.item())
    out["d_logit"] = logit_leaf.grad.numpy().copy()
    out["IL_loss"] = np.float64(me.logs["IL_loss"][0])
    if feedback == "sample":
        out["RL_loss"] = np.float64(rl_loss_value)
        out["policy_sum"] = np.float64(sum(me.logs["policy_loss"]))
        out["critic_sum"] = np.float64(sum(me.logs["critic_loss"]))
        out["total"] = np.float64(me.logs["total"][0])
        # the entropy term of :501 summed over the rollout (the reference adds it to rl_loss without logging it), from its own lists
        out["entropy_sum"] = np.float64(sum(float((-me.args.entropy_loss_weight * ns["entropys"][t].detach() * torch.from_numpy(ns["masks"][t])).sum())
                                            for t in range(T)))
        out["entropy_logged"] = np.float64(sum(me.logs["entropy"]))     # :363, c.entropy().sum() of every step, unmasked
        out["d_hidden_norm"] = hidden.grad.double().flatten(1).norm(dim=1).numpy()
        for k, p_ in critic.named_parameters():
            out["d_critic_norm/" + k] = np.float64(p_.grad.double().norm().item())
    return out


def main():
    code, spans = reference_blocks()
    _, mh = ref_shim.import_finetune_agent_models()
    critic = mh.Critic(types.SimpleNamespace(dropout=0.5))
    critic.load_state_dict(make_state_dict({"state2value.0.weight": (512, 768), "state2value.0.bias": (512,), "state2value.3.weight": (1, 512),
                                            "state2value.3.bias": (1,)}, seed=CRITIC_SEED), strict=True)
    critic.eval()
    sc = script()
    store = {"meta/critic_seed": np.array(CRITIC_SEED), "meta/hidden_seed": np.array(HIDDEN_SEED), "meta/ignoreid": np.array(IGNORE),
             "in/logits": sc["logits"], "in/ob_ang": sc["ob_ang"], "in/cand_len": CAND_LEN, "in/rewards": sc["rewards"], "in/weights": sc["weights"]}
    for k, v in spans.items():
        store["meta/span/" + k] = np.asarray(v)
    cases = [(f"sample_{n}", "sample", n, 0.2, True) for n in ("total", "batch", "none")] + [("teacher", "teacher", "total", 1.0, False),
                                                                                            ("argmax", "argmax", "total", 0.5, True)]
    for tag, feedback, normalize, train_ml, backtrack in cases:
        out = run_case(code, sc, critic, feedback, normalize, train_ml, backtrack)
        store[f"{tag}/train_ml"] = np.float64(train_ml)
        for k, v in out.items():
            store[f"{tag}/{k}"] = v
        print(f"  [{tag}] loss {float(out['loss']):.6f}; ended {out['ended'][-1].astype(int)}; masked slots {int(out['bt_mask'].sum())}; "
              f"min logp {float(out['logp'].min()):.4f}")
    # the scripted corners are really there
    am = store["argmax/bt_mask"].astype(bool)
    raw_best = np.where(np.isfinite(sc["logits"]), sc["logits"], -np.inf).argmax(2)
    assert int(np.take_along_axis(am, raw_best[..., None], 2).sum()) >= 3, "no back-track mask on a would-be argmax"
    assert abs(float(store["sample_total/logp"][2, 2]) - float(np.log(np.finfo(np.float32).eps))) < 1e-6, "the clamp corner is not clamped"
    assert store["sample_total/ended"][-1].sum() >= 2 and not store["sample_total/ended"][-1].all()
    np.savez_compressed(OUT, **store)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(store)} arrays, {os.path.getsize(OUT)} bytes; spans {spans}")


if __name__ == "__main__":
    main()
