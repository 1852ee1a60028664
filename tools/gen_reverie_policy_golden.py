#!/usr/bin/env python3
"""Generate tests/golden/reverie_policy.npz by running the REFERENCE REVERIE agent's own statements (finetune_src/reverie/agent.py) on a
scripted rollout, CPU, fp32.

Test infrastructure, like tools/gen_policy_step_golden.py (needs the reference checkout, oracle.ref_shim.REF):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_reverie_policy_golden.py

The blocks below are cut out of the reference FILE at generation time (located by their first and last statement, not by line number)
and compiled -- nothing of them is restated here:
  teacher `def _teacher_action(self, obs, ended, ob_img_max_len):` ... its `return` (:141-165): the action AND the object target;
  step    `_, max_obj_logits = torch.max(obj_logits, 1)` ... `cpu_a_t[i] = -1` (:253-307; `t_outputs = ...` in front of it excluded):
          the object column, back-track mask, both cross-entropies, the three feedback modes, the predicted object, the environment action;
  angle   `prev_act_angle = np.zeros(...)` ... the candidate loop (:311-314);
  hist    the `hist_lens` loop (:328-330);     ended   `ended[:] = np.logical_or(...)` (:368);
  a2c     `rl_loss = 0.` ... `self.loss += rl_loss` (:404-445), for the `sample` case;
  il      `if train_ml is not None:` ... `self.logs['REF_loss'].append(...)` (:448-451).
What is scripted: both logits (B 6, T 4, V 9, O 5; ragged navigable and object counts, -inf behind them, an empty object list padded to
one slot as `_object_variable` does), the observations (viewpoint names whose re-visits make the back-track mask, candidate features,
object ids, the goal object), the teacher's viewpoint, the rewards, the hidden states.  Cases: `teacher` (train_ml 1), `argmax` (train_ml
0.5, back-track mask, a scripted weight per (t, b) on log pi takes the gradient the reference never asks for) and `sample` (train_ml 0.2,
back-track mask, A2C through the reference's Critic; the draws come from torch's seeded stream, some scripted by answering
`Categorical.sample`).  The recorded a_t goes into the tests as `forced_action`.
"""
import os
import sys
import types
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

from gen_policy_step_golden import _block                             # noqa: E402
from oracle import ref_shim                                            # noqa: E402
from oracle.hamt_oracle import make_state_dict                         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reverie_policy.npz")
B, T, V, O, A, HS = 6, 4, 9, 5, 4, 768
IGNORE = -100
CRITIC_SEED, HIDDEN_SEED = 12, 57
N_NAV = np.array([[4, 8, 2, 6, 1, 5], [3, 7, 5, 6, 2, 8], [5, 4, 8, 3, 1, 6], [2, 8, 4, 7, 3, 5]], np.int32)       # [T, B] navigable candidates
OBJ_LEN = np.array([[3, 5, 1, 4, 2, 5], [2, 4, 5, 0, 3, 1], [5, 3, 4, 2, 0, 4], [1, 5, 0, 3, 4, 2]], np.int32)     # [T, B] true object counts
GOAL = [901, 902, 903, 904, 905, 906]                                  # each episode's goal object


def reference_blocks():
    path = os.path.join(ref_shim.REF, "finetune_src", "reverie", "agent.py")
    lines = open(path).read().split("\n")
    loop = next(i for i, ln in enumerate(lines) if ln.strip() == "for t in range(self.args.max_action_len):")
    src, spans = {}, {}
    src["teacher"], spans["teacher"] = _block(lines, "def _teacher_action(self, obs, ended, ob_img_max_len):", "return torch.from_numpy(a).cuda(), torch.from_numpy(ref).cuda()")
    src["step"], spans["step"] = _block(lines, "_, max_obj_logits = torch.max(obj_logits, 1)", "cpu_a_t[i] = -1", loop)
    src["angle"], spans["angle"] = _block(lines, "prev_act_angle = np.zeros(", "prev_act_angle[i] = obs[i]['candidate'][next_id]['feature']", loop)
    src["hist"], spans["hist"] = _block(lines, "for i, i_ended in enumerate(ended):", "hist_lens[i] += 1", loop)
    src["ended"], spans["ended"] = _block(lines, "ended[:] = np.logical_or(ended, (cpu_a_t == -1))", "ended[:] = np.logical_or(ended, (cpu_a_t == -1))", loop)
    src["a2c"], spans["a2c"] = _block(lines, "rl_loss = 0.", "self.loss += rl_loss", loop)
    tail = next(i for i, ln in enumerate(lines) if ln.strip() == "self.loss += rl_loss")
    src["il"], spans["il"] = _block(lines, "if train_ml is not None:", "self.logs['REF_loss'].append(", tail)
    assert "self.criterion(obj_logits, ref_target)" in src["step"] and "masked_fill_" in src["step"] and "predObjId" in src["step"]
    assert src["step"].index("masked_fill_") < src["step"].index("self.criterion(act_logits, target)"), "the mask no longer precedes the CE"
    assert "ml_loss * train_ml / batch_size + ref_loss / batch_size" in src["il"], "reverie/agent.py changed"
    assert "last_value__ = self.critic(last_h_).detach()" in src["a2c"]
    code = {k: compile(v, f"{path}:{spans[k][0]}-{spans[k][1]}", "exec") for k, v in src.items()}
    return code, spans


def script(seed=41):
    """the scripted rollout: logits, observations (with the teacher's viewpoint and the objects), scripted draws, rewards"""
    rng = np.random.Generator(np.random.PCG64(seed))
    act = (rng.standard_normal((T, B, V)) * 2.0 + 2.0).astype(np.float32)        # (+2: the STOP column holds an index 0..4)
    obj = (rng.standard_normal((T, B, O)) * 2.0).astype(np.float32)
    feats = rng.standard_normal((T, B, V, 3 + A)).astype(np.float32)
    for t in range(T):
        for b in range(B):
            act[t, b, N_NAV[t, b]:] = -np.inf                         # panorama context: not navigable
            feats[t, b, N_NAV[t, b]:] = 0.0
            obj[t, b, max(OBJ_LEN[t, b], 1):] = -np.inf               # (_object_variable pads an empty list to one slot)
    act[1, 4, :N_NAV[1, 4]] = [-2.5, -3.0]                            # argmax feedback: episode 4 stops at t = 1 (no navigable logit above the index) ...
    act[2, 1, :N_NAV[2, 1]] -= 9.0                                    # ... and episode 1 at t = 2
    for t, b in ((0, 4), (0, 1), (1, 1)):                             # (and not before)
        act[t, b, 0] = 7.5
    for t in range(T):                                                # episodes 0 and 5 never stop by themselves: the last step forces their prediction
        for b in (0, 5):
            act[t, b, 1] = 8.0 + 0.25 * t
    # observations: episode b stands at viewpoint "b.t" at step t; candidate j leads to "b.t.j" unless scripted as a re-visit
    revisit = {}
    for t in range(1, T):
        for b in range(B):
            row = act[t, b, :N_NAV[t, b]]
            if (t + b) % 2 == 0 and N_NAV[t, b] > 1:                  # (a lone candidate stays open: the teacher never leads back)
                revisit[(t, b, int(row.argmax()))] = f"{b}.{t - 1}"     # the best navigable slot leads back to where the episode was
    # the teacher: a navigable slot, or STOP (its viewpoint is the episode's own)
    teach = np.stack([rng.integers(0, N_NAV[t]) for t in range(T)]).astype(np.int64)
    stops = {(1, 0), (2, 2), (3, 5), (1, 3), (3, 1)}                   # (t, b): teacher STOP; (1, 0): goal absent; (1, 3): no object in view
    obj_ids = np.zeros((T, B, O), np.int32)
    obs_all = []
    for t in range(T):
        obs = []
        for b in range(B):
            cands = [{"viewpointId": revisit.get((t, b, j), f"{b}.{t}.{j}"), "feature": feats[t, b, j]} for j in range(N_NAV[t, b])]
            ids = [1000 + 100 * t + 10 * b + k for k in range(OBJ_LEN[t, b])]
            if ids and (t, b) != (1, 0):
                ids[int(rng.integers(0, len(ids)))] = GOAL[b]         # the goal is in view (everywhere but at episode 0's teacher STOP)
            obj_ids[t, b, :len(ids)] = ids
            vp = f"{b}.{t}"
            j = int(teach[t, b])
            while (t, b) not in stops and (t, b, j) in revisit:       # (the teacher never leads back)
                j = (j + 1) % N_NAV[t, b]
            teacher_vp = vp if (t, b) in stops else cands[j]["viewpointId"]
            obs.append({"viewpoint": vp, "teacher": teacher_vp, "objId": str(GOAL[b]), "candidate": cands, "candidate_obj": ([], [], ids)})
        obs_all.append(obs)
    draws = {(1, 0): V, (2, 3): V, (0, 2): 0, (1, 2): 0}               # sample feedback: scripted draws (two STOPs that end episodes early)
    for t in range(T):
        for b in (1, 5):                                              # episodes 1 and 5 walk on: a navigable, unmasked slot
            draws[(t, b)] = 1 if (t, b, 0) in revisit else 0
    rewards = (rng.standard_normal((T, B)) * 2.0).astype(np.float32)
    weights = rng.standard_normal((T, B)).astype(np.float32)
    return dict(act=act, obj=obj, ob_ang=np.ascontiguousarray(feats[..., -A:]), obs=obs_all, obj_ids=obj_ids, draws=draws, rewards=rewards,
                weights=weights)


def hidden_states(seed=HIDDEN_SEED):
    """the critic's inputs, rebuilt by the tests from the seed (tests/_policy_ref.py::golden_hidden)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((T, B, HS), dtype=np.float32) * 0.5, rng.standard_normal((B, HS), dtype=np.float32) * 0.5


def run_case(code, sc, critic, feedback, train_ml, backtrack):
    act_leaf = torch.from_numpy(sc["act"]).requires_grad_(True)
    obj_leaf = torch.from_numpy(sc["obj"]).requires_grad_(True)
    hid, last_h = hidden_states()
    hidden = torch.from_numpy(hid)
    critic.zero_grad(set_to_none=True)
    ended = np.array([False] * B)
    state = {"t": 0}
    me = types.SimpleNamespace(critic=critic, feedback=feedback, logs=defaultdict(list), loss=0,
                               criterion=torch.nn.CrossEntropyLoss(ignore_index=IGNORE, reduction="sum"),       # r2r/agent_cmt.py: size_average=False
                               args=types.SimpleNamespace(gamma=0.9, entropy_loss_weight=0.01, normalize_loss="total", ignoreid=IGNORE,
                                                          no_cand_backtrack=backtrack, angle_feat_size=A, max_action_len=T))
    tns = {"np": np, "torch": torch}
    exec(code["teacher"], tns)
    me._teacher_action = types.MethodType(tns["_teacher_action"], me)
    orig_sample, orig_cpu = torch.distributions.Categorical.sample, torch.Tensor.cpu

    def scripted_sample(self_, *a, **k):
        s = orig_sample(self_, *a, **k)
        for (t_, b_), v in sc["draws"].items():
            if t_ == state["t"]:
                s[b_] = v
        return s

    traj = [{"predObjId": str(None)} for _ in range(B)]
    ns = {"self": me, "np": np, "torch": torch, "F": F, "sys": sys, "train_ml": train_ml, "train_rl": feedback == "sample", "batch_size": B,
          "ended": ended, "ml_loss": 0., "ref_loss": 0., "visited": [set() for _ in range(B)], "policy_log_probs": [], "entropys": [],
          "hist_lens": [1] * B, "rewards": [], "masks": [], "hidden_states": [], "last_h_": torch.from_numpy(last_h), "traj": traj,
          "ob_img_max_len": V}
    per = defaultdict(list)
    torch.manual_seed(4321)
    torch.distributions.Categorical.sample = scripted_sample
    torch.Tensor.cpu = lambda t_, *a, **k: t_.detach().clone()      # (`a_t.cpu()` is a COPY on the reference's path: the -1 edits never reach a_t)
    try:
        with ref_shim.cuda_is_identity():
            for t in range(T):
                state["t"] = t
                ns.update(t=t, obs=sc["obs"][t], act_logits=act_leaf[t].clone(), obj_logits=obj_leaf[t].clone(),
                          obj_lens=[max(int(n), 1) for n in OBJ_LEN[t]], t_outputs={"states": hidden[t]})
                n_lp, ml_before, ref_before = len(ns["policy_log_probs"]), float(torch.as_tensor(ns["ml_loss"]).detach()), float(torch.as_tensor(ns["ref_loss"]).detach())
                exec(code["step"], ns)
                exec(code["angle"], ns)
                exec(code["hist"], ns)
                mask = (~ns["ended"]).astype(np.float32)              # :340-346 (inside the simulator-bound reward loop: 0 where ended)
                ns["rewards"].append(sc["rewards"][t] * mask)
                ns["masks"].append(mask)
                per["mask"].append(mask)
                per["target"].append(ns["target"].numpy().copy())
                per["ref_target"].append(ns["ref_target"].numpy().copy())
                btm = ns["bt_masks"].numpy().astype(np.uint8) if backtrack else np.zeros((B, V + 1), np.uint8)
                assert btm.shape == (B, V + 1) and not btm[:, V].any()  # the mask covers the V + 1 row and is never set on column V
                per["bt_mask"].append(np.ascontiguousarray(btm[:, :V]))
                per["stop_col"].append(ns["act_logits"].detach().numpy()[:, V].copy())
                per["a_t"].append(ns["a_t"].numpy().astype(np.int64).copy())
                per["env_action"].append(ns["cpu_a_t"].astype(np.int32).copy())
                per["prev_angle"].append(ns["prev_act_angle"].copy())
                per["ml_sum"].append(np.float32(float(ns["ml_loss"].detach()) - ml_before))
                per["ref_sum"].append(np.float32(float(ns["ref_loss"].detach()) - ref_before))
                if len(ns["policy_log_probs"]) > n_lp:
                    per["logp"].append(ns["policy_log_probs"][-1].detach().reshape(B).numpy().copy())
                else:
                    per["logp"].append(np.zeros(B, np.float32))
                per["ent"].append(ns["entropys"][-1].detach().numpy().copy() if feedback == "sample" else np.zeros(B, np.float32))
                per["pred_obj_id"].append(np.array([-1 if tr["predObjId"] == str(None) else int(tr["predObjId"]) for tr in traj], np.int32))
                exec(code["ended"], ns)
                per["ended"].append(ns["ended"].copy())
                per["hist_len"].append(np.array(ns["hist_lens"], np.int32))
            if feedback == "sample":
                exec(code["a2c"], ns)
                rl_loss_value = float(me.loss.detach())
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
    out["d_act"] = act_leaf.grad.numpy().copy()
    out["d_obj"] = obj_leaf.grad.numpy().copy() if obj_leaf.grad is not None else np.zeros_like(sc["obj"])
    out["IL_loss"] = np.float64(me.logs["IL_loss"][0])
    out["REF_loss"] = np.float64(float(me.logs["REF_loss"][0]))
    if feedback == "sample":
        out["RL_loss"] = np.float64(rl_loss_value)
        out["total"] = np.float64(me.logs["total"][0])
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
             "in/act_logits": sc["act"], "in/obj_logits": sc["obj"], "in/ob_ang": sc["ob_ang"], "in/cand_len": N_NAV + 1, "in/obj_len": OBJ_LEN,
             "in/obj_ids": sc["obj_ids"], "in/goal_obj": np.array(GOAL, np.int32), "in/rewards": sc["rewards"], "in/weights": sc["weights"]}
    for k, v in spans.items():
        store["meta/span/" + k] = np.asarray(v)
    for tag, train_ml, backtrack in (("teacher", 1.0, False), ("argmax", 0.5, True), ("sample", 0.2, True)):
        out = run_case(code, sc, critic, tag, train_ml, backtrack)
        store[f"{tag}/train_ml"] = np.float64(train_ml)
        for k, v in out.items():
            store[f"{tag}/{k}"] = v
        print(f"  [{tag}] loss {float(out['loss']):.6f} IL {float(out['IL_loss']):.6f} REF {float(out['REF_loss']):.6f}; ended {out['ended'].astype(int).tolist()}; "
              f"masked slots {int(out['bt_mask'].sum())}; pred {out['pred_obj_id'][-1].tolist()}; a_t {out['a_t'].tolist()}")
    # the scripted corners are really there
    t_ = store["teacher/target"]
    assert t_[1, 0] == V and store["teacher/ref_target"][1, 0] == IGNORE, "teacher STOP with the goal absent"
    assert store["teacher/ref_target"][2, 2] >= 0 and store["teacher/ref_sum"][2] > 0
    assert store["teacher/pred_obj_id"][-1][3] == -1 and OBJ_LEN[1, 3] == 0, "a STOP at a viewpoint without objects predicts None"
    for tag in ("teacher", "argmax", "sample"):
        e = store[f"{tag}/ended"]
        assert e[1].any() and not e[-2].all(), (tag, "an early stop, and episodes the last step forces")
        forced = ~e[-2] & (store[f"{tag}/a_t"][-1] < V)
        assert (store[f"{tag}/pred_obj_id"][-1][forced & (OBJ_LEN[-1] > 0)] >= 0).all() and forced.any(), (tag, "forced last-step prediction")
    assert store["argmax/bt_mask"].sum() >= 3 and store["sample/bt_mask"].sum() >= 3
    am = store["argmax/bt_mask"].astype(bool)
    raw_best = np.concatenate([sc["act"], store["argmax/stop_col"][..., None]], 2).argmax(2)
    assert int(np.take_along_axis(np.concatenate([am, np.zeros((T, B, 1), bool)], 2), raw_best[..., None], 2).sum()) >= 2, "no mask on a would-be argmax"
    np.savez_compressed(OUT, **store)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(store)} arrays, {os.path.getsize(OUT)} bytes; spans {spans}")


if __name__ == "__main__":
    main()
