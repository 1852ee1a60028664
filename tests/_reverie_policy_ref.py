"""A small torch restatement of one rollout step of REVERIE's agent (finetune_src/reverie/agent.py:253-307, 311-314, 328-330, 368) and of
its imitation / object losses (:448-451), for the tests of ops.policy_ref_step / agent.ReverieRolloutRecorder.  Test infrastructure:
pinned against the reference's own statements by tests/golden/reverie_policy.npz (tools/gen_reverie_policy_golden.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from _policy_ref import inverse_cdf

MODES = ("teacher", "argmax", "sample")


def lowest_argmax(x):
    """the lowest index among the maxima of every row (the kernel's documented tie rule), int64 [B]"""
    hit = x == x.max(1, keepdim=True)[0]
    return torch.where(hit, torch.arange(x.shape[1])[None], x.shape[1]).min(1)[0]


def ref_target_from_ids(target_eff, obj_id, goal_obj, obj_len, ended, V, ignoreid=-100):
    """_teacher_action's second answer (:150-160): the goal object's first slot where the teacher says STOP, else ignoreid"""
    out = np.full(len(goal_obj), ignoreid, np.int64)
    for i in range(len(goal_obj)):
        if int(target_eff[i]) == V and not ended[i]:
            hit = np.nonzero(np.asarray(obj_id[i, :obj_len[i]]) == goal_obj[i])[0]
            if hit.size:
                out[i] = hit[0]
    return out


def reverie_step_ref(act_logit, obj_logit, obj_len, cand_len, ended, mode, stop_logit="index", target=None, ref_target=None, obj_id=None,
                     goal_obj=None, bt_mask=None, ob_ang=None, forced_action=None, uniform=None, last_step=False, ignoreid=-100):
    """act_logit [B, V], obj_logit [B, O] (either may require grad); obj_len / cand_len / ended numpy [B].  Returns a dict of the step's
    values: ml, ref per row; pred_obj = -1 for None, -2 where the step records no prediction."""
    B, V = act_logit.shape
    best = lowest_argmax(obj_logit.detach())                                                              # :253
    if stop_logit == "index":
        col = best.to(torch.float32)                                                                      # (the indices: no gradient)
    else:
        col = obj_logit.gather(1, best[:, None]).squeeze(1)
    x = torch.cat([act_logit, col[:, None]], 1)                                                           # :254
    if bt_mask is not None:                                                                               # :269, never on column V
        x = x.masked_fill(torch.cat([torch.as_tensor(bt_mask).bool(), torch.zeros(B, 1, dtype=torch.bool)], 1), -float("inf"))
    out = {"stop_col": col.detach(), "best": best}
    teff = None
    if target is not None:
        cl = torch.as_tensor(np.asarray(cand_len), dtype=torch.int64)
        teff = torch.where((target != ignoreid) & (target >= cl - 1), torch.full_like(target, V), target)  # STOP written as V or as cand_len - 1
        out["ml"] = F.cross_entropy(x, teff, ignore_index=ignoreid, reduction="none")                     # :274, on the masked row
    else:
        out["ml"] = torch.zeros(B)
    if ref_target is None and obj_id is not None and teff is not None:
        ref_target = torch.from_numpy(ref_target_from_ids(teff.numpy(), np.asarray(obj_id), np.asarray(goal_obj), obj_len, ended, V, ignoreid))
    out["ref"] = F.cross_entropy(obj_logit, ref_target, ignore_index=ignoreid, reduction="none") if ref_target is not None else torch.zeros(B)   # :275
    out["ref_target"] = ref_target
    ent = None
    if mode == "teacher":
        a_t = teff if forced_action is None else forced_action                                            # :279
        logp = torch.zeros(B)
    elif mode == "argmax":
        a_t = x.max(1)[1].detach() if forced_action is None else forced_action                            # :281
        logp = F.log_softmax(x, 1).gather(1, a_t.unsqueeze(1)).squeeze(1)                                 # :283-284
    else:
        probs = F.softmax(x, 1)                                                                           # :286
        c = torch.distributions.Categorical(probs)
        ent = c.entropy()                                                                                 # :289
        a_t = forced_action if forced_action is not None else inverse_cdf(probs, uniform)[0]
        logp = c.log_prob(a_t)                                                                            # :291
    cpu_a_t = a_t.numpy().copy()
    pred = np.full(B, -2, np.int32)
    for i, next_id in enumerate(cpu_a_t):
        if (next_id >= V or last_step) and not ended[i]:                                                  # :299-304
            pred[i] = -1 if obj_len[i] == 0 else int(lowest_argmax(obj_logit.detach()[i:i + 1, :obj_len[i]])[0])
        if next_id >= V or next_id == ignoreid or ended[i]:                                               # :306-307
            cpu_a_t[i] = -1
    A = 0 if ob_ang is None else ob_ang.shape[-1]
    prev = np.zeros((B, A), np.float32)                                                                   # :311-314
    for i, next_id in enumerate(cpu_a_t):
        if next_id != -1 and A:
            prev[i] = np.asarray(ob_ang[i, next_id])
    pred_id = None
    if obj_id is not None:
        pred_id = np.where(pred >= 0, np.take_along_axis(np.asarray(obj_id), np.maximum(pred, 0)[:, None].astype(np.int64), 1)[:, 0], pred).astype(np.int32)
    out.update(logp=logp, ent=ent, action=a_t, env_action=cpu_a_t.astype(np.int32), prev_angle=prev, pred_obj=pred, pred_obj_id=pred_id,
               mask=(~np.asarray(ended, bool)).astype(np.float32), hist_inc=(~np.asarray(ended, bool)).astype(np.int32),      # :328-330
               ended=np.logical_or(ended, cpu_a_t == -1))                                                 # :368
    return out


def apply_pred(pred_state, step_pred):
    """the recorder's in-place pred_obj after a step: updated only where the step recorded a prediction"""
    return np.where(step_pred != -2, step_pred, pred_state).astype(np.int32)


def rollout_loss_ref(steps, train_ml, weights=None):
    """:448-451 over the per-step dicts: (loss, logs); `ref` is NOT scaled by train_ml.  `weights` [T, B]: the golden's scripted weights
    on the log-probabilities (tools/gen_reverie_policy_golden.py)."""
    B = len(steps[0]["mask"])
    il = sum(s["ml"].sum() for s in steps) * train_ml / B
    rf = sum(s["ref"].sum() for s in steps) / B
    loss = il + rf
    if weights is not None:
        loss = loss + sum((torch.as_tensor(weights[t]) * steps[t]["logp"]).sum() for t in range(len(steps)))
    return loss, {"IL_loss": float(il.detach()), "REF_loss": float(rf.detach())}


def random_case(seed, B, V, O):
    """One step's inputs for the op-level tests: ragged candidate and object counts (-inf behind them; obj_len 0 rows keep one finite
    slot, as the reference's padding to length 1 does), no exact ties in obj_logit, a random back-track mask on navigable slots,
    targets with STOP (written as V or as cand_len - 1) and ignored rows, ended rows, object ids with and without the goal."""
    g = torch.Generator().manual_seed(seed)
    act = torch.randn(B, V, generator=g) * 2.0
    n_nav = torch.randint(0, V + 1, (B,), generator=g)
    act[torch.arange(V)[None] >= n_nav[:, None]] = -float("inf")
    obj = torch.randn(B, O, generator=g) * 2.0
    for _ in range(8):                                                        # no exact ties in a row
        s = obj.sort(1)[0]
        tie = (s[:, 1:] == s[:, :-1]).any(1) if O > 1 else torch.zeros(B, dtype=torch.bool)
        if not bool(tie.any()):
            break
        obj[tie] = torch.randn(int(tie.sum()), O, generator=g) * 2.0
    obj_len = torch.randint(0, O + 1, (B,), generator=g)
    obj[torch.arange(O)[None] >= obj_len.clamp(min=1)[:, None]] = -float("inf")
    cand_len = (n_nav + 1).to(torch.int32)
    ended = torch.rand(B, generator=g) < 0.15
    target = (torch.rand(B, generator=g) * n_nav).long().clamp(max=V - 1)
    stop = torch.rand(B, generator=g)
    target = torch.where((stop < 0.15) | (n_nav == 0), torch.full_like(target, V), target)               # STOP as the reference writes it
    target = torch.where((stop >= 0.15) & (stop < 0.3), n_nav, target)                                    # ... and as nav_observe does
    target[torch.rand(B, generator=g) < 0.1] = -100
    target[ended] = -100
    bt = (torch.rand(B, V, generator=g) < 0.2) & (torch.arange(V)[None] < n_nav[:, None])
    valid = (target >= 0) & (target < V)
    bt[torch.arange(B)[valid], target[valid]] = False                                                     # (the teacher's slot stays: a finite loss)
    obj_id = torch.stack([torch.randperm(4 * O, generator=g)[:O] for _ in range(B)]).to(torch.int32) + 100
    pick = torch.randint(0, O, (B,), generator=g)
    goal = obj_id[torch.arange(B), pick].clone()                                                          # in view only if pick < obj_len
    goal[torch.rand(B, generator=g) < 0.2] = 7                                                            # ... or nowhere
    ob_ang = torch.randn(B, V, 4, generator=g)
    w = torch.randn(4, B, generator=g)
    u = torch.rand(B, generator=g)
    return dict(act=act, obj=obj, obj_len=obj_len.to(torch.int32), cand_len=cand_len, ended=ended, target=target, bt=bt, obj_id=obj_id,
                goal=goal.to(torch.int32), ob_ang=ob_ang, w=w, u=u)


# the op-level GPU cases: (B, V, O).  1027 rows are no multiple of the 4 rows of a workgroup; V = 63 puts the STOP column into lane 63,
# V = 64 into the next register column, V = 255 is the cap (V + 1 = 256); O = 1, 65 (a second register column), 256 (the cap).
OP_SHAPES = [(1027, 37, 7), (1027, 63, 7), (1027, 64, 7), (1027, 255, 7), (1027, 37, 1), (1027, 37, 65), (1027, 37, 256)]
OP_SEED = 32                                     # (tests/test_reverie_policy.py checks the exclusion cap of the sample cases for it)


def sample_margin(case, stop_logit):
    """the distance of every row's uniform to the nearest boundary of its CDF (fp64), for the exclusion cap of the sample cases"""
    o = reverie_step_ref(case["act"], case["obj"], case["obj_len"].numpy(), case["cand_len"].numpy(), case["ended"].numpy(), "teacher",
                         stop_logit=stop_logit, target=case["target"])
    x = torch.cat([case["act"], o["stop_col"][:, None]], 1)
    x = x.masked_fill(torch.cat([case["bt"], torch.zeros(len(x), 1, dtype=torch.bool)], 1), -float("inf"))
    return inverse_cdf(torch.softmax(x, 1), case["u"])[1]
