"""A small torch restatement of one rollout step of the finetune agents (finetune_src/r2r/agent_cmt.py:336-401) and of the rollout's
loss (:453-522), for the tests of ops.policy_step / agent.RolloutRecorder.  Test infrastructure: pinned against the reference's own
statements by tests/golden/policy_step.npz (tools/gen_policy_step_golden.py)."""
import numpy as np
import torch
import torch.nn.functional as F


def inverse_cdf(probs, u):
    """The first index whose inclusive cumulative probability exceeds u (fp64), never behind the last slot of non-zero probability.
    Returns (index [B] int64, margin [B]: the distance of u to the nearest CDF boundary)."""
    p = probs.detach().double()
    cdf = p.cumsum(1)
    u = torch.as_tensor(u, dtype=torch.float64).reshape(-1, 1)
    last = (p > 0).double().mul(torch.arange(p.shape[1], dtype=torch.float64)[None]).argmax(1)
    a = torch.minimum((cdf <= u).sum(1), last)
    return a, (cdf - u).abs().min(1)[0]


def policy_step_ref(logit, cand_len, ended, mode, target=None, bt_mask=None, ob_ang=None, forced_action=None, uniform=None, ignoreid=-100):
    """logit [B, V] (may require grad), cand_len / ended numpy [B]; returns a dict of the step's values (ml per row)."""
    B, V = logit.shape
    out = {}
    if target is not None:
        out["ml"] = F.cross_entropy(logit, target, ignore_index=ignoreid, reduction="none")                  # :339
    else:
        out["ml"] = torch.zeros(B)
    x = logit if bt_mask is None else logit.masked_fill(torch.as_tensor(bt_mask).bool(), -float("inf"))      # :350
    ent = None
    if mode == "teacher":
        a_t = target if forced_action is None else forced_action                                              # :354
        logp = torch.zeros(B)
    elif mode == "argmax":
        a_t = x.max(1)[1].detach() if forced_action is None else forced_action                                # :356
        logp = F.log_softmax(x, 1).gather(1, a_t.unsqueeze(1)).squeeze(1)                                     # :358-359
    else:
        probs = F.softmax(x, 1)                                                                               # :361
        c = torch.distributions.Categorical(probs)
        ent = c.entropy()                                                                                     # :364
        a_t = forced_action if forced_action is not None else inverse_cdf(probs, uniform)[0]
        logp = c.log_prob(a_t)                                                                                # :366
    cpu_a_t = a_t.numpy().copy()
    for i, next_id in enumerate(cpu_a_t):                                                                     # :372-375
        if next_id == (cand_len[i] - 1) or next_id == ignoreid or ended[i]:
            cpu_a_t[i] = -1
    A = 0 if ob_ang is None else ob_ang.shape[-1]
    prev = np.zeros((B, A), np.float32)                                                                       # :382-385
    for i, next_id in enumerate(cpu_a_t):
        if next_id != -1 and A:
            prev[i] = np.asarray(ob_ang[i, next_id])
    out.update(logp=logp, ent=ent, action=a_t, env_action=cpu_a_t.astype(np.int32), prev_angle=prev,
               mask=(~np.asarray(ended, bool)).astype(np.float32),                                            # :418-420
               hist_inc=(~np.asarray(ended, bool)).astype(np.int32),                                          # :399-401
               ended=np.logical_or(ended, cpu_a_t == -1))                                                     # :447
    return out


CASES = {"sample_total": ("sample", "total"), "sample_batch": ("sample", "batch"), "sample_none": ("sample", "none"),
         "teacher": ("teacher", "total"), "argmax": ("argmax", "total")}


def golden_hidden(store):
    """the critic's inputs of tests/golden/policy_step.npz, rebuilt from the stored seed (tools/gen_policy_step_golden.py::hidden_states)"""
    T, B = store["in/cand_len"].shape
    rng = np.random.Generator(np.random.PCG64(int(store["meta/hidden_seed"])))
    return rng.standard_normal((T, B, 768), dtype=np.float32) * 0.5, rng.standard_normal((B, 768), dtype=np.float32) * 0.5


def critic_state_dict(store):
    from oracle.hamt_oracle import make_state_dict
    return make_state_dict({"state2value.0.weight": (512, 768), "state2value.0.bias": (512,), "state2value.3.weight": (1, 512),
                            "state2value.3.bias": (1,)}, seed=int(store["meta/critic_seed"]))


def critic_ref(sd):
    """the Critic in eval mode (finetune_src/models/model_HAMT.py:258-269): Linear 768 -> 512, ReLU, (Dropout), Linear 512 -> 1, squeeze"""
    return lambda s: F.linear(F.relu(F.linear(s, sd["state2value.0.weight"], sd["state2value.0.bias"])),
                              sd["state2value.3.weight"], sd["state2value.3.bias"]).squeeze()


def rollout_loss_ref(steps, rewards, hidden, last_h, critic, feedback, normalize, train_ml, weights=None, gamma=0.9, entropy_weight=0.01):
    """agent_cmt.py:453-522 over the per-step dicts of policy_step_ref: (loss, logs).  `weights` [T, B]: the golden's scripted weights on
    the argmax log-probabilities (tools/gen_policy_step_golden.py)."""
    from oracle.hamt_oracle import a2c_loss_ref
    T, B = len(steps), len(steps[0]["mask"])
    loss, logs = 0.0, {}
    if feedback == "sample":
        masks = [s["mask"] for s in steps]
        rl, lg = a2c_loss_ref([s["logp"] for s in steps], [critic(hidden[t]) for t in range(T)], [np.asarray(rewards[t], np.float32) * masks[t] for t in range(T)],
                              masks, critic(last_h).detach(), steps[-1]["ended"], [s["ent"] for s in steps], gamma=gamma,
                              entropy_loss_weight=entropy_weight, normalize_loss=normalize)
        loss = loss + rl
        logs.update(RL_loss=float(rl), policy=sum(lg["policy_loss"]), critic=sum(lg["critic_loss"]), total=float(np.sum(masks)),
                    entropy=sum(float((-entropy_weight * s["ent"].detach() * torch.from_numpy(s["mask"])).sum()) for s in steps))    # :501
    if train_ml is not None:
        il = sum(s["ml"].sum() for s in steps) * train_ml / B
        loss = loss + il
        logs["IL_loss"] = float(il)
    if weights is not None:
        loss = loss + sum((torch.as_tensor(weights[t]) * steps[t]["logp"]).sum() for t in range(T))
    return loss, logs


def uniform_case(seed=11, B=8192, V=37):
    """logits [B, V] with ragged -inf tails and injected uniforms [B] for the inverse-CDF test"""
    g = torch.Generator().manual_seed(seed)
    logit = torch.randn(B, V, generator=g) * 2.0
    n = torch.randint(2, V + 1, (B,), generator=g)
    logit[torch.arange(V)[None] >= n[:, None]] = -float("inf")
    return logit, torch.rand(B, generator=g)
