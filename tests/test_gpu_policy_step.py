"""-m gpu: the fused per-step action choice and losses of the finetune agents (csrc/policy.hip -> ops.policy_step -> agent.RolloutRecorder)
against the reference's own statements (tests/golden/policy_step.npz), the torch restatement (tests/_policy_ref.py) and the oracle.

Bounds: integer outputs and the positions of zero gradient exact; fp32 outputs and gradients 1e-5 of max(1, |ref|_max) -- what
ops.a2c_loss is held to against its restatement (tests/test_gpu_ops.py)."""
import math
import types

import numpy as np
import pytest
import torch

from _policy_ref import CASES, critic_state_dict, golden_hidden, inverse_cdf, policy_step_ref, rollout_loss_ref, critic_ref, uniform_case
from _util import load_npz, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"fp32": 1e-3, "bf16": 1e-2}            # tests/test_gpu_model.py


def close(a, b, tol, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    print(f"[{what}] max|d| {err:.3e} (scale {scale:.3e})")
    assert err <= tol * scale, f"{what}: max|d|={err:.3e} scale={scale:.3e} tol={tol}"


def _critic(store, prec="fp32", dropout=0.5):
    from vln_hamt_amd.models.model_HAMT import Critic
    critic = Critic(types.SimpleNamespace(dropout=dropout, hamt_precision=prec))
    critic.load_state_dict(critic_state_dict(store), strict=True)
    return critic.to(DEV)


def _poisoned_empty(real_empty):
    """torch.empty whose result is filled with NaN (floating point) or 0xFF bytes: every scratch and output buffer of the ops"""
    def empty(*a, **k):
        t = real_empty(*a, **k)
        if t.numel() and t.device.type == "cuda":
            if t.dtype.is_floating_point:
                t.fill_(float("nan"))
            else:
                t.view(torch.uint8).fill_(0xFF)
        return t
    return empty


def _golden_rollout(store, tag, check=True):
    """the golden's scripted rollout through RolloutRecorder; returns every result as host tensors"""
    from vln_hamt_amd.agent import RolloutRecorder
    feedback, normalize = CASES[tag]
    g = lambda k: store[f"{tag}/{k}"]
    T, B = store["in/cand_len"].shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    logits = d(store["in/logits"]).requires_grad_(True)
    rec = RolloutRecorder(T, B, DEV, ignoreid=int(store["meta/ignoreid"]))
    for buf in (rec.ml, rec.logp, rec.ent, rec.mask, rec.reward):
        buf.fill_(float("nan"))
    rec.env_host.fill_(-7)
    rec.reset(B)
    res = {}
    for t in range(T):
        a_t, env, prev = rec.step(t, logits[t], target=d(g("target")[t]), cand_lens=d(store["in/cand_len"][t]), bt_mask=d(g("bt_mask")[t]),
                                  ob_ang_feats=d(store["in/ob_ang"][t]), feedback=feedback,
                                  forced_action=d(g("a_t")[t]) if feedback == "sample" else None)
        res[f"a_t{t}"], res[f"env{t}"], res[f"prev{t}"] = a_t.cpu(), torch.from_numpy(env.copy()), prev.cpu()
        res[f"ended{t}"], res[f"hist_len{t}"] = rec.ended.cpu(), rec.hist_len.cpu()
        res[f"mask{t}"], res[f"ml{t}"], res[f"logp{t}"] = rec.mask[t].cpu(), rec.ml[t].detach().cpu(), rec.logp[t].detach().cpu()
        if feedback == "sample":
            res[f"ent{t}"] = rec.ent[t].detach().cpu()
        if check:
            assert a_t.dtype == torch.int64 and env.dtype == np.int32
            assert np.array_equal(res[f"a_t{t}"].numpy(), g("a_t")[t]), (t, res[f"a_t{t}"], g("a_t")[t])
            assert np.array_equal(env, g("env_action")[t]), (t, env, g("env_action")[t])
            assert np.array_equal(res[f"ended{t}"].numpy().astype(bool), g("ended")[t]) and np.array_equal(res[f"hist_len{t}"].numpy(), g("hist_len")[t])
            assert np.array_equal(res[f"mask{t}"].numpy(), g("mask")[t])
            assert np.array_equal(res[f"prev{t}"].numpy(), g("prev_angle")[t])                    # (a copy: exact)
            close(res[f"ml{t}"].sum(), torch.tensor(float(g("ml_sum")[t])), 1e-5, f"{tag} ml step {t}")
            close(res[f"logp{t}"], g("logp")[t], 1e-5, f"{tag} logp step {t}")
            if feedback == "sample":
                close(res[f"ent{t}"], g("ent")[t], 1e-5, f"{tag} entropy step {t}")
    rec.set_rewards(store["in/rewards"] * g("mask"))                                               # (:419: an ended episode's reward is 0)
    hid, last_h = golden_hidden(store)
    hidden = d(hid).requires_grad_(True)
    critic = _critic(store).eval()
    loss, logs = rec.loss(critic, hidden, d(last_h), train_ml=float(g("train_ml")), normalize=normalize)
    if feedback == "argmax":                                                                       # (the golden's scripted weights on log pi: see its generator)
        loss = loss + (d(store["in/weights"]) * rec.stacked("logp")).sum()
    loss.backward()
    res.update(loss=loss.detach().cpu(), d_logit=logits.grad.cpu(), **{"log_" + k: v.cpu() for k, v in logs.items()})
    if feedback == "sample":
        res["d_hidden"] = hidden.grad.cpu()
        res.update({"d_critic/" + k: p.grad.cpu() for k, p in critic.named_parameters()})
    return res


@pytest.mark.parametrize("tag", sorted(CASES))
def test_recorder_vs_reference_goldens(tag):
    """RolloutRecorder (ops.policy_step per step, ops.a2c_loss at the end, a real Critic) on the golden's scripted rollout: every per-step
    output, the final loss with its logged sums and d loss / d logit per step against the reference's own statements."""
    store = load_npz("policy_step.npz")
    feedback, _ = CASES[tag]
    g = lambda k: store[f"{tag}/{k}"]
    res = _golden_rollout(store, tag)
    close(res["loss"], torch.tensor(float(g("loss"))), 1e-5, f"{tag} loss")
    close(res["log_IL_loss"], torch.tensor(float(g("IL_loss"))), 1e-5, f"{tag} IL_loss")
    ref = g("d_logit")
    got = res["d_logit"].numpy()
    assert np.array_equal(got == 0, ref == 0), np.argwhere((got == 0) != (ref == 0))
    close(got, ref, 1e-5, f"{tag} d_logit")
    if feedback == "sample":
        close(res["log_RL_loss"], torch.tensor(float(g("RL_loss"))), 1e-5, f"{tag} RL_loss")
        assert float(res["log_total"]) == float(g("total"))
        close(res["log_policy"], torch.tensor(float(g("policy_sum"))), 1e-4, f"{tag} policy sum")
        close(res["log_critic"], torch.tensor(float(g("critic_sum"))), 1e-4, f"{tag} critic sum")
        close(res["log_entropy"], torch.tensor(float(g("entropy_sum"))), 1e-5, f"{tag} entropy sum")
        close(sum(res[f"ent{t}"].double().sum() for t in range(store["in/cand_len"].shape[0])), torch.tensor(float(g("entropy_logged"))), 1e-5, f"{tag} logged entropy")
        close(res["d_hidden"].double().flatten(1).norm(dim=1), g("d_hidden_norm"), 1e-4, f"{tag} |d hidden| per step")
        for k, v in sub(store, f"{tag}/d_critic_norm/").items():
            assert abs(float(res["d_critic/" + k].double().norm()) - float(v)) <= 1e-4 * max(1.0, float(v)), k


@pytest.mark.parametrize("tag", ["sample_total", "argmax", "teacher"])
def test_poisoned_buffers_change_nothing(tag, monkeypatch):
    """Every scratch and output buffer pre-filled with NaN / 0xFF (the recorder's arrays by _golden_rollout, every torch.empty of the ops
    here): bit-identical step outputs, losses and d loss / d logit (the gradients behind the Critic's GEMMs to 1e-6)."""
    store = load_npz("policy_step.npz")
    want = _golden_rollout(store, tag, check=False)
    monkeypatch.setattr(torch, "empty", _poisoned_empty(torch.empty))
    got = _golden_rollout(store, tag, check=False)
    monkeypatch.undo()
    assert set(want) == set(got)
    for k, w in want.items():
        assert not bool(torch.isnan(got[k].double()).any()), k
        if k == "d_hidden" or k.startswith("d_critic/"):           # (the Critic's weight-gradient GEMMs: summation order is not pinned run to run)
            close(got[k], w, 1e-6, f"poisoned {tag} {k}")
        else:
            assert torch.equal(w, got[k]), k


def _ops_step(logit, cand_len, mode, ended=None, **kw):
    from vln_hamt_amd import ops
    B = logit.shape[0]
    ended = torch.zeros(B, dtype=torch.uint8, device=DEV) if ended is None else ended
    mask = torch.empty(B, dtype=torch.float32, device=DEV)
    return ops.policy_step(logit, cand_len, ended, mask, mode=mode, **kw), ended, mask


@pytest.mark.parametrize("mode", ["teacher", "argmax", "sample"])
def test_policy_step_vs_restatement(mode):
    """ops.policy_step on 8192 rows of V = 37 (ragged -inf tails, a random back-track mask that never takes a whole row, targets with
    ignored rows, some episodes ended) against the torch restatement: outputs, and the gradient of a randomly weighted sum of
    ml, logp and ent.  In `sample` the injected uniforms choose: the action must equal the restatement's inverse CDF (rows whose u
    lies within 1e-6 of a CDF boundary excluded, at most 1 in 1000: tests/test_policy_step.py checks the seed)."""
    logit_c, u = uniform_case()
    B, V = logit_c.shape
    g = torch.Generator().manual_seed(5)
    n = torch.isfinite(logit_c).sum(1)
    cand_len = n.to(torch.int32)
    target = (torch.rand(B, generator=g) * n).long().clamp(max=V - 1)
    target[torch.rand(B, generator=g) < 0.1] = -100
    bt = (torch.rand(B, V, generator=g) < 0.2) & (torch.arange(V)[None] < (n - 1)[:, None])          # never the STOP slot
    ended = torch.rand(B, generator=g) < 0.15
    ob_ang = torch.randn(B, V, 4, generator=g)
    w = torch.randn(3, B, generator=g)
    x_ref = logit_c.clone().requires_grad_(True)
    o = policy_step_ref(x_ref, cand_len.numpy(), ended.numpy(), mode, target=target, bt_mask=bt, ob_ang=ob_ang.numpy(), uniform=u)
    x = logit_c.to(DEV).requires_grad_(True)
    hist_len = torch.full((B,), 3, dtype=torch.int32, device=DEV)
    (ml, logp, ent, a_t, env, prev), ended_d, mask = _ops_step(
        x, cand_len.to(DEV), mode, ended=ended.to(torch.uint8).to(DEV), target=target.to(DEV), bt_mask=bt.to(torch.uint8).to(DEV),
        ob_ang=ob_ang.to(DEV), hist_len=hist_len, uniform=u.to(DEV) if mode == "sample" else None)
    keep = torch.ones(B, dtype=torch.bool)
    if mode == "sample":
        probs = torch.softmax(logit_c.masked_fill(bt, -float("inf")), 1)
        keep = inverse_cdf(probs, u)[1] >= 1e-6
        assert int((~keep).sum()) * 1000 <= B, int((~keep).sum())
    assert torch.equal(a_t.cpu()[keep], o["action"][keep])
    assert bool(((a_t.cpu() == o["action"]) | ~keep).all())
    same = (a_t.cpu() == o["action"]).numpy()                      # (an excluded row that chose the neighbour: compared no further)
    assert np.array_equal(env.cpu().numpy()[same], o["env_action"][same]) and np.array_equal(prev.cpu().numpy()[same], o["prev_angle"][same])
    assert np.array_equal(ended_d.cpu().numpy().astype(bool)[same], o["ended"][same]) and np.array_equal(mask.cpu().numpy(), o["mask"])
    assert np.array_equal(hist_len.cpu().numpy(), 3 + o["hist_inc"])
    close(ml, o["ml"], 1e-5, f"{mode} ml")
    st = torch.from_numpy(same)
    close(logp.detach().cpu()[st], o["logp"].detach()[st], 1e-5, f"{mode} logp")
    if mode == "sample":
        close(ent, o["ent"], 1e-5, f"{mode} entropy")
    else:
        assert ent is None
    if not bool(st.all()):                                         # the gradient of log pi(a) depends on a: redo the restatement on the kernel's actions
        x_ref = logit_c.clone().requires_grad_(True)
        o = policy_step_ref(x_ref, cand_len.numpy(), ended.numpy(), mode, target=target, bt_mask=bt, ob_ang=ob_ang.numpy(), forced_action=a_t.cpu())
    loss_ref = (w[0] * o["ml"]).sum() + (w[1] * o["logp"]).sum() + ((w[2] * o["ent"]).sum() if mode == "sample" else 0.0)
    loss_ref.backward()
    wd = w.to(DEV)
    loss = (wd[0] * ml).sum() + (wd[1] * logp).sum() + ((wd[2] * ent).sum() if mode == "sample" else 0.0)
    loss.backward()
    got, ref = x.grad.cpu(), x_ref.grad
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got == 0, ref == 0), int(((got == 0) != (ref == 0)).sum())
    close(got, ref, 1e-5, f"{mode} d_logit")


def test_wide_rows_and_strided_logits():
    """V = 256 (four columns per lane) on a row-strided view, argmax: action, log-probability and gradient against the restatement."""
    g = torch.Generator().manual_seed(9)
    B, V = 33, 256
    full = torch.randn(B, V + 24, generator=g) * 3
    full[:, 200:V] = -float("inf")
    x_ref = full[:, :V].clone().requires_grad_(True)
    cand_len = torch.full((B,), 200, dtype=torch.int32)
    target = torch.randint(0, 200, (B,), generator=g)
    o = policy_step_ref(x_ref, cand_len.numpy(), np.zeros(B, bool), "argmax", target=target)
    (o["ml"].sum() + 2 * o["logp"].sum()).backward()
    base = full.to(DEV).requires_grad_(True)
    (ml, logp, ent, a_t, env, prev), _, _ = _ops_step(base[:, :V], cand_len.to(DEV), "argmax", target=target.to(DEV))
    (ml.sum() + 2 * logp.sum()).backward()
    assert torch.equal(a_t.cpu(), o["action"]) and np.array_equal(env.cpu().numpy(), o["env_action"]) and prev.shape == (B, 0)
    close(ml, o["ml"], 1e-5, "wide ml")
    close(logp, o["logp"], 1e-5, "wide logp")
    close(base.grad[:, :V], x_ref.grad, 1e-5, "wide d_logit")
    assert float(base.grad[:, V:].abs().max()) == 0.0


def test_fully_masked_row_gives_stop_and_zero_gradients():
    """A row whose every slot is masked cannot occur on the path; the launcher documents env_action -1 and zero gradients, no NaN."""
    x = torch.randn(4, 9, device=DEV, requires_grad=True)
    bt = torch.zeros(4, 9, dtype=torch.uint8, device=DEV)
    bt[1] = 1
    cl = torch.full((4,), 9, dtype=torch.int32, device=DEV)
    for mode in ("argmax", "sample"):
        (ml, logp, ent, a_t, env, prev), ended, _ = _ops_step(x, cl, mode, bt_mask=bt, uniform=torch.full((4,), 0.5, device=DEV))
        x.grad = None
        (logp.sum() + (ent.sum() if ent is not None else 0.0)).backward()
        assert int(env[1]) == -1 and int(ended[1]) == 1 and float(x.grad[1].abs().max()) == 0.0
        assert not bool(torch.isnan(x.grad).any()) and not bool(torch.isnan(logp).any())


def test_own_draws_follow_the_distribution_and_the_rng_epoch():
    """sample without injected uniforms: 2^20 rows of one 8-way distribution in ONE launch -- every frequency within
    5 sqrt(p (1 - p) / N) of p; the same (rng, call_id) draws the same, a new epoch (hamt_rng_advance) does not."""
    from vln_hamt_amd import ops
    N, V = 1 << 20, 8
    row = torch.tensor([0.3, -1.0, 2.0, 0.0, 1.1, -2.5, 0.7, -0.2])
    p = torch.softmax(row.double(), 0)
    x = row.to(DEV)[None].expand(N, V).contiguous()
    cl = torch.full((N,), V, dtype=torch.int32, device=DEV)
    ops.manual_seed(1234, torch.device(DEV))
    draw = lambda: _ops_step(x, cl, "sample", call_id=77)[0][3]
    a1, a2 = draw(), draw()
    assert torch.equal(a1, a2)
    ops.advance_rng_epoch(DEV)
    a3 = draw()
    assert float((a1 != a3).double().mean()) > 0.5
    for a in (a1, a3):
        freq = torch.bincount(a, minlength=V).double().cpu() / N
        dev = (freq - p).abs() / torch.sqrt(p * (1 - p) / N)
        print("[own draws] frequencies", [f"{f:.5f}" for f in freq.tolist()], "sigmas", [f"{s:.2f}" for s in dev.tolist()])
        assert int(a.min()) >= 0 and int(a.max()) < V and float(dev.max()) <= 5.0, dev


def test_eager_rollouts_draw_differently_without_an_epoch_advance():
    """Two eager `sample` rollouts of one recorder, `reset()` between them and NOTHING advancing the RNG epoch: different draws (a fresh
    block of call ids per reset, as dropout calls get); `reset(fresh_draws=False)` repeats the rollout's draws exactly."""
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import RolloutRecorder
    B, V, T = 64, 37, 3
    g = torch.Generator().manual_seed(4)
    logit = (torch.randn(T, B, V, generator=g) * 2).to(DEV)
    cl = torch.full((B,), V, dtype=torch.int32, device=DEV)
    ops.manual_seed(99, torch.device(DEV))
    rec = RolloutRecorder(T, B, DEV)

    def rollout(**kw):
        rec.reset(**kw)
        return torch.stack([rec.step(t, logit[t], cand_lens=cl, feedback="sample")[0].clone() for t in range(T)])
    a1, a2 = rollout(), rollout()
    a3 = rollout(fresh_draws=False)
    for t in range(T):
        assert float((a1[t] != a2[t]).double().mean()) > 0.5, (t, a1[t], a2[t])
    assert float((a1[0] != a1[1]).double().mean()) > 0.5                 # (and the steps of one rollout differ from each other)
    assert torch.equal(a2, a3)
    other = RolloutRecorder(T, B, DEV)                                   # a second recorder never shares a block
    assert not (other.call_id <= rec.call_id + T - 1 and rec.call_id <= other.call_id + T - 1)


def _tiny_agent(prec="bf16", no_lang_ca=True, hidden=128, heads=2, train=False):
    from oracle.hamt_oracle import OracleConfig, make_state_dict, navcmt_param_shapes
    from vln_hamt_amd.modeling import HamtConfig
    from vln_hamt_amd.models.model_HAMT import VLNBertCMT
    from vln_hamt_amd.models.vilmodel_cmt import NavCMT
    ocfg = OracleConfig.tiny(hidden_size=hidden, num_attention_heads=heads, intermediate_size=256, image_feat_size=64,
                             no_lang_ca=no_lang_ca, act_pred_token="ob" if no_lang_ca else "ob_txt")
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "pred_head_dropout_prob"):
        setattr(ocfg, k, 0.0)
    sd = make_state_dict(navcmt_param_shapes(ocfg), seed=9)
    kw = dict(vars(ocfg))
    kw.pop("pretrain_tasks")
    agent = VLNBertCMT.__new__(VLNBertCMT)
    torch.nn.Module.__init__(agent)
    agent.args = types.SimpleNamespace(no_lang_ca=no_lang_ca, feat_dropout=0.0)
    agent.vln_bert = NavCMT(HamtConfig(hamt_precision=prec, **kw))
    agent.vln_bert.load_state_dict(sd, strict=True)
    agent.drop_env = torch.nn.Dropout(0.0)
    return agent.to(DEV).train(train), ocfg, sd


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("no_lang_ca", [False, True])
def test_recorder_rollout_backward_vs_oracle(prec, no_lang_ca):
    """A 3-step rollout of a tiny VLNBertCMT (hidden 768: the Critic's input width) driven through RolloutRecorder -- sample feedback with
    scripted draws (one episode stops at step 1, one at step 2), the chosen candidate's angle fed to `history`, imitation + A2C loss
    through a real Critic, ONE backward -- against the oracle's autograd over the restatement (tests/_policy_ref.py).  Built like
    tests/test_gpu_model.py::test_finetune_rollout_backward_vs_oracle, with that test's bounds."""
    from oracle.hamt_oracle import HamtOracle
    from vln_hamt_amd.agent import RolloutRecorder
    store = load_npz("tiny_finetune.npz")
    gstore = load_npz("policy_step.npz")
    tag = "nolangca" if no_lang_ca else "ca"
    agent, ocfg, sd = _tiny_agent(prec, no_lang_ca, hidden=768, heads=12, train=True)
    critic = _critic(gstore, prec, dropout=0.0).train()
    bc = {k: torch.from_numpy(v) for k, v in sub(store, f"{tag}/in/").items()}
    b = {k: v.to(DEV) for k, v in bc.items()}
    B, V, T, STOP = bc["txt_ids"].shape[0], bc["ob_nav_types"].shape[1], 3, -100
    nav = [torch.nonzero(bc["ob_nav_types"][i] == 1).flatten().tolist() for i in range(B)]
    cand_len = np.full(B, V, np.int32)                                     # panorama layout: the STOP token is the last of the 37
    forced = torch.tensor([[nav[i][0] for i in range(B)], [V - 1] + [nav[i][1] for i in range(1, B)],
                           [nav[0][2], nav[1][2], V - 1, nav[3][2]]])
    target = torch.tensor([[nav[i][1] for i in range(B)], [nav[i][1] for i in range(B)], [STOP] + [nav[i][2] for i in range(1, B)]])
    rewards = np.random.Generator(np.random.PCG64(3)).standard_normal((T, B)).astype(np.float32)
    rewards[2, 0] = 0.0                                                    # (episode 0 has ended by then)
    train_ml = 0.2

    rec = RolloutRecorder(T, B, DEV).reset(B)
    lang = agent("language", txt_ids=b["txt_ids"], txt_masks=b["txt_masks"])
    hs, states = [agent("history").expand(B, -1)], []
    vkw = dict(txt_masks=b["txt_masks"], ob_img_feats=b["ob_img_fts"], ob_ang_feats=b["ob_ang_fts"], ob_nav_types=b["ob_nav_types"], ob_masks=b["ob_masks"])
    envs = []
    for t in range(T):
        logit, h_t = agent("visual", txt_embeds=lang, hist_embeds=hs, hist_lens=rec.hist_len, return_states=True, **vkw)
        states.append(h_t)
        a_t, env, prev = rec.step(t, logit, target=target[t].to(DEV), cand_lens=cand_len, ob_ang_feats=b["ob_ang_fts"], feedback="sample",
                                  forced_action=forced[t].to(DEV))
        envs.append(env.copy())
        hs.append(agent("history", hist_img_feats=b["hist_img_fts"][:, t].contiguous(), hist_ang_feats=prev,
                        hist_pano_img_feats=b["hist_pano_img_fts"][:, t].contiguous(), hist_pano_ang_feats=b["hist_pano_ang_fts"][:, t].contiguous(), ob_step=t))
    _, last_h = agent("visual", txt_embeds=lang, hist_embeds=hs, hist_lens=rec.hist_len, return_states=True, **vkw)
    rec.set_rewards(rewards)
    loss, logs = rec.loss(critic, states, last_h, train_ml=train_ml, normalize="total")
    loss.backward()
    torch.cuda.synchronize()

    # oracle (CPU, fp32 autograd) over the restatement of the step
    osd = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in sd.items()}
    csd = {k: v.clone().requires_grad_(True) for k, v in critic_state_dict(gstore).items()}
    orc = HamtOracle(osd, ocfg, training=True)          # (every dropout probability is 0)
    olang = orc.ft_forward("language", txt_ids=bc["txt_ids"], txt_masks=bc["txt_masks"])
    ohs, ostates, steps = [orc.ft_forward("history").expand(B, -1)], [], []
    ended, hist_len = np.zeros(B, bool), np.ones(B, np.int64)

    def ovisual():
        hm = torch.arange(len(ohs))[None] < torch.from_numpy(hist_len)[:, None]
        lg, txt, hist_o, _ = orc.ft_forward("visual", txt_embeds=olang, hist_embeds=torch.stack(ohs, 1), txt_masks=bc["txt_masks"], hist_masks=hm,
                                            ob_img_feats=bc["ob_img_fts"], ob_ang_feats=bc["ob_ang_fts"], ob_nav_types=bc["ob_nav_types"], ob_masks=bc["ob_masks"])
        return lg, (hist_o[:, 0] if no_lang_ca else txt[:, 0] * hist_o[:, 0])            # model_HAMT.py:56-62

    for t in range(T):
        lg, st = ovisual()
        ostates.append(st)
        o = policy_step_ref(lg, cand_len, ended, "sample", target=target[t], ob_ang=bc["ob_ang_fts"].numpy(), forced_action=forced[t])
        assert np.array_equal(o["env_action"], envs[t]), (t, o["env_action"], envs[t])
        steps.append(o)
        ended, hist_len = o["ended"], hist_len + o["hist_inc"]
        ohs.append(orc.ft_forward("history", hist_img_feats=bc["hist_img_fts"][:, t], hist_ang_feats=torch.from_numpy(o["prev_angle"]),
                                  ob_step_ids=torch.LongTensor([t]), hist_pano_img_feats=bc["hist_pano_img_fts"][:, t],
                                  hist_pano_ang_feats=bc["hist_pano_ang_fts"][:, t]))
    _, olast = ovisual()
    oloss, ologs = rollout_loss_ref(steps, rewards, ostates, olast, critic_ref(csd), "sample", "total", train_ml)
    oloss.backward()
    assert np.array_equal(rec.ended.cpu().numpy().astype(bool), ended) and np.array_equal(rec.hist_len.cpu().numpy(), hist_len)
    e_loss = abs(float(loss) - float(oloss)) / max(1.0, abs(float(oloss)))
    ref = {k: v.grad for k, v in osd.items() if v.grad is not None}
    ref.update({"critic." + k: v.grad for k, v in csd.items()})
    got = {k: p.grad for k, p in agent.vln_bert.named_parameters() if p.grad is not None}
    got.update({"critic." + k: p.grad for k, p in critic.named_parameters()})
    gmax = max(float(v.norm()) for v in ref.values())
    num = den = dot = worst = 0.0
    for k, r in ref.items():
        if float(r.norm()) == 0.0 and k not in got:
            continue
        g_ = got[k].detach().cpu().double()
        r = r.double()
        worst = max(worst, abs(float(g_.norm()) - float(r.norm())) / max(float(r.norm()), 5e-2 * gmax))
        dot += float((g_ * r).sum()); num += float((g_ * g_).sum()); den += float((r * r).sum())
    cos = dot / math.sqrt(num * den)
    print(f"[recorder rollout bwd {tag} {prec}] loss {float(loss):.5f} vs {float(oloss):.5f} (rel {e_loss:.2e}); IL {float(logs['IL_loss']):.5f} vs "
          f"{ologs['IL_loss']:.5f}; RL {float(logs['RL_loss']):.5f} vs {ologs['RL_loss']:.5f}; global grad cosine {cos:.6f}; worst per-parameter norm error {worst:.2e}")
    assert e_loss <= TOL[prec], e_loss
    assert cos >= (0.99999 if prec == "fp32" else 0.995), cos
    assert worst <= (2e-3 if prec == "fp32" else 6e-2), worst


@pytest.mark.parametrize("mode", ["argmax", "sample"])
def test_captured_step_matches_eager(mode):
    """graph.GraphedInference over `visual -> RolloutRecorder.step(sync=False) -> history` with the chosen angle fed straight in: argmax
    bit-identical to the eager step; sample: two replays (two RNG epochs) differ, and each equals the eager step under its epoch.  The
    recorder's in-place state (`ended`, `hist_len`) moves exactly once per call, the capturing one included."""
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import RolloutRecorder
    from vln_hamt_amd.graph import GraphedInference
    store = load_npz("tiny_finetune.npz")
    agent, _, _ = _tiny_agent("bf16", True)
    b = {k: torch.from_numpy(v).to(DEV) for k, v in sub(store, "nolangca/in/").items()}
    B, V = b["ob_nav_types"].shape
    cl = torch.full((B,), V, dtype=torch.int32, device=DEV)
    sid = torch.zeros(1, dtype=torch.long, device=DEV)
    recs = {"graph": RolloutRecorder(4, B, DEV), "eager": RolloutRecorder(4, B, DEV)}
    recs["eager"].call_id = recs["graph"].call_id                        # the same counter stream for both
    with torch.no_grad():
        lang = agent("language", txt_ids=b["txt_ids"], txt_masks=b["txt_masks"])
        cls_h = agent("history").expand(B, -1).contiguous()[:, None].contiguous()

        def make(rec):
            def fn(hist, oi, oa, himg, pimg, pang):
                hm = torch.arange(hist.shape[1], device=DEV)[None] < rec.hist_len[:, None]
                logit = agent.vln_bert("visual", txt_embeds=lang, txt_masks=b["txt_masks"], hist_embeds=hist, hist_masks=hm, ob_img_feats=oi,
                                       ob_ang_feats=oa, ob_nav_types=b["ob_nav_types"], ob_masks=b["ob_masks"])[0]
                a_t, env, prev = rec.step(0, logit, cand_lens=cl, ob_ang_feats=oa, feedback=mode, sync=False)
                h = agent.vln_bert("history", hist_img_feats=himg, hist_ang_feats=prev, ob_step_ids=sid, hist_pano_img_feats=pimg, hist_pano_ang_feats=pang)
                return a_t, env, prev, h, rec.logp[0], logit
            return fn

        args = (cls_h, b["ob_img_fts"], b["ob_ang_fts"], b["hist_img_fts"][:, 0].contiguous(), b["hist_pano_img_fts"][:, 0].contiguous(),
                b["hist_pano_ang_fts"][:, 0].contiguous())
        gi = GraphedInference(make(recs["graph"]), state=(recs["graph"].ended, recs["graph"].hist_len))
        eager = make(recs["eager"])
        outs = {"graph": [], "eager": []}
        for name, call in (("graph", lambda: gi("step0", *args)), ("eager", lambda: eager(*args))):
            ops.manual_seed(7, torch.device(DEV))
            for epoch in range(3):
                recs[name].reset(fresh_draws=False)       # (the graph holds the call id it was captured with)
                out = [t.clone() for t in call()]
                assert int(recs[name].hist_len.min()) == 2 and int(recs[name].hist_len.max()) == 2, (name, epoch, recs[name].hist_len)
                outs[name].append(out + [recs[name].ended.clone()])
                ops.advance_rng_epoch(DEV)
    for epoch in range(3):
        for w, g_ in zip(outs["eager"][epoch], outs["graph"][epoch]):
            fin = torch.isfinite(w.float())
            assert torch.equal(torch.isfinite(g_.float()), fin) and torch.equal(w[fin], g_[fin]), (mode, epoch)
    acts = [o[0] for o in outs["graph"]]
    if mode == "sample":
        assert not torch.equal(acts[0], acts[1]) and not torch.equal(acts[1], acts[2]) and not torch.equal(acts[0], acts[2]), acts
    else:
        assert torch.equal(acts[0], acts[1])


def test_env_action_is_the_only_transfer_to_the_host():
    """RolloutRecorder.step under torch.cuda.set_sync_debug_mode('error'): nothing in it synchronises the host with the device except the
    declared copy of the int32 environment actions into the pinned buffer (non-blocking, then ONE event wait, which the debug mode does
    not police); the values arrive."""
    from vln_hamt_amd.agent import RolloutRecorder
    B, V = 8, 37
    g = torch.Generator().manual_seed(2)
    logit = torch.randn(B, V, generator=g).to(DEV).requires_grad_(True)
    cl = torch.full((B,), V, dtype=torch.int32, device=DEV)
    ang = torch.randn(B, V, 4, generator=g).to(DEV)
    target = torch.randint(0, V - 1, (B,), generator=g).to(DEV)
    forced = torch.tensor([3, V - 1, 0, 7, -100, 5, 36, 1]).to(DEV)
    rec = RolloutRecorder(3, B, DEV).reset(B)
    assert rec.env_host.is_pinned() and rec.env_host.dtype == torch.int32
    rec.step(0, logit, target=target, cand_lens=cl, ob_ang_feats=ang, feedback="sample")          # (first use: library load, allocator)
    rec.reset()
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a_t, env, prev = rec.step(0, logit, target=target, cand_lens=cl, ob_ang_feats=ang, feedback="sample", forced_action=forced)
        a2, env_dev, _ = rec.step(1, logit, target=target, cand_lens=cl, ob_ang_feats=ang, feedback="argmax", sync=False)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert isinstance(env, np.ndarray) and env.tolist() == [3, -1, 0, 7, -1, 5, -1, 1]
    assert torch.is_tensor(env_dev) and env_dev.is_cuda and env_dev.dtype == torch.int32
    exp_end = np.array([0, 1, 0, 0, 1, 0, 1, 0], bool)
    got_end = rec.ended.cpu().numpy().astype(bool)
    assert np.array_equal(got_end[exp_end], exp_end[exp_end])                                      # (step 1 may have ended more)
    assert (env_dev.cpu().numpy()[exp_end] == -1).all()
