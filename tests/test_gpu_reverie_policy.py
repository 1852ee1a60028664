"""-m gpu: REVERIE's rollout step (csrc/policy.hip -> ops.policy_ref_step -> agent.ReverieRolloutRecorder) against the reference's own
statements (tests/golden/reverie_policy.npz) and the torch restatement (tests/_reverie_policy_ref.py).

Bounds, tests/test_gpu_policy_step.py's: integer outputs exact; fp32 outputs and gradients 1e-5 of max(1, |ref|_max); positions of zero
gradient exact.  With stop_logit='index' column V holds an integer up to O - 1, so with O = 65 / 256 a softmax term can fall below the
smallest normal fp32 (1.18e-38), where an exp may or may not flush to 0 on either side: there `zeros_agree` holds the structural zeros
(masked and -inf positions) to exactly 0 and lets a position be 0 on one side only where the other side is below FLT_MIN."""
import numpy as np
import pytest
import torch

from _policy_ref import golden_hidden, inverse_cdf
from _reverie_policy_ref import MODES, OP_SEED, OP_SHAPES, apply_pred, random_case, reverie_step_ref
from _util import load_npz
from test_gpu_policy_step import _critic, _poisoned_empty, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLT_MIN = float(np.finfo(np.float32).tiny)
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def zeros_agree(got, ref, structural, what):
    got, ref = torch.as_tensor(got).cpu(), torch.as_tensor(ref).cpu()
    assert not bool(torch.isnan(got).any()), what
    assert float(got[structural].abs().max() if bool(structural.any()) else 0.0) == 0.0, what
    flip = (got == 0) != (ref == 0)
    print(f"[{what}] zero positions differing (all below FLT_MIN on the other side): {int(flip.sum())}")
    assert float(torch.where(flip, torch.maximum(got.abs(), ref.abs()), torch.zeros_like(ref)).max()) < FLT_MIN, what


def _golden_rollout(store, tag, check=True):
    """the golden's scripted rollout through ReverieRolloutRecorder (object targets looked up from the ids); every result on the host"""
    from vln_hamt_amd.agent import ReverieRolloutRecorder
    g = lambda k: store[f"{tag}/{k}"]
    T, B = store["in/cand_len"].shape
    act = d(store["in/act_logits"]).requires_grad_(True)
    obj = d(store["in/obj_logits"]).requires_grad_(True)
    rec = ReverieRolloutRecorder(T, B, DEV, ignoreid=int(store["meta/ignoreid"]))
    for buf in (rec.ml, rec.ref, rec.logp, rec.ent, rec.mask, rec.reward):
        buf.fill_(float("nan"))
    rec.env_host.fill_(-7)
    rec.reset(B)
    res = {}
    for t in range(T):
        a_t, env, prev = rec.step(t, act[t], obj[t], d(store["in/obj_len"][t]), target=d(g("target")[t]), cand_lens=d(store["in/cand_len"][t]),
                                  bt_mask=d(g("bt_mask")[t]), ob_ang_feats=d(store["in/ob_ang"][t]), feedback=tag, obj_ids=d(store["in/obj_ids"][t]),
                                  goal_obj=d(store["in/goal_obj"]), forced_action=d(g("a_t")[t]) if tag == "sample" else None)
        res[f"a_t{t}"], res[f"env{t}"], res[f"prev{t}"] = a_t.cpu(), torch.from_numpy(env.copy()), prev.cpu()
        res[f"ended{t}"], res[f"hist_len{t}"], res[f"pred_id{t}"] = rec.ended.cpu(), rec.hist_len.cpu(), rec.pred_obj_id.cpu()
        res[f"mask{t}"] = rec.mask[t].cpu()
        for k in ("ml", "ref", "logp") + (("ent",) if tag == "sample" else ()):
            res[f"{k}{t}"] = getattr(rec, k)[t].detach().cpu()
        if check:
            assert np.array_equal(res[f"a_t{t}"].numpy(), g("a_t")[t]) and np.array_equal(env, g("env_action")[t]), (t, a_t, env)
            assert np.array_equal(res[f"ended{t}"].numpy().astype(bool), g("ended")[t]) and np.array_equal(res[f"hist_len{t}"].numpy(), g("hist_len")[t])
            assert np.array_equal(res[f"mask{t}"].numpy(), g("mask")[t]) and np.array_equal(res[f"prev{t}"].numpy(), g("prev_angle")[t])
            assert np.array_equal(res[f"pred_id{t}"].numpy(), g("pred_obj_id")[t]), (t, res[f"pred_id{t}"], g("pred_obj_id")[t])
            close(res[f"ml{t}"].sum(), torch.tensor(float(g("ml_sum")[t])), 1e-5, f"{tag} ml step {t}")
            close(res[f"ref{t}"].sum(), torch.tensor(float(g("ref_sum")[t])), 1e-5, f"{tag} ref step {t}")
            close(res[f"logp{t}"], g("logp")[t], 1e-5, f"{tag} logp step {t}")
            if tag == "sample":
                close(res[f"ent{t}"], g("ent")[t], 1e-5, f"{tag} entropy step {t}")
    slots, ids = rec.predicted_objects()
    res["pred_slot"], res["pred_id"] = torch.from_numpy(slots.copy()), torch.from_numpy(ids.copy())
    rec.set_rewards(store["in/rewards"] * g("mask"))
    hid, last_h = golden_hidden(store)
    critic = _critic(store).eval()
    loss, logs = rec.loss(critic, d(hid), d(last_h), train_ml=float(g("train_ml")), normalize="total")
    if tag == "argmax":
        loss = loss + (d(store["in/weights"]) * rec.stacked("logp")).sum()
    loss.backward()
    res.update(loss=loss.detach().cpu(), d_act=act.grad.cpu(), d_obj=obj.grad.cpu(), **{"log_" + k: v.cpu() for k, v in logs.items()})
    return res


@pytest.mark.parametrize("tag", MODES)
def test_recorder_vs_reference_goldens(tag):
    """ReverieRolloutRecorder on the golden's scripted rollout (a real Critic and ops.a2c_loss for `sample`): every per-step output, the
    predicted objects, the loss with IL_loss / REF_loss (/ RL_loss) and both logit gradients against the reference's own statements."""
    store = load_npz("reverie_policy.npz")
    g = lambda k: store[f"{tag}/{k}"]
    res = _golden_rollout(store, tag)
    assert np.array_equal(res["pred_id"].numpy(), g("pred_obj_id")[-1])
    ids = store["in/obj_ids"]
    for b, (slot, oid) in enumerate(zip(res["pred_slot"].tolist(), res["pred_id"].tolist())):
        assert (slot == -1) == (oid == -1) and (slot == -1 or oid in ids[:, b, slot]), (b, slot, oid)
    for k in ("loss", "IL_loss", "REF_loss") + (("RL_loss",) if tag == "sample" else ()):
        close(res["loss" if k == "loss" else "log_" + k], torch.tensor(float(g(k))), 1e-5, f"{tag} {k}")
    for k in ("d_act", "d_obj"):
        assert np.array_equal(res[k].numpy() == 0, g(k) == 0), (k, np.argwhere((res[k].numpy() == 0) != (g(k) == 0)))
        close(res[k], g(k), 1e-5, f"{tag} {k}")


@pytest.mark.parametrize("tag", MODES)
def test_poisoned_buffers_change_nothing(tag, monkeypatch):
    """Every torch.empty of the ops filled with NaN / 0xFF (the recorder's arrays by _golden_rollout): bit-identical step outputs, losses
    and logit gradients."""
    store = load_npz("reverie_policy.npz")
    want = _golden_rollout(store, tag, check=False)
    monkeypatch.setattr(torch, "empty", _poisoned_empty(torch.empty))
    got = _golden_rollout(store, tag, check=False)
    monkeypatch.undo()
    assert set(want) == set(got)
    for k, w in want.items():
        assert not bool(torch.isnan(got[k].double()).any()), k
        assert torch.equal(w, got[k]), k


def _ops_step(c, mode, stop_logit, strided=True, last_step=False, use_ids=False, **kw):
    """ops.policy_ref_step on a random_case: logits as row-strided views of wider leaves; returns the outputs and the state tensors"""
    from vln_hamt_amd import ops
    B, V = c["act"].shape
    O = c["obj"].shape[1]
    pad = 5 if strided else 0
    act_full = torch.cat([c["act"], torch.full((B, pad), 3.0)], 1).to(DEV).requires_grad_(True)
    obj_full = torch.cat([c["obj"], torch.full((B, pad), 9.0)], 1).to(DEV).requires_grad_(True)
    st = dict(ended=c["ended"].to(torch.uint8).to(DEV), mask=torch.empty(B, dtype=torch.float32, device=DEV),
              hist_len=torch.full((B,), 3, dtype=torch.int32, device=DEV), pred=torch.full((B,), -5, dtype=torch.int32, device=DEV),
              pred_id=torch.full((B,), -5, dtype=torch.int32, device=DEV), act_full=act_full, obj_full=obj_full)
    ids = dict(obj_id=c["obj_id"].to(DEV), goal_obj=c["goal"].to(DEV), pred_obj_id=st["pred_id"]) if use_ids else {}
    out = ops.policy_ref_step(act_full[:, :V], obj_full[:, :O], c["obj_len"].to(DEV), c["cand_len"].to(DEV), st["ended"], st["mask"], mode=mode,
                              stop_logit=stop_logit, target=c["target"].to(DEV), bt_mask=c["bt"].to(torch.uint8).to(DEV), ob_ang=c["ob_ang"].to(DEV),
                              hist_len=st["hist_len"], uniform=c["u"].to(DEV) if mode == "sample" else None, last_step=last_step,
                              pred_obj=st["pred"], **ids, **kw)
    return out, st


def _check_case(c, mode, stop_logit, last_step=False):
    B, V = c["act"].shape
    O = c["obj"].shape[1]
    ref_kw = dict(stop_logit=stop_logit, target=c["target"], obj_id=c["obj_id"].numpy(), goal_obj=c["goal"].numpy(), bt_mask=c["bt"],
                  ob_ang=c["ob_ang"].numpy(), last_step=last_step)
    np_ = lambda k: c[k].numpy()
    a_ref, o_ref = c["act"].clone().requires_grad_(True), c["obj"].clone().requires_grad_(True)
    o = reverie_step_ref(a_ref, o_ref, np_("obj_len"), np_("cand_len"), np_("ended"), mode, uniform=c["u"], **ref_kw)
    (ml, ref, logp, ent, a_t, env, prev), st = _ops_step(c, mode, stop_logit, last_step=last_step, use_ids=True)
    keep = torch.ones(B, dtype=torch.bool)
    if mode == "sample":
        x = torch.cat([c["act"], o["stop_col"][:, None]], 1).masked_fill(torch.cat([c["bt"], torch.zeros(B, 1, dtype=torch.bool)], 1), -float("inf"))
        keep = inverse_cdf(torch.softmax(x, 1), c["u"])[1] >= 1e-6
        assert int((~keep).sum()) * 1000 <= B, int((~keep).sum())
    assert torch.equal(a_t.cpu()[keep], o["action"][keep])
    same_t = a_t.cpu() == o["action"]
    if not bool(same_t.all()):                                       # an excluded row that chose the neighbour: the restatement follows the kernel's action
        a_ref, o_ref = c["act"].clone().requires_grad_(True), c["obj"].clone().requires_grad_(True)
        o = reverie_step_ref(a_ref, o_ref, np_("obj_len"), np_("cand_len"), np_("ended"), mode, forced_action=a_t.cpu(), **ref_kw)
    assert np.array_equal(env.cpu().numpy(), o["env_action"]) and np.array_equal(prev.cpu().numpy(), o["prev_angle"])
    assert np.array_equal(st["ended"].cpu().numpy().astype(bool), o["ended"]) and np.array_equal(st["mask"].cpu().numpy(), o["mask"])
    assert np.array_equal(st["hist_len"].cpu().numpy(), 3 + o["hist_inc"])
    assert np.array_equal(st["pred"].cpu().numpy(), apply_pred(np.full(B, -5, np.int32), o["pred_obj"]))
    assert np.array_equal(st["pred_id"].cpu().numpy(), apply_pred(np.full(B, -5, np.int32), o["pred_obj_id"]))
    close(ml, o["ml"], 1e-5, f"{mode} {stop_logit} ml")
    close(ref, o["ref"], 1e-5, f"{mode} {stop_logit} ref")
    close(logp, o["logp"], 1e-5, f"{mode} {stop_logit} logp")
    if mode == "sample":
        close(ent, o["ent"], 1e-5, f"{mode} {stop_logit} entropy")
    else:
        assert ent is None
    w = c["w"]
    (w[0] * o["ml"]).sum().add((w[1] * o["ref"]).sum()).add((w[2] * o["logp"]).sum()).add((w[3] * o["ent"]).sum() if mode == "sample" else 0.0).backward()
    wd = w.to(DEV)
    (wd[0] * ml).sum().add((wd[1] * ref).sum()).add((wd[2] * logp).sum()).add((wd[3] * ent).sum() if mode == "sample" else 0.0).backward()
    g_act, g_obj = st["act_full"].grad.cpu(), st["obj_full"].grad.cpu()
    assert float(g_act[:, V:].abs().max()) == 0.0 and float(g_obj[:, O:].abs().max()) == 0.0          # (the views' padding)
    r_obj = o_ref.grad if o_ref.grad is not None else torch.zeros(B, O)
    zeros_agree(g_act[:, :V], a_ref.grad, c["bt"] | torch.isinf(c["act"]), f"{mode} {stop_logit} d_act zeros")
    zeros_agree(g_obj[:, :O], r_obj, torch.isinf(c["obj"]), f"{mode} {stop_logit} d_obj zeros")
    close(g_act[:, :V], a_ref.grad, 1e-5, f"{mode} {stop_logit} d_act")
    close(g_obj[:, :O], r_obj, 1e-5, f"{mode} {stop_logit} d_obj")


@pytest.mark.parametrize("stop_logit", ["index", "value"])
@pytest.mark.parametrize("mode", MODES)
def test_policy_ref_step_vs_restatement(mode, stop_logit):
    """ops.policy_ref_step against the restatement on 1027 rows (no multiple of the 4 rows of a workgroup), V = 37, O = 7, then V in
    {63, 64, 255} and O in {1, 65, 256} one at a time: row-strided logit views, obj_len 0 rows, ended rows, ignored targets, STOP
    targets in both spellings, random masks, object targets looked up from the ids; the last shape also as the rollout's last step."""
    for i, (B, V, O) in enumerate(OP_SHAPES):
        _check_case(random_case(OP_SEED, B, V, O), mode, stop_logit, last_step=(i == len(OP_SHAPES) - 1))


def test_equal_object_maxima_pick_the_lowest_index():
    """The documented tie rule, not torch's: two equal maxima in obj_logit -> the lowest index, for column V ('index'), for the gradient's
    landing place ('value') and for the predicted object."""
    from vln_hamt_amd import ops
    B, V, O = 5, 6, 70
    obj = torch.full((B, O), -1.0)
    pairs = [(3, 66), (0, 69), (63, 64), (10, 11), (65, 68)]
    for b, (lo, hi) in enumerate(pairs):
        obj[b, lo] = obj[b, hi] = 2.5
    act = torch.full((B, V), -3.0)                                   # argmax chooses STOP in both modes
    z = lambda dt, v=0: torch.full((B,), v, dtype=dt, device=DEV)
    for stop_logit in ("index", "value"):
        x, xo = act.to(DEV).requires_grad_(True), obj.to(DEV).requires_grad_(True)
        pred = z(torch.int32, -5)
        ml, ref, logp, ent, a_t, env, prev = ops.policy_ref_step(x, xo, z(torch.int32, O), z(torch.int32, V + 1), z(torch.uint8), z(torch.float32),
                                                                 mode="argmax", stop_logit=stop_logit, target=z(torch.int64, V), pred_obj=pred)
        assert a_t.tolist() == [V] * B and env.tolist() == [-1] * B and pred.tolist() == [lo for lo, _ in pairs]
        ml.sum().backward()
        if stop_logit == "index":
            close(ml, torch.logsumexp(torch.cat([act, torch.tensor([float(lo) for lo, _ in pairs])[:, None]], 1), 1)
                  - torch.tensor([float(lo) for lo, _ in pairs]), 1e-5, "tie ml")
            assert float(xo.grad.abs().max()) == 0.0
        else:
            nz = xo.grad.cpu() != 0
            assert nz.sum(1).tolist() == [1] * B and [int(r.nonzero()[0]) for r in nz] == [lo for lo, _ in pairs]


def test_row_without_a_live_action_column():
    """Every action column -inf or masked: 'index' chooses STOP with log-probability 0 in argmax mode; no NaN in any output or gradient,
    in both modes of the STOP column and in sample mode too."""
    from vln_hamt_amd import ops
    B, V, O = 4, 9, 5
    g = torch.Generator().manual_seed(1)
    act = torch.randn(B, V, generator=g)
    act[0] = -float("inf")
    act[1, 4:] = -float("inf")
    bt = torch.zeros(B, V, dtype=torch.uint8)
    bt[1, :4] = 1                                                     # row 1: what is not -inf is masked
    obj = torch.randn(B, O, generator=g)
    z = lambda dt, v=0: torch.full((B,), v, dtype=dt, device=DEV)
    for stop_logit in ("index", "value"):
        for mode in ("argmax", "sample"):
            x, xo = act.to(DEV).requires_grad_(True), obj.to(DEV).requires_grad_(True)
            ml, ref, logp, ent, a_t, env, prev = ops.policy_ref_step(x, xo, z(torch.int32, O), z(torch.int32, 5), z(torch.uint8), z(torch.float32), mode=mode,
                                                                     stop_logit=stop_logit, target=z(torch.int64, V), ref_target=z(torch.int64, 2),
                                                                     bt_mask=bt.to(DEV), uniform=z(torch.float32, 0.5))
            (ml.sum() + ref.sum() + logp.sum() + (ent.sum() if ent is not None else 0.0)).backward()
            assert a_t[:2].tolist() == [V, V] and env[:2].tolist() == [-1, -1], (stop_logit, mode, a_t)
            assert ml[:2].tolist() == [0.0, 0.0]
            if mode == "argmax":
                assert logp[:2].tolist() == [0.0, 0.0]
            else:                                                     # (Categorical's clamp: log(1 - eps))
                assert float(logp[:2].abs().max()) <= 2e-7
            for t_ in (ml, ref, logp, x.grad, xo.grad) + ((ent,) if ent is not None else ()):
                assert not bool(torch.isnan(t_).any()), (stop_logit, mode)
            assert float(x.grad[:2].abs().max()) == 0.0


@pytest.mark.parametrize("stop_logit", ["index", "value"])
def test_object_ids_give_what_an_explicit_ref_target_gives(stop_logit):
    c = random_case(7, 203, 37, 7)
    o = reverie_step_ref(c["act"], c["obj"], c["obj_len"].numpy(), c["cand_len"].numpy(), c["ended"].numpy(), "teacher", target=c["target"],
                         obj_id=c["obj_id"].numpy(), goal_obj=c["goal"].numpy())
    assert int((o["ref_target"] >= 0).sum()) >= 5 and int(((o["ref_target"] < 0) & (c["target"] != -100)).sum()) >= 5
    outs = []
    for kw in (dict(use_ids=True), dict(ref_target=o["ref_target"].to(DEV))):
        (ml, ref, logp, ent, a_t, env, prev), st = _ops_step(c, "argmax", stop_logit, **kw)
        (ml.sum() + (c["w"][1].to(DEV) * ref).sum() + logp.sum()).backward()
        outs.append((ref.detach().cpu(), st["act_full"].grad.cpu(), st["obj_full"].grad.cpu()))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    assert float(outs[0][0].abs().max()) > 0


def test_nav_goal_set_episodes_equal_a_handed_in_target():
    """step(nav=GoalSetEpisodes) on tests/golden/nav_tiny == the same step with target and bt_mask from ops.nav_observe handed in and
    ops.nav_advance_goals called by hand: actions, losses, rewards, the episodes' nodes and both logit gradients, bit for bit."""
    from test_gpu_nav_tasks import _random_setup, _random_step
    from vln_hamt_amd import ops
    from vln_hamt_amd.agent import GoalSetEpisodes, ReverieRolloutRecorder
    B, V, O, T = 9, 12, 5, 4
    G, rng, nbrs, scan, gts, start, gpad, glen, name = _random_setup(B, V, 77)

    def episodes():
        return GoalSetEpisodes(G, T, B, max_gt=65, max_goals=4).reset([G.scans[s] for s in scan], [name(b, v) for b, v in enumerate(start)],
                                                                      [[name(b, v) for v in gt] for b, gt in enumerate(gts)],
                                                                      [[name(b, gt[-1])] for b, gt in enumerate(gts)])
    navs = episodes(), episodes()
    recs = ReverieRolloutRecorder(T, B, DEV).reset(B), ReverieRolloutRecorder(T, B, DEV).reset(B)
    gen = torch.Generator().manual_seed(3)
    leaves, stops = [], 0
    for t in range(T):
        cur, ended = navs[0].cur.cpu().numpy(), recs[0].ended.cpu().numpy().astype(bool)
        cand, cl, _ = _random_step(rng, nbrs, scan, cur, ended, V)
        act = torch.randn(B, V, generator=gen) * 2 + 1
        act[torch.arange(V)[None] >= torch.from_numpy(cl - 1)[:, None]] = -float("inf")
        obj, ol = torch.randn(B, O, generator=gen), torch.randint(0, O + 1, (B,), generator=gen).to(torch.int32).to(DEV)
        xs = [(act.to(DEV).requires_grad_(True), obj.to(DEV).requires_grad_(True)) for _ in range(2)]
        leaves.append(xs)
        a0, env0, _ = recs[0].step(t, *xs[0], ol, cand_lens=d(cl), feedback="argmax", nav=navs[0], cand_nodes=d(cand), teacher_mode="shortest")
        tgt, btm = ops.nav_observe(navs[1], t, d(cand), d(cl), recs[1].ended, mode="shortest")
        stops += int((tgt == d(cl).long() - 1).sum())
        a1, env1, _ = recs[1].step(t, *xs[1], ol, target=tgt, bt_mask=btm, cand_lens=d(cl), feedback="argmax", sync=False)
        ops.nav_advance_goals(navs[1], d(cand), env1, recs[1].mask[t], recs[1].reward[t])
        assert torch.equal(a0, a1) and np.array_equal(env0, env1.cpu().numpy()) and torch.equal(navs[0].cur, navs[1].cur), t
        assert torch.equal(recs[0].target, tgt) and torch.equal(recs[0].bt_mask, btm)
    for k in ("ml", "ref", "logp", "mask", "reward", "ended", "hist_len", "_pred"):
        assert torch.equal(getattr(recs[0], k), getattr(recs[1], k)), k
    for rec in recs:
        rec.loss(train_ml=0.3)[0].add(rec.stacked("logp").sum()).backward()
    for (x0, o0), (x1, o1) in leaves:
        assert torch.equal(x0.grad, x1.grad) and torch.equal(o0.grad, o1.grad) and not bool(torch.isnan(x0.grad).any())
    assert float(recs[0].ml.abs().sum()) > 0 and not bool(torch.isnan(recs[0].ml).any())
    print(f"[nav] teacher STOPs (target == cand_len - 1, read as V by the step): {stops}")


def test_env_action_is_the_only_transfer_to_the_host():
    """ReverieRolloutRecorder.step under torch.cuda.set_sync_debug_mode('error'): nothing synchronises but the declared copy of the int32
    environment actions (non-blocking + one event wait); sync=False copies nothing."""
    from vln_hamt_amd.agent import ReverieRolloutRecorder
    c = random_case(2, 8, 37, 7)
    B, V = c["act"].shape
    act, obj = c["act"].to(DEV).requires_grad_(True), c["obj"].to(DEV).requires_grad_(True)
    kw = dict(target=c["target"].to(DEV), cand_lens=c["cand_len"].to(DEV), bt_mask=c["bt"].to(torch.uint8).to(DEV), ob_ang_feats=c["ob_ang"].to(DEV),
              obj_ids=c["obj_id"].to(DEV), goal_obj=c["goal"].to(DEV))
    ol = c["obj_len"].to(DEV)
    forced = torch.tensor([0, V, 1, -100, V, 0, 2, 1]).to(DEV)
    rec = ReverieRolloutRecorder(3, B, DEV).reset(B)
    rec.step(0, act, obj, ol, feedback="sample", **kw)                 # (first use: library load, allocator)
    rec.reset()
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a_t, env, prev = rec.step(0, act, obj, ol, feedback="sample", forced_action=forced, **kw)
        a2, env_dev, _ = rec.step(1, act, obj, ol, feedback="argmax", sync=False, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert isinstance(env, np.ndarray) and env.dtype == np.int32 and env.tolist() == [0, -1, 1, -1, -1, 0, 2, 1]
    assert torch.is_tensor(env_dev) and env_dev.is_cuda and env_dev.dtype == torch.int32
    slots, ids = rec.predicted_objects()
    ol_h = c["obj_len"].numpy()
    assert slots.shape == (B,) and ids.shape == (B,) and slots[3] == -1                                # (row 3 was ignored: ended without a prediction)
    for b in (1, 4):                                                                                   # the forced STOPs of step 0
        assert (slots[b] == -1) == (ol_h[b] == 0) and (ids[b] == -1) == (ol_h[b] == 0), (b, slots, ids, ol_h)


def test_captured_step_matches_eager():
    """graph.GraphedInference over ReverieRolloutRecorder.step(sync=False), argmax: bit-identical to the eager step; the in-place state
    (`ended`, `hist_len`, the predictions) moves exactly once per call, the capturing one included."""
    from vln_hamt_amd.agent import ReverieRolloutRecorder
    from vln_hamt_amd.graph import GraphedInference
    c = random_case(5, 16, 37, 7)
    B = 16
    args = (c["act"].to(DEV), c["obj"].to(DEV))
    kw = dict(cand_lens=c["cand_len"].to(DEV), bt_mask=c["bt"].to(torch.uint8).to(DEV), ob_ang_feats=c["ob_ang"].to(DEV), obj_ids=c["obj_id"].to(DEV),
              goal_obj=c["goal"].to(DEV), target=c["target"].to(DEV))
    ol = c["obj_len"].to(DEV)
    outs = {}
    with torch.no_grad():
        for name in ("graph", "eager"):
            rec = ReverieRolloutRecorder(1, B, DEV)                    # (T_max 1: every step is the last one, predictions for all)
            fn = lambda a, o, rec=rec: rec.step(0, a, o, ol, feedback="argmax", sync=False, **kw) + (rec.logp[0], rec.ml[0], rec.ref[0])
            call = fn if name == "eager" else (lambda a, o, gi=GraphedInference(fn, state=(rec.ended, rec.hist_len, rec._pred)): gi("s", a, o))
            runs = []
            for _ in range(2):
                rec.reset(fresh_draws=False)
                out = [t.clone() for t in call(*args)]
                assert int(rec.hist_len.min()) == 2 and int(rec.hist_len.max()) == 2
                runs.append(out + [rec.ended.clone(), rec._pred.clone()])
            outs[name] = runs
    for e_run, g_run in zip(outs["eager"], outs["graph"]):
        for w, g_ in zip(e_run, g_run):
            assert torch.equal(w, g_)
    assert int((outs["graph"][0][-1][0] >= 0).sum()) > 0
