"""Not gpu: REVERIE's rollout step (vln_hamt_amd/csrc/policy.hip -> ops.policy_ref_step -> agent.ReverieRolloutRecorder) -- the torch
restatement the GPU tests compare against (tests/_reverie_policy_ref.py) reproduces the REFERENCE's own statements
(tests/golden/reverie_policy.npz, tools/gen_reverie_policy_golden.py), the reference's 'index' quirk is pinned, the entry points are
declared and bound, and the seeds of the GPU sample cases respect the exclusion cap."""
import os
import re

import numpy as np
import pytest
import torch

from _policy_ref import critic_ref, critic_state_dict, golden_hidden
from _policy_ref import rollout_loss_ref as a2c_rollout_loss_ref
from _reverie_policy_ref import MODES, OP_SEED, OP_SHAPES, apply_pred, random_case, reverie_step_ref, rollout_loss_ref, sample_margin
from _util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry_points():
    from vln_hamt_amd import _lib
    return _lib.SIGNATURES["hamt_policy_ref_step_fwd"], _lib.SIGNATURES["hamt_policy_ref_step_bwd"]


def golden_rollout_ref(store, tag, stop_logit="index"):
    """the golden's scripted rollout through the restatement: (steps, pred_obj_id per step, loss, logs, act leaf, obj leaf)"""
    g = lambda k: store[f"{tag}/{k}"]
    T, B = store["in/cand_len"].shape
    ignoreid = int(store["meta/ignoreid"])
    act = torch.from_numpy(store["in/act_logits"]).requires_grad_(True)
    obj = torch.from_numpy(store["in/obj_logits"]).requires_grad_(True)
    ended, steps, preds = np.zeros(B, bool), [], []
    pred = np.full(B, -1, np.int32)
    for t in range(T):
        o = reverie_step_ref(act[t], obj[t], store["in/obj_len"][t], store["in/cand_len"][t], ended, tag, stop_logit=stop_logit,
                             target=torch.from_numpy(g("target")[t]), obj_id=store["in/obj_ids"][t], goal_obj=store["in/goal_obj"],
                             bt_mask=g("bt_mask")[t], ob_ang=store["in/ob_ang"][t],
                             forced_action=torch.from_numpy(g("a_t")[t]) if tag == "sample" else None, last_step=t == T - 1, ignoreid=ignoreid)
        pred = apply_pred(pred, o["pred_obj_id"])
        preds.append(pred)
        steps.append(o)
        ended = o["ended"]
    if tag == "sample":
        hid, last_h = golden_hidden(store)
        loss, logs = a2c_rollout_loss_ref(steps, store["in/rewards"], torch.from_numpy(hid), torch.from_numpy(last_h),
                                          critic_ref(critic_state_dict(store)), "sample", "total", float(g("train_ml")))
        rf = sum(s["ref"].sum() for s in steps) / B
        loss, logs = loss + rf, dict(logs, REF_loss=float(rf.detach()))
    else:
        loss, logs = rollout_loss_ref(steps, float(g("train_ml")), weights=store["in/weights"] if tag == "argmax" else None)
    return steps, preds, loss, logs, act, obj


@pytest.mark.parametrize("tag", MODES)
def test_restatement_reproduces_the_reference_statements(tag):
    """tests/_reverie_policy_ref.py against the golden of the reference's own statements (reverie/agent.py:141-165, 253-307, 311-314,
    328-330, 368, 404-445, 448-451): every per-step output, the object target looked up from the ids, the predicted object, the final
    loss with IL_loss / REF_loss (/ RL_loss), and both logit gradients."""
    _entry_points()                                # (this file tests the feature: it fails where the feature is absent)
    store = load_npz("reverie_policy.npz")
    g = lambda k: store[f"{tag}/{k}"]
    T, B = store["in/cand_len"].shape
    V = store["in/act_logits"].shape[2]
    steps, preds, loss, logs, act, obj = golden_rollout_ref(store, tag)
    hist_len = np.ones(B, np.int32)
    for t, o in enumerate(steps):
        assert np.array_equal(o["stop_col"].numpy(), g("stop_col")[t]) and np.array_equal(o["stop_col"].numpy(), o["best"].float().numpy())
        assert np.array_equal(o["ref_target"].numpy(), g("ref_target")[t]), (t, o["ref_target"], g("ref_target")[t])
        assert np.array_equal(o["action"].numpy(), g("a_t")[t]), (t, o["action"], g("a_t")[t])
        assert np.array_equal(o["env_action"], g("env_action")[t]) and np.array_equal(o["mask"], g("mask")[t])
        assert np.array_equal(o["prev_angle"], g("prev_angle")[t]) and np.array_equal(o["ended"], g("ended")[t])
        hist_len = hist_len + o["hist_inc"]
        assert np.array_equal(hist_len, g("hist_len")[t]) and np.array_equal(preds[t], g("pred_obj_id")[t]), (t, preds[t], g("pred_obj_id")[t])
        for k in ("ml", "ref"):
            assert abs(float(o[k].detach().sum()) - float(g(k + "_sum")[t])) <= 1e-5 * max(1.0, abs(float(g(k + "_sum")[t]))), (k, t)
        assert float(np.abs(o["logp"].detach().numpy() - g("logp")[t]).max()) <= 1e-6
        if tag == "sample":
            assert float(np.abs(o["ent"].detach().numpy() - g("ent")[t]).max()) <= 1e-6
    loss.backward()
    assert abs(float(loss) - float(g("loss"))) <= 1e-5 * max(1.0, abs(float(g("loss"))))
    for k in ("IL_loss", "REF_loss") + (("RL_loss",) if tag == "sample" else ()):
        assert abs(logs[k] - float(g(k))) <= 1e-5 * max(1.0, abs(float(g(k)))), k
    for got, ref in ((act.grad.numpy(), g("d_act")), (obj.grad.numpy(), g("d_obj"))):
        assert np.array_equal(got == 0, ref == 0)
        assert float(np.abs(got - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))


def test_golden_holds_the_corners_the_issue_names():
    _entry_points()
    store = load_npz("reverie_policy.npz")
    T, B = store["in/cand_len"].shape
    V, O = store["in/act_logits"].shape[2], store["in/obj_logits"].shape[2]
    assert (B, T, V, O) == (6, 4, 9, 5)
    assert len(set(store["in/cand_len"].flatten().tolist())) > 3 and len(set(store["in/obj_len"].flatten().tolist())) > 3      # ragged
    assert (store["in/obj_len"] == 0).any()
    t_, r_ = store["teacher/target"], store["teacher/ref_target"]
    assert ((t_ == V) & (r_ == -100)).any() and ((t_ == V) & (r_ >= 0)).any()          # a teacher STOP with the goal absent, and with it in view
    stopped_blind = (store["teacher/a_t"] == V) & (store["in/obj_len"] == 0)
    assert stopped_blind.any() and (store["teacher/pred_obj_id"][-1][stopped_blind.any(0)] == -1).all()                         # None
    for tag in MODES:
        e = store[f"{tag}/ended"]
        assert e[1].any() and not e[-2].all(), tag                                     # an early stop; episodes the last step forces
        assert (store[f"{tag}/pred_obj_id"][-1][~e[-2] & (store["in/obj_len"][-1] > 0)] >= 0).all()
    assert store["argmax/bt_mask"].sum() >= 3 and store["sample/bt_mask"].sum() >= 3 and store["teacher/bt_mask"].sum() == 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "reverie_policy.npz")) < 100 * 1024


def test_index_quirk_is_pinned():
    """stop_logit='index' (the reference, :253-254): column V is the arg-max INDEX and the action terms send exactly nothing to obj_logit;
    'value': their gradient arrives at the arg-max element alone."""
    _entry_points()
    c = random_case(3, 64, 9, 5)
    for stop_logit in ("index", "value"):
        act, obj = c["act"].clone().requires_grad_(True), c["obj"].clone().requires_grad_(True)
        o = reverie_step_ref(act, obj, c["obj_len"].numpy(), c["cand_len"].numpy(), c["ended"].numpy(), "sample", stop_logit=stop_logit,
                             target=c["target"], bt_mask=c["bt"], uniform=c["u"])
        (o["ml"].sum() + (c["w"][0, :64] * o["logp"]).sum() + o["ent"].sum()).backward()
        if stop_logit == "index":
            assert torch.equal(o["stop_col"], c["obj"].argmax(1).float())
            assert obj.grad is None or float(obj.grad.abs().max()) == 0.0
        else:
            assert torch.equal(o["stop_col"], c["obj"].max(1)[0])
            off = torch.ones_like(obj.grad, dtype=torch.bool)
            off[torch.arange(64), c["obj"].argmax(1)] = False
            assert float(obj.grad[off].abs().max()) == 0.0 and float(obj.grad.abs().max()) > 0.0


def test_sample_seeds_stay_under_the_exclusion_cap():
    """The GPU sample cases may exclude rows whose uniform lies within 1e-6 of a CDF boundary, at most 1 in 1000
    (tests/test_gpu_policy_step.py's cap): their seed and shapes, checked here."""
    _entry_points()
    for B, V, O in OP_SHAPES:
        c = random_case(OP_SEED, B, V, O)
        for stop_logit in ("index", "value"):
            n = int((sample_margin(c, stop_logit) < 1e-6).sum())
            assert n * 1000 <= B, (B, V, O, stop_logit, n)


def test_symbols_in_header_and_binding():
    fwd, bwd = _entry_points()
    src = open(os.path.join(ROOT, "include", "hamt.h")).read()
    for name, sig in (("hamt_policy_ref_step_fwd", fwd), ("hamt_policy_ref_step_bwd", bwd)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(sig), name
    assert re.search(r"#define HAMT_STOP_LOGIT_INDEX 0", src) and re.search(r"#define HAMT_STOP_LOGIT_VALUE 1", src)
    from vln_hamt_amd import _lib, ops
    assert ops.STOP_LOGITS == {"index": 0, "value": 1}
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert hasattr(lib, "hamt_policy_ref_step_fwd") and hasattr(lib, "hamt_policy_ref_step_bwd") and lib.hamt_version() == 2
    from vln_hamt_amd.agent import ReverieRolloutRecorder, RolloutRecorder
    assert issubclass(ReverieRolloutRecorder, RolloutRecorder) and callable(ReverieRolloutRecorder.predicted_objects)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HamtError):
            ops.policy_ref_step(torch.zeros(2, 3), torch.zeros(2, 2), torch.ones(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32),
                                torch.zeros(2, dtype=torch.uint8), torch.zeros(2))
