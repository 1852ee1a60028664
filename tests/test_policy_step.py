"""Not gpu: the fused per-step action choice and losses of the finetune agents (vln_hamt_amd/csrc/policy.hip, ops.policy_step,
agent.RolloutRecorder) -- the torch restatement the GPU tests compare against reproduces the REFERENCE's own statements
(tests/golden/policy_step.npz, tools/gen_policy_step_golden.py), the new entry points are declared and bound, and the cross-compiled
kernels use no scratch memory."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from _policy_ref import CASES, critic_ref, critic_state_dict, golden_hidden, inverse_cdf, policy_step_ref, rollout_loss_ref
from _util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry_points():
    from vln_hamt_amd import _lib
    return _lib.SIGNATURES["hamt_policy_step_fwd"], _lib.SIGNATURES["hamt_policy_step_bwd"]


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_reproduces_the_reference_statements(tag):
    """tests/_policy_ref.py against the golden of the reference's own statements (agent_cmt.py:336-375, 382-385, 399-401, 447, 476-522):
    every per-step output, the final loss with its logged sums, d loss / d logit per step.  In `sample` the reference's draw (torch's
    stream) goes in as the forced action; `argmax` and `teacher` choose for themselves."""
    _entry_points()                                # (this file tests the feature: it fails where the feature is absent)
    store = load_npz("policy_step.npz")
    feedback, normalize = CASES[tag]
    g = lambda k: store[f"{tag}/{k}"]
    T, B = store["in/cand_len"].shape
    ignoreid = int(store["meta/ignoreid"])
    logits = torch.from_numpy(store["in/logits"]).requires_grad_(True)
    ended, hist_len, steps = np.zeros(B, bool), np.ones(B, np.int32), []
    for t in range(T):
        o = policy_step_ref(logits[t], store["in/cand_len"][t], ended, feedback, target=torch.from_numpy(g("target")[t]), bt_mask=g("bt_mask")[t],
                            ob_ang=store["in/ob_ang"][t], forced_action=torch.from_numpy(g("a_t")[t]) if feedback == "sample" else None,
                            ignoreid=ignoreid)
        assert np.array_equal(o["action"].numpy(), g("a_t")[t]), (t, o["action"], g("a_t")[t])
        assert np.array_equal(o["env_action"], g("env_action")[t]) and np.array_equal(o["mask"], g("mask")[t])
        assert np.array_equal(o["prev_angle"], g("prev_angle")[t])
        ended, hist_len = o["ended"], hist_len + o["hist_inc"]
        assert np.array_equal(ended, g("ended")[t]) and np.array_equal(hist_len, g("hist_len")[t])
        assert abs(float(o["ml"].detach().sum()) - float(g("ml_sum")[t])) <= 1e-5 * max(1.0, abs(float(g("ml_sum")[t])))
        assert float(np.abs(o["logp"].detach().numpy() - g("logp")[t]).max()) <= 1e-6
        if feedback == "sample":
            assert float(np.abs(o["ent"].detach().numpy() - g("ent")[t]).max()) <= 1e-6
        steps.append(o)
    hid, last_h = golden_hidden(store)
    critic = critic_ref(critic_state_dict(store))
    loss, logs = rollout_loss_ref(steps, store["in/rewards"], torch.from_numpy(hid), torch.from_numpy(last_h), critic, feedback, normalize,
                                  float(g("train_ml")), weights=store["in/weights"] if feedback == "argmax" else None)
    loss.backward()
    assert abs(float(loss) - float(g("loss"))) <= 1e-5 * max(1.0, abs(float(g("loss"))))
    for k in ("IL_loss",) + (("RL_loss", "total") if feedback == "sample" else ()):
        assert abs(logs[k] - float(g(k))) <= 1e-5 * max(1.0, abs(float(g(k)))), k
    for k in (("policy", "critic", "entropy") if feedback == "sample" else ()):
        assert abs(logs[k] - float(g(k + "_sum"))) <= 1e-4 * max(1.0, abs(float(g(k + "_sum")))), k
    if feedback == "sample":
        assert abs(sum(float(s["ent"].detach().sum()) for s in steps) - float(g("entropy_logged"))) <= 1e-5 * max(1.0, float(g("entropy_logged")))
    ref = g("d_logit")
    assert np.array_equal(logits.grad.numpy() == 0, ref == 0)
    assert float(np.abs(logits.grad.numpy() - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))


def test_golden_holds_the_corners_the_issue_names():
    store = load_npz("policy_step.npz")
    _entry_points()
    T, B = store["in/cand_len"].shape
    assert (B, T) == (6, 5) and len(set(store["in/cand_len"].flatten().tolist())) > 3                       # ragged
    assert np.isinf(store["in/logits"]).any()
    e = store["sample_total/ended"]
    assert e[1].any() and not e[-1].all()                                                                    # early ends, and episodes that never end
    raw_best = store["in/logits"].argmax(2)
    assert np.take_along_axis(store["argmax/bt_mask"], raw_best[..., None], 2).sum() >= 3                    # the mask hits the would-be argmax
    lp = store["sample_total/logp"]
    assert abs(float(lp.min()) - float(np.log(np.finfo(np.float32).eps))) < 1e-6                             # the clamp corner
    t, b = np.unravel_index(lp.argmin(), lp.shape)
    row = store["in/logits"][t, b]
    assert abs(float(row[np.isfinite(row)].max() - row[store["sample_total/a_t"][t, b]]) - 40.0) < 1e-4
    assert float(np.abs(store["sample_total/d_logit"][t, b]).max()) > 0                                      # (IL and entropy terms still flow there)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "policy_step.npz")) < 200 * 1024


def test_inverse_cdf_exclusions_stay_under_the_cap():
    """The injected-uniform GPU test may exclude rows whose u lies within 1e-6 of a CDF boundary, at most 1 in 1000: its seed, checked here."""
    _entry_points()
    from _policy_ref import uniform_case
    logit, u = uniform_case()
    a, margin = inverse_cdf(torch.softmax(logit, 1), u)
    assert int((margin < 1e-6).sum()) * 1000 <= logit.shape[0], int((margin < 1e-6).sum())
    assert bool((torch.softmax(logit.double(), 1).gather(1, a[:, None]) > 0).all())


def test_symbols_in_header_and_binding():
    fwd, bwd = _entry_points()
    src = open(os.path.join(ROOT, "include", "hamt.h")).read()
    for name, sig in (("hamt_policy_step_fwd", fwd), ("hamt_policy_step_bwd", bwd)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(sig), name
    assert re.search(r"#define HAMT_POLICY_SAMPLE 2", src)
    from vln_hamt_amd import _lib, ops
    assert '"policy.hip"' in open(os.path.join(ROOT, "vln_hamt_amd", "csrc", "build.py")).read()
    assert ops.POLICY_MODES == {"teacher": 0, "argmax": 1, "sample": 2}
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert hasattr(lib, "hamt_policy_step_fwd") and hasattr(lib, "hamt_policy_step_bwd") and lib.hamt_version() == 2
    from vln_hamt_amd.agent import RolloutRecorder
    assert callable(RolloutRecorder.step) and callable(RolloutRecorder.loss)


def test_policy_kernels_use_no_scratch(tmp_path):
    """The cross-compiled gfx950 code object of policy.hip: no scratch memory, no spilled registers (read as tests/test_kernel_resources.py does)."""
    from test_kernel_resources import OBJCOPY, READELF, _code_objects
    from vln_hamt_amd import _lib
    _entry_points()
    if not (os.path.exists(READELF) and os.path.exists(OBJCOPY)):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = []
    for co in _code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or not re.search(r"policy_(step|ref)_(fwd|bwd)_kernel", name.group(1)):
                continue
            num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
            seen.append(name.group(1))
            assert num("vgpr_spill_count") == 0 and num("sgpr_spill_count") == 0 and num("private_segment_fixed_size") == 0, (name.group(1), blk)
            assert num("group_segment_fixed_size") == 0, name.group(1)                         # wave reductions only: no LDS
    assert len(seen) == 4 and all(sum(k in s for s in seen) == 1 for k in ("policy_step_fwd", "policy_step_bwd", "policy_ref_fwd", "policy_ref_bwd")), seen
