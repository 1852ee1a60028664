#!/usr/bin/env python3
"""Every output of ops.policy_step and ops.policy_ref_step, forward and backward, from a given libhamt_hip.so, as one .npz: the
evidence for "a change to csrc/policy.hip moved no bit".

    python tools/policy_dump.py --lib PATH/libhamt_hip.so --out a.npz       # once per library, each in a fresh process
    python tools/policy_dump.py --compare a.npz b.npz [--report FILE]      # byte for byte; exit status 1 unless every array is equal

The inputs are the ones the GPU tests build: tests/_policy_ref.uniform_case() with the generator seed of
test_policy_step_vs_restatement, and tests/_reverie_policy_ref.random_case(OP_SEED, *shape) for every entry of OP_SHAPES.  All three
modes, both stop_logit values, and 'sample' twice: with injected uniforms and with the kernel's own draws (ops.manual_seed and the
call id fixed).  Arrays are compared as raw bytes, so a NaN equals only a NaN of the same bit pattern."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
MODES = ("teacher", "argmax", "sample", "sample_own_draw")
SEED, CALL_ID = 1234, 77


def dump(lib, out):
    import torch
    from vln_hamt_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)                # before the first load
    from vln_hamt_amd import ops
    from _policy_ref import uniform_case
    from _reverie_policy_ref import OP_SEED, OP_SHAPES, random_case
    dev = torch.device("cuda:0")
    arrays = {}

    def put(tag, **ts):
        for k, t in ts.items():
            if t is not None:
                arrays[f"{tag}/{k}"] = t.detach().cpu().numpy()

    logit_c, u = uniform_case()
    B, V = logit_c.shape
    g = torch.Generator().manual_seed(5)
    n = torch.isfinite(logit_c).sum(1)
    target = (torch.rand(B, generator=g) * n).long().clamp(max=V - 1)
    target[torch.rand(B, generator=g) < 0.1] = -100
    bt = (torch.rand(B, V, generator=g) < 0.2) & (torch.arange(V)[None] < (n - 1)[:, None])
    ended0 = torch.rand(B, generator=g) < 0.15
    ob_ang = torch.randn(B, V, 4, generator=g)
    w = torch.randn(3, B, generator=g).to(dev)
    for mode in MODES:
        ops.manual_seed(SEED, dev)
        x = logit_c.to(dev).requires_grad_(True)
        ended, mask = ended0.to(torch.uint8).to(dev), torch.empty(B, dtype=torch.float32, device=dev)
        hist_len = torch.full((B,), 3, dtype=torch.int32, device=dev)
        ml, logp, ent, a_t, env, prev = ops.policy_step(
            x, n.to(torch.int32).to(dev), ended, mask, mode=mode.split("_")[0], target=target.to(dev), bt_mask=bt.to(torch.uint8).to(dev),
            ob_ang=ob_ang.to(dev), hist_len=hist_len, uniform=u.to(dev) if mode == "sample" else None, call_id=CALL_ID)
        ((w[0] * ml).sum() + (w[1] * logp).sum() + ((w[2] * ent).sum() if ent is not None else 0.0)).backward()
        put(f"step/{mode}", ml=ml, logp=logp, ent=ent, action=a_t, env_action=env, prev_angle=prev, ended=ended, mask=mask, hist_len=hist_len,
            d_logit=x.grad)

    for B, V, O in OP_SHAPES:
        c = random_case(OP_SEED, B, V, O)
        w = c["w"].to(dev)
        for stop_logit in ("index", "value"):
            for mode in MODES:
                for last_step in (False, True):
                    ops.manual_seed(SEED, dev)
                    act_full = torch.cat([c["act"], torch.full((B, 5), 3.0)], 1).to(dev).requires_grad_(True)      # row-strided views, as the test
                    obj_full = torch.cat([c["obj"], torch.full((B, 5), 9.0)], 1).to(dev).requires_grad_(True)
                    ended, mask = c["ended"].to(torch.uint8).to(dev), torch.empty(B, dtype=torch.float32, device=dev)
                    hist_len = torch.full((B,), 3, dtype=torch.int32, device=dev)
                    pred, pred_id = (torch.full((B,), -5, dtype=torch.int32, device=dev) for _ in range(2))
                    ml, ref, logp, ent, a_t, env, prev = ops.policy_ref_step(
                        act_full[:, :V], obj_full[:, :O], c["obj_len"].to(dev), c["cand_len"].to(dev), ended, mask, mode=mode.split("_")[0],
                        stop_logit=stop_logit, target=c["target"].to(dev), obj_id=c["obj_id"].to(dev), goal_obj=c["goal"].to(dev),
                        bt_mask=c["bt"].to(torch.uint8).to(dev), ob_ang=c["ob_ang"].to(dev), hist_len=hist_len,
                        uniform=c["u"].to(dev) if mode == "sample" else None, last_step=last_step, call_id=CALL_ID, pred_obj=pred,
                        pred_obj_id=pred_id)
                    ((w[0] * ml).sum() + (w[1] * ref).sum() + (w[2] * logp).sum() + ((w[3] * ent).sum() if ent is not None else 0.0)).backward()
                    put(f"ref/{B}x{V}x{O}/{stop_logit}/{mode}/last{int(last_step)}", ml=ml, ref=ref, logp=logp, ent=ent, action=a_t, env_action=env,
                        prev_angle=prev, ended=ended, mask=mask, hist_len=hist_len, pred_obj=pred, pred_obj_id=pred_id, d_act=act_full.grad,
                        d_obj=obj_full.grad)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print(f"policy_dump: {len(arrays)} arrays from {_lib.LIB_PATH} -> {out}", flush=True)


def compare(a, b, report):
    fa, fb = np.load(a), np.load(b)
    lines, equal = [], 0
    if sorted(fa.files) != sorted(fb.files):
        lines.append(f"array names differ: {sorted(set(fa.files) ^ set(fb.files))}")
    names = sorted(set(fa.files) & set(fb.files))
    for k in names:
        x, y = fa[k], fb[k]
        same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        equal += same
        if not same:
            lines.append(f"DIFFERS {k}: {x.dtype}{x.shape} vs {y.dtype}{y.shape}"
                         + (f", {int((x.view(np.uint8) != y.view(np.uint8)).sum())} bytes" if x.shape == y.shape and x.dtype == y.dtype else ""))
    nans = sum(int(np.isnan(fa[k]).sum()) for k in names if fa[k].dtype.kind == "f")
    head = [f"arrays compared: {len(names)}", f"arrays equal (byte for byte): {equal}", f"elements: {sum(fa[k].size for k in names)} ({nans} NaN in the first file)"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if report:
        with open(report, "w") as f:
            f.write(text)
    return 0 if equal == len(names) and not lines else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.report))
    dump(a.lib, a.out)
