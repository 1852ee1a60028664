#!/usr/bin/env python3
"""Everything the seven optimiser classes of vln_hamt_amd.optim compute over a short schedule, from the Python sources under a given
root: the evidence for "a change to the Python side of the optimisers moved no bit" when both roots load the same libhamt_hip.so.

    python tools/optim_class_dump.py --src ROOT --out a.json              # once per source tree, each in a fresh process
    python tools/optim_class_dump.py --compare a.json b.json [--report FILE]     # exit status 1 unless every array is equal

ROOT holds vln_hamt_amd/ (with its built library) and tests/_adamw_ref.py.  Per class, the five steps of _adamw_ref.py_case() -- eight
bare parameters in two groups, PY_LAG without a gradient in steps 2 and 3, the groups' learning rates of PY_LR, the clip biting in
steps 1, 3 and 5 -- three ways: "eager" (clip_grad_norm_ + step() + zero_grad()), "staged" (prepare_step() / launch_step(), the calls
a captured step makes) and "dropped" (eager, with a pass that is clipped and then dropped by zero_grad() after step 2).  After step 3
state_dict() goes into a fresh instance over clones of the parameters, and the fresh instance takes steps 4 and 5.  Recorded per run
and step: every table host_table() returned, _steps, and the arenas p, g, m, v, p16, slow and _stats; at the end every tensor of
state_dict() and the SHA-256 of the rest of its structure.  The file format is tools/image_dump.py's."""
import argparse
import copy
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from image_dump import compare  # noqa: E402  (the same file format)

ARENAS = ("_flat_p", "_flat_g", "_flat_m", "_flat_v", "_flat_p16", "_flat_slow", "_stats")


def dump(src, out):
    src = os.path.abspath(src)
    sys.path[:0] = [src, os.path.join(src, "tests")]
    import torch
    import _adamw_ref as A
    from vln_hamt_amd import optim
    assert os.path.abspath(optim.__file__).startswith(src + os.sep), optim.__file__
    dev, pc, arrays = "cuda", A.py_case(), {}
    classes = {"AdamW": lambda g: optim.AdamW(g, lr=1e-3, betas=A.PY_BETAS, eps=A.PY_EPS), "Ralamb": lambda g: optim.Ralamb(g, lr=1e-3),
               "RangerLars": lambda g: optim.RangerLars(g, alpha=0.5, k=2, lr=1e-3), "TorchAdamW": lambda g: optim.TorchAdamW(g, lr=1e-3),
               "TorchAdam": lambda g: optim.TorchAdam(g, lr=1e-3), "TorchRMSprop": lambda g: optim.TorchRMSprop(g, lr=1e-3),
               "TorchSGD": lambda g: optim.TorchSGD(g, lr=1e-3)}

    def put(name, t):
        a = np.ascontiguousarray(t.detach().cpu().reshape(-1).view(torch.uint8).numpy() if torch.is_tensor(t) else t)
        assert name not in arrays, name
        arrays[name] = [str(t.dtype), list(t.shape), hashlib.sha256(a.tobytes()).hexdigest()]

    def make(name, init, tag):
        params = [torch.nn.Parameter(t) for t in init]
        opt = classes[name]([{"params": [p for p, g in zip(params, A.PY_GROUP) if g == k], "weight_decay": A.PY_WD[k]} for k in (0, 1)])
        inner, calls = opt.host_table, [0]

        def host_table(*a, **kw):
            h = inner(*a, **kw)
            calls[0] += 1
            put(f"{tag}/host_table{calls[0]}", h)
            return h
        opt.host_table = host_table
        return params, opt

    def backward(params, s):
        for p, g in zip(params, pc["grads"][s]):
            p.grad = None if g is None else torch.from_numpy(g).to(dev)

    def structure(tag, x):
        """the tensors of a state_dict as arrays of their own; what is left, with the tensors' places marked, as one hashed string"""
        if torch.is_tensor(x):
            put(tag, x)
            return "tensor"
        if isinstance(x, dict):
            return {repr(k): structure(f"{tag}/{k}", v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [structure(f"{tag}/{i}", v) for i, v in enumerate(x)]
        return repr(x)

    for name in classes:
        for mode in ("eager", "staged", "dropped"):
            tag = f"{name}/{mode}"
            params, opt = make(name, [torch.from_numpy(a.copy()).to(dev) for a in pc["init"]], tag)
            for s in range(5):
                for k, grp in enumerate(opt.param_groups):
                    grp["lr"] = A.PY_LR[s][k]
                backward(params, s)
                if mode == "staged":
                    opt._pack_grads()
                    opt.prepare_step()
                    opt._pending_clip = (opt.global_grad_sumsq(), A.PY_MAX_NORM)
                    opt.launch_step()
                    opt.mark_updated()
                else:
                    optim.clip_grad_norm_(params, A.PY_MAX_NORM, optimizer=opt)
                    opt.step()
                opt.zero_grad()
                if mode == "dropped" and s == 1:
                    backward(params, 2)
                    optim.clip_grad_norm_(params, A.PY_MAX_NORM, optimizer=opt)
                    opt.zero_grad()
                if s == 2:
                    sd = copy.deepcopy(opt.state_dict())
                    params, opt = make(name, [p.detach().clone() for p in params], tag + "/resumed")
                    opt.load_state_dict(sd)
                torch.cuda.synchronize()
                put(f"{tag}/step{s + 1}/_steps", opt._steps)
                for k in ARENAS:
                    if getattr(opt, k, None) is not None:
                        put(f"{tag}/step{s + 1}/{k}", getattr(opt, k))
            rest = json.dumps(structure(f"{tag}/state_dict", opt.state_dict()), sort_keys=True)
            arrays[f"{tag}/state_dict"] = ["structure", [len(rest)], hashlib.sha256(rest.encode()).hexdigest()]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(arrays, f, indent=0)
    print(f"optim_class_dump: {len(arrays)} arrays from {os.path.dirname(optim.__file__)} -> {out}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--src")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.report))
    dump(a.src, a.out)
