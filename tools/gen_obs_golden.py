#!/usr/bin/env python3
"""Generate tests/golden/obs_tiny.npz: the observations of a scripted walk, built by the REFERENCE's own functions on the CPU.

Test infrastructure, like tools/gen_reverie_golden.py (needs the reference checkout, oracle.ref_shim.REF):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_obs_golden.py

The reference is imported through oracle.ref_shim with empty stand-in modules for what this machine lacks (MatterSim, jsonlines, h5py,
none of which the four functions below touch).  Per step of the walk, with `buffered_state_dict` pre-filled, on namespace objects:
  R2RBatch.make_candidate (finetune_src/r2r/env.py:182-252, its cached branch)  the candidates of each episode's viewpoint and view;
  Seq2SeqCMTAgent._cand_pano_feature_variable (agent_cmt.py:104-151)            pano/<t>/...
  Seq2SeqCMTAgent._candidate_variable (:153-171)                                cand/<t>/...
  Seq2SeqCMTAgent._history_variable (:173-190)                                  hist/<t>/...
An observation's 'feature' is the viewpoint's image features next to the angle table of the view looked at, as env.py::_get_obs joins
them (:282); a move puts the episode on the chosen candidate's viewpoint, looking at its pointId (agent_cmt.py::make_equiv_action).

The table (F = 16, A = 4): tests/golden/r2r_tiny (scanA, scanB; scanvp_cands.json converted by ObsStore.candidates_from_scanvp) plus a
synthetic third scan `scanS` of 9 viewpoints for what the tiny set lacks: s00 without a candidate, s01 with two and s02 with three
candidates on one view, s03 with C = 7 candidates (views 0, 11, 12, 23, 24, 35 and 11 again).  `table/cand_ang` is the reference's own
make_candidate for each of the 12 base headings; `table/cand_nh` / `table/cand_el` keep the doubles it was computed from.
The walk (B = 6, T = 6): two episodes on scanA's a00 looking at views 0 and 11, one in scanB from view 12, three in scanS from views
35, 23 and 24 -- the last on s00, which can only stop; episode 0 stops at step 3 and is gathered on as an ended episode; episode 3 is
scripted through the shared-view viewpoints, the others draw their moves.
"""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import ref_shim                                                  # noqa: E402
from vln_hamt_amd.agent.obs import ObsStore                                  # noqa: E402
from vln_hamt_amd.data.r2r_data import get_all_point_angle_feature           # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NAME = "obs_tiny.npz"
TINY = os.path.join(OUT, "r2r_tiny")
F, A, T, SEED = 16, 4, 6, 23
SCANS = ("scanA", "scanB", "scanS")
S_NODES = ["s%02d" % i for i in range(9)]
S_CANDS = {"s00": [], "s01": [("s02", 35), ("s03", 35), ("s04", 5)], "s02": [("s01", 12), ("s03", 12), ("s04", 12)],
           "s03": [("s01", 0), ("s02", 11), ("s04", 12), ("s05", 23), ("s06", 24), ("s07", 35), ("s08", 11)],
           "s04": [("s03", 7)], "s05": [("s03", 19)], "s06": [("s03", 30)], "s07": [("s03", 1)], "s08": [("s03", 17), ("s01", 17)]}
STARTS = [("scanA", "a00", 0), ("scanA", "a00", 11), ("scanB", "b00", 12), ("scanS", "s01", 35), ("scanS", "s03", 23), ("scanS", "s00", 24)]
STOP_AT = {0: 3}                                  # episode: the step at which it stops
FORCED = {(3, 0): 0, (3, 1): 1, (3, 2): 0, (3, 3): 1, (3, 4): 1}     # (episode, step): slot -- s01 -> s02 -> s03 -> s01 -> s03 -> s02; the rest is drawn


def import_ref():
    if not hasattr(np, "bool"):
        np.bool = np.bool_                        # (numpy >= 1.24 dropped the alias agent_cmt.py:113 uses)
    for name in ("MatterSim", "jsonlines", "h5py"):
        sys.modules.setdefault(name, types.ModuleType(name))
    try:
        import networkx  # noqa: F401
    except ImportError:
        sys.modules["networkx"] = types.ModuleType("networkx")
    for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        del sys.modules[k]
    return ref_shim._import_pkg("finetune_src", "r2r", ["env", "agent_cmt"])


def world():
    """-> (nodes per scan, candidates in buffered_state_dict form, features {scan_vp: [36, F] float32})"""
    rng = np.random.Generator(np.random.PCG64(SEED))
    nodes, feats = {}, {}
    with open(os.path.join(TINY, "scanvp_cands.json")) as f:
        cands = ObsStore.candidates_from_scanvp(json.load(f))
    img = np.load(os.path.join(TINY, "img_fts.npz"))
    for scan in SCANS[:2]:
        with open(os.path.join(TINY, f"{scan}_connectivity.json")) as f:
            nodes[scan] = [nd["image_id"] for nd in json.load(f) if nd["included"]]
        for vp in nodes[scan]:
            feats[f"{scan}_{vp}"] = np.asarray(img[f"{scan}_{vp}"])[:, :F].astype(np.float32)
    nodes["scanS"] = S_NODES
    for vp in S_NODES:
        feats[f"scanS_{vp}"] = rng.standard_normal((36, F)).astype(np.float32)
        cands[f"scanS_{vp}"] = [{"normalized_heading": float(rng.uniform(0, 2 * np.pi)), "elevation": float(rng.uniform(-0.6, 0.6)), "scanId": "scanS",
                                 "viewpointId": to, "pointId": p, "idx": j + 1} for j, (to, p) in enumerate(S_CANDS[vp])]
    return nodes, cands, feats


def generate():
    env_mod, agent_mod = import_ref()
    nodes, cands, feats = world()
    index = {s: {vp: i for i, vp in enumerate(nodes[s])} for s in SCANS}
    scan_n = np.array([len(nodes[s]) for s in SCANS], np.int32)
    vp_base = np.concatenate([[0], np.cumsum(scan_n.astype(np.int64))[:-1]]).astype(np.int64)
    NV, C = int(scan_n.sum()), max(len(v) for v in cands.values())
    angle_table = get_all_point_angle_feature(A)
    env = types.SimpleNamespace(buffered_state_dict={k: [dict(c) for c in v] for k, v in cands.items()}, angle_feat_size=A, sim=None)
    agent = types.SimpleNamespace(args=types.SimpleNamespace(views=36, image_feat_size=F, angle_feat_size=A, hist_enc_pano=True))
    make_candidate = lambda scan, vp, view: env_mod.R2RBatch.make_candidate(env, feats[f"{scan}_{vp}"], scan, vp, view)

    # ---- the table: the reference's candidates for each base heading
    store = {"meta/scans": np.array(SCANS), "meta/F": np.array(F), "meta/A": np.array(A), "meta/seed": np.array(SEED)}
    tab = {"feat": np.zeros((NV, 36, F), np.float32), "ang36": np.stack(angle_table, 0), "cand_cnt": np.zeros(NV, np.int32),
           "cand_point": np.full((NV, C), -1, np.int32), "cand_node": np.full((NV, C), -1, np.int32), "cand_ang": np.zeros((NV, C, 12, A), np.float32),
           "vp_base": vp_base, "scan_n": scan_n, "cand_nh": np.zeros((NV, C)), "cand_el": np.zeros((NV, C))}
    for si, scan in enumerate(SCANS):
        for li, vp in enumerate(nodes[scan]):
            row = int(vp_base[si]) + li
            tab["feat"][row] = feats[f"{scan}_{vp}"]
            tab["cand_cnt"][row] = len(cands[f"{scan}_{vp}"])
            for h in range(12):
                for c, cc in enumerate(make_candidate(scan, vp, h)):
                    assert np.array_equal(cc["feature"][:F], feats[f"{scan}_{vp}"][cc["pointId"]])
                    tab["cand_point"][row, c], tab["cand_node"][row, c] = cc["pointId"], index[scan][cc["viewpointId"]]
                    tab["cand_ang"][row, c, h] = cc["feature"][F:]
            for c, cc in enumerate(cands[f"{scan}_{vp}"]):
                tab["cand_nh"][row, c], tab["cand_el"][row, c] = cc["normalized_heading"], cc["elevation"]
    store.update({"table/" + k: v for k, v in tab.items()})

    # ---- the walk
    rng = np.random.Generator(np.random.PCG64(SEED + 1))
    B = len(STARTS)
    scan = [s for s, _, _ in STARTS]
    cur, view, ended = [vp for _, vp, _ in STARTS], [v for _, _, v in STARTS], [False] * B
    w = {"scan": np.array([SCANS.index(s) for s in scan], np.int32), "cur": np.zeros((T, B), np.int32), "view": np.zeros((T + 1, B), np.int32),
         "env_action": np.zeros((T, B), np.int32), "ended": np.zeros((T, B), bool), "cand_node": np.full((T, B, C), -1, np.int32),
         "cand_point": np.full((T, B, C), -1, np.int32)}
    w["view"][0] = view
    with ref_shim.cuda_is_identity():
        for t in range(T):
            obs = []
            for b in range(B):
                base = feats[f"{scan[b]}_{cur[b]}"]
                obs.append({"candidate": make_candidate(scan[b], cur[b], view[b]), "viewIndex": view[b], "viewpoint": cur[b], "scan": scan[b],
                            "feature": np.concatenate((base, angle_table[view[b]]), -1)})
                w["cur"][t, b], w["ended"][t, b] = index[scan[b]][cur[b]], ended[b]
                for c, cc in enumerate(obs[-1]["candidate"]):
                    w["cand_node"][t, b, c], w["cand_point"][t, b, c] = index[scan[b]][cc["viewpointId"]], cc["pointId"]
            img, ang, nav, lens, cand_lens = agent_mod.Seq2SeqCMTAgent._cand_pano_feature_variable(agent, obs)
            store.update({f"pano/{t}/ob_img": img.numpy(), f"pano/{t}/ob_ang": ang.numpy(), f"pano/{t}/ob_nav": nav.numpy().astype(np.int64),
                          f"pano/{t}/ob_len": np.array(lens, np.int32), f"pano/{t}/cand_len": np.array(cand_lens, np.int32)})
            img, ang, nav, cand_lens = agent_mod.Seq2SeqCMTAgent._candidate_variable(agent, obs)
            store.update({f"cand/{t}/ob_img": img.numpy(), f"cand/{t}/ob_ang": ang.numpy(), f"cand/{t}/ob_nav": nav.numpy().astype(np.int64),
                          f"cand/{t}/cand_len": np.array(cand_lens, np.int32)})
            h_img, h_pimg, h_pang = agent_mod.Seq2SeqCMTAgent._history_variable(agent, obs)
            store.update({f"hist/{t}/hist_img": h_img.numpy(), f"hist/{t}/hist_pano_img": h_pimg.numpy(), f"hist/{t}/hist_pano_ang": h_pang.numpy()})
            for b in range(B):
                n = len(obs[b]["candidate"])
                a = -1 if (ended[b] or n == 0 or STOP_AT.get(b) == t) else int(rng.integers(0, n))
                a = FORCED.get((b, t), a)
                w["env_action"][t, b] = a
                if a < 0:
                    ended[b] = True
                else:
                    cur[b], view[b] = obs[b]["candidate"][a]["viewpointId"], obs[b]["candidate"][a]["pointId"]
            w["view"][t + 1] = view
    store.update({"walk/" + k: v for k, v in w.items()})

    # ---- what the cases must contain
    cnt_seen = {int(tab["cand_cnt"][vp_base[s] + c]) for s, c in zip(np.repeat(w["scan"][None], T, 0).ravel(), w["cur"].ravel())}
    assert {0, C} <= cnt_seen, cnt_seen
    rows = {(int(s), int(c)) for s, c in zip(np.repeat(w["scan"][None], T, 0).ravel(), w["cur"].ravel())}
    assert {(2, 1), (2, 2)} <= rows, rows                                   # s01 and s02: two / three candidates on one view
    assert {0, 11, 12, 35} <= set(w["view"].ravel().tolist()) and {v // 12 for v in w["view"].ravel().tolist()} == {0, 1, 2}, w["view"]
    assert w["ended"][:, 0].any() and len(set(w["scan"].tolist())) == 3
    return store


def main():
    store = generate()
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME), **store)
    print(f"{NAME}: {len(store)} arrays, {os.path.getsize(os.path.join(OUT, NAME))} bytes")


if __name__ == "__main__":
    main()
