#!/usr/bin/env python3
"""Generate tests/golden/obj_obs_tiny.npz: REVERIE's object observations of a scripted walk, built by the REFERENCE's own functions on
the CPU.

Test infrastructure, like tools/gen_obs_golden.py and tools/gen_reverie_golden.py (needs the reference checkout, oracle.ref_shim.REF):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_obj_obs_golden.py

The reference is imported through oracle.ref_shim with empty stand-in modules for what is not installed here (MatterSim, jsonlines, h5py,
none of which the functions below touch).  Per step of the walk:
  ReverieNavRefBatch._get_obs (finetune_src/reverie/env.py:181-215)   its OWN object block, on an instance made with __new__; the base
                                                                      class's _get_obs, which it calls first, is replaced by the
                                                                      scripted list of {scan, viewpoint, viewIndex, instr_id} (plus
                                                                      'teacher' and 'candidate', which _teacher_action reads);
  NavRefCMTAgent._object_variable (reverie/agent.py:125-139)          step/<t>/obj_feats, obj_angles, obj_poses, obj_lens
  NavRefCMTAgent._teacher_action (:141-165)                           step/<t>/target, ref_target
The tables (`table/...`) are the store a device would hold: CSR over the rows of tests/golden/r2r_tiny (scanA, scanB), the positions by
the reference's own get_obj_local_pos (reverie/data_utils.py:25-31) stored into float32 as _object_variable stores them; `untrunc/...`
is the same without the cut to max_objects (what a store that forgot it would hold), `db/...` the database itself.

The database (seeded, Fo = 16, A = 4, max_objects = 3): objects per viewpoint a00 1, a01 3, a02 5 (cut to 3), a03 absent, a04 2, a05 3,
a06 1, b00 2, b01 3, b02 4, b03 absent, b04 1; `bboxes` int64 at every other key and float32 at the rest; `viewindexs` from all 36
views.  The walk (B = 6, T = 4; three episodes per scan): step 0 has objects for every episode (the batch is as wide as the store),
step 2 at most two per episode (narrower); episode 0 stops at step 1 on its goal (slot 0) and is gathered on as an ended episode with
stale rows behind it; 1 stops at step 3 on slot 2; 2 stops at step 3 where its goal is among the objects cut off; 3 has no goal object
(objId None); 4 stops at step 3 on slot 1; 5 stops at step 2 on a viewpoint without objects.
"""
import json
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import ref_shim                                                  # noqa: E402
from vln_hamt_amd.agent.nav_graph import NavGraphs                           # noqa: E402
from vln_hamt_amd.data.r2r_data import _view_angles, angle_feature           # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NAME = "obj_obs_tiny.npz"
TINY = os.path.join(OUT, "r2r_tiny")
FO, A, MAX_OBJECTS, SEED, IGNOREID, OB_IMG_MAX_LEN = 16, 4, 3, 29, -100, 7
COUNTS = {"scanA_a00": 1, "scanA_a01": 3, "scanA_a02": 5, "scanA_a04": 2, "scanA_a05": 3, "scanA_a06": 1,
          "scanB_b00": 2, "scanB_b01": 3, "scanB_b02": 4, "scanB_b04": 1}                      # a03 and b03: not in the database
SCAN_OF = ["scanA", "scanA", "scanA", "scanB", "scanB", "scanB"]
WALK = [["a01", "a02", "a00", "b01", "b02", "b00"],                                           # step: the viewpoint of each episode
        ["a00", "a03", "a02", "b04", "b03", "b02"],
        ["a00", "a04", "a06", "b04", "b04", "b03"],
        ["a00", "a05", "a02", "b04", "b01", "b03"]]
VIEWS = [[3, 12, 35, 0, 23, 11], [14, 7, 24, 30, 2, 19], [14, 33, 5, 30, 13, 8], [14, 0, 17, 30, 26, 8]]
STOP_AT = {0: 1, 1: 3, 2: 3, 3: 1, 4: 3, 5: 2}                                                # episode: the step at which the teacher stops
GOAL = {0: ("scanA_a00", 0), 1: ("scanA_a05", 2), 2: ("scanA_a02", 4), 3: None, 4: ("scanB_b01", 1), 5: ("scanB_b02", 0)}   # (viewpoint, object) or None


def import_ref():
    if not hasattr(np, "bool"):
        np.bool = np.bool_
    for name in ("MatterSim", "jsonlines", "h5py"):
        sys.modules.setdefault(name, types.ModuleType(name))
    try:
        import networkx  # noqa: F401
    except ImportError:
        sys.modules["networkx"] = types.ModuleType("networkx")
    for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.") or k == "r2r" or k.startswith("r2r.")]:
        del sys.modules[k]
    return ref_shim._import_pkg("finetune_src", "reverie", ["env", "agent", "data_utils"])


def angle_table():
    """36 x [36, A]: the reference's table in its `minus_elevation` form (r2r/data_utils.py:139-167), in which the base view's elevation
    counts as well as its heading -- in the default form row v equals row v % 12, and a view index reduced mod 12 would go unseen"""
    step = math.radians(30)
    return [np.stack([angle_feature(h - (base % 12) * step, e - (base // 12 - 1) * step, A) for h, e in _view_angles()], 0).astype(np.float32)
            for base in range(36)]


def database():
    """the object database in the form reverie/data_utils.py::load_obj_database returns"""
    rng = np.random.Generator(np.random.PCG64(SEED))
    db, next_id = {}, {"scanA": 100, "scanB": 500}
    for i, (key, n) in enumerate(COUNTS.items()):
        scan = key.split("_")[0]
        xy = rng.integers(0, 400, (n, 2))
        wh = rng.integers(8, 200, (n, 2))
        boxes = np.concatenate([xy, wh], 1)
        boxes = boxes.astype(np.int64) if i % 2 == 0 else (boxes + rng.random((n, 4))).astype(np.float32)
        db[key] = {"obj_ids": [str(next_id[scan] + 3 * j) for j in range(n)], "fts": rng.standard_normal((n, FO)).astype(np.float32),
                   "bboxes": boxes, "viewindexs": rng.integers(0, 36, n).astype(np.int64)}
        next_id[scan] += 3 * n + 1
    db["scanA_a02"]["viewindexs"][:3] = [0, 12, 35]
    db["scanB_b01"]["viewindexs"][:3] = [11, 24, 13]
    return db


def tables(graphs, db, du, limit):
    """the CSR store over the graphs' rows, the first `limit` objects of a viewpoint kept; positions by the reference's get_obj_local_pos"""
    off, feat, view, pos, ids, box = [0], [], [], [], [], []
    for scan in graphs.scans:
        for vp in graphs.nodes[scan]:
            e = db.get(f"{scan}_{vp}")
            n = 0 if e is None else min(len(e["obj_ids"]), limit)
            if n:
                local = np.zeros((n, 5), np.float32)
                local[:] = du.get_obj_local_pos(e["bboxes"])[:n]                       # (as agent.py:134 stores them: into a float32 array)
                feat.append(e["fts"][:n]); view.append(e["viewindexs"][:n].astype(np.int32)); pos.append(local)
                ids.append(np.array([int(x) for x in e["obj_ids"][:n]], np.int32)); box.append(e["bboxes"][:n].astype(np.float64))
            off.append(off[-1] + n)
    return {"obj_off": np.array(off, np.int64), "obj_feat": np.concatenate(feat), "obj_view": np.concatenate(view), "obj_pos": np.concatenate(pos),
            "obj_id": np.concatenate(ids), "obj_box": np.concatenate(box)}


def generate():
    env_mod, agent_mod, du = import_ref()
    graphs = NavGraphs(TINY)
    db = database()
    with open(os.path.join(TINY, "scanvp_cands.json")) as f:
        neighbours = {k: list(v) for k, v in json.load(f).items()}
    table = angle_table()
    B, T = len(SCAN_OF), len(WALK)
    goal_ids = [None if GOAL[b] is None else int(db[GOAL[b][0]]["obj_ids"][GOAL[b][1]]) for b in range(B)]

    store = {"meta/scans": np.array(graphs.scans), "meta/Fo": np.array(FO), "meta/A": np.array(A), "meta/max_objects": np.array(MAX_OBJECTS),
             "meta/seed": np.array(SEED), "meta/ignoreid": np.array(IGNOREID), "meta/ob_img_max_len": np.array(OB_IMG_MAX_LEN),
             "meta/db_keys": np.array(list(db))}
    for key, e in db.items():
        store.update({f"db/{key}/obj_ids": np.array(e["obj_ids"]), f"db/{key}/fts": e["fts"], f"db/{key}/bboxes": e["bboxes"],
                      f"db/{key}/viewindexs": e["viewindexs"]})
    scan_n = np.asarray(graphs.scan_n_host, np.int32)
    shared = {"ang36": np.stack(table, 0), "scan_n": scan_n,
              "vp_base": np.concatenate([[0], np.cumsum(scan_n.astype(np.int64))[:-1]]).astype(np.int64)}
    tab = tables(graphs, db, du, MAX_OBJECTS)
    store.update({"table/" + k: v for k, v in {**tab, **shared}.items()})
    store.update({"untrunc/" + k: v for k, v in tables(graphs, db, du, 10 ** 6).items()})

    # ---- the reference's environment and agent, as far as the three functions read them
    items = [{"id": f"ep{b}", "objId": goal_ids[b], "instr_id": f"ep{b}_{goal_ids[b]}_0", "scan": SCAN_OF[b], "path": [WALK[0][b]]} for b in range(B)]
    env = env_mod.ReverieNavRefBatch.__new__(env_mod.ReverieNavRefBatch)
    env.angle_feature, env.obj_db, env.max_objects, env.batch = table, db, MAX_OBJECTS, items
    env.gt_trajs = {it["instr_id"]: (it["scan"], it["path"], it["objId"]) for it in items}
    env.obj2viewpoint = {f"{it['scan']}_{it['objId']}": [it["path"][0]] for it in items if it["objId"] is not None}
    env.shortest_distances = {s: {a: {b_: 0.0 for b_ in graphs.nodes[s]} for a in graphs.nodes[s]} for s in graphs.scans}
    agent = types.SimpleNamespace(args=types.SimpleNamespace(obj_feat_size=FO, angle_feat_size=A, ignoreid=IGNOREID))
    script = {}
    real_get_obs = env_mod.R2RBatch._get_obs
    env_mod.R2RBatch._get_obs = lambda self, t=None, shortest_teacher=False: [dict(o) for o in script["obs"]]

    w = {"scan": np.array([graphs.scan_index[s] for s in SCAN_OF], np.int32), "cur": np.zeros((T, B), np.int32), "view": np.array(VIEWS, np.int32),
         "ended": np.zeros((T, B), bool), "teacher_stop": np.zeros((T, B), bool), "goal": np.array([-1 if g is None else g for g in goal_ids], np.int32)}
    try:
        with ref_shim.cuda_is_identity():
            for t in range(T):
                script["obs"] = []
                for b in range(B):
                    scan, vp = SCAN_OF[b], WALK[t][b]
                    stop, ended = STOP_AT[b] == t, STOP_AT[b] < t
                    teacher = vp if (stop or ended) else WALK[t + 1][b]
                    assert teacher == vp or teacher in neighbours[f"{scan}_{vp}"], (t, b)
                    script["obs"].append({"scan": scan, "viewpoint": vp, "viewIndex": VIEWS[t][b], "instr_id": items[b]["instr_id"], "teacher": teacher,
                                          "candidate": [{"viewpointId": v} for v in neighbours[f"{scan}_{vp}"]]})
                    w["cur"][t, b], w["ended"][t, b], w["teacher_stop"][t, b] = graphs.node_id(scan, vp), ended, stop
                obs = env._get_obs()
                feats, angles, poses, lens = agent_mod.NavRefCMTAgent._object_variable(agent, obs)
                a, ref = agent_mod.NavRefCMTAgent._teacher_action(agent, obs, w["ended"][t], OB_IMG_MAX_LEN)
                O = feats.shape[1]
                ids = np.full((B, O), -1, np.int32)
                true_len = np.zeros(B, np.int32)
                for b, ob in enumerate(obs):
                    kept = [int(x) for x in ob["candidate_obj"][2]]
                    ids[b, :len(kept)], true_len[b] = kept, len(kept)
                    assert ob["objId"] == str(goal_ids[b])
                store.update({f"step/{t}/obj_feats": feats.numpy(), f"step/{t}/obj_angles": angles.numpy(), f"step/{t}/obj_poses": poses.numpy(),
                              f"step/{t}/obj_lens": np.array(lens, np.int32), f"step/{t}/true_len": true_len, f"step/{t}/obj_ids": ids,
                              f"step/{t}/target": a.numpy(), f"step/{t}/ref_target": ref.numpy()})
    finally:
        env_mod.R2RBatch._get_obs = real_get_obs
    store.update({"walk/" + k: v for k, v in w.items()})

    # ---- what the cases must contain
    widths = [store[f"step/{t}/obj_feats"].shape[1] for t in range(T)]
    lens = np.stack([store[f"step/{t}/true_len"] for t in range(T)])
    assert widths[0] == MAX_OBJECTS and lens[0].min() >= 1 and min(widths) < MAX_OBJECTS, (widths, lens)
    assert {0, 1, MAX_OBJECTS} <= set(lens.ravel().tolist())
    seen = w["view"][lens > 0]
    assert (seen < 12).any() and (seen >= 12).any()
    refs = np.stack([store[f"step/{t}/ref_target"] for t in range(T)])
    assert {0, 1, 2, IGNOREID} <= set(refs.ravel().tolist()) and refs[3, 2] == IGNOREID and refs[2, 5] == IGNOREID, refs
    assert {str(tab_box.dtype) for tab_box in (e["bboxes"] for e in db.values())} == {"int64", "float32"}
    assert not np.array_equal(shared["ang36"][12:], np.concatenate([shared["ang36"][:12]] * 2))
    views = np.concatenate([e["viewindexs"] for e in db.values()])
    assert (views < 12).any() and (views >= 12).any()
    return store


def main():
    store = generate()
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME), **store)
    print(f"{NAME}: {len(store)} arrays, {os.path.getsize(os.path.join(OUT, NAME))} bytes")


if __name__ == "__main__":
    main()
