"""A numpy restatement of csrc/obs.hip's object gather (what include/hamt.h says of hamt_obj_gather), serial: tests/test_obj_obs_ref.py
holds it to the reference's own functions (tests/golden/obj_obs_tiny.npz, tools/gen_obj_obs_golden.py), the GPU tests use it for the
shapes the golden does not hold.  `mutate` names one deliberate error; the CPU test shows that each changes the result on the golden's
inputs, i.e. that the golden's cases can tell them apart."""
import numpy as np

VIEWS = 36
OBJ_TABLES = ("obj_off", "obj_feat", "obj_view", "obj_pos", "obj_id")
SHARED = ("ang36", "vp_base", "scan_n")
MUTATIONS = ("view_mod12", "angle_transposed", "no_truncation", "empty_unmasked", "len_padded", "stale_padding", "vp_base_ignored", "x2_is_w",
             "area_unnormalised", "ids_by_slot")
OUTPUTS = ("obj_feats", "obj_angles", "obj_poses", "obj_masks", "obj_lens", "obj_ids")


def golden_obj_tables(store):
    """the golden's store; 'obj_box' (the raw boxes, fp64) and 'untruncated' (the store without the cut to max_objects) serve the
    mutations only"""
    tab = {k: store["table/" + k] for k in OBJ_TABLES + SHARED + ("obj_box",)}
    tab["untruncated"] = {k: store["untrunc/" + k] for k in OBJ_TABLES + ("obj_box",)}
    return tab


def obj_gather_ref(tab, ep_scan, cur, view, Ow, mutate=None, stale=None):
    """-> ({name: array} for OUTPUTS, anomalies).  `stale` (with mutate='stale_padding'): the outputs of the step before, which the
    padding slots then keep."""
    src = tab["untruncated"] if mutate == "no_truncation" else tab
    off, feat, oview, pos, oid = (src[k] for k in OBJ_TABLES)
    ang36 = tab["ang36"]
    B, Fo, A, S, NV = len(cur), feat.shape[1], ang36.shape[2], len(tab["scan_n"]), len(off) - 1
    o = {"obj_feats": np.zeros((B, Ow, Fo), np.float32), "obj_angles": np.zeros((B, Ow, A), np.float32), "obj_poses": np.zeros((B, Ow, 5), np.float32),
         "obj_masks": np.zeros((B, Ow), np.uint8), "obj_lens": np.zeros(B, np.int32), "obj_ids": np.full((B, Ow), -1, np.int32)}
    keep = mutate == "stale_padding" and stale is not None
    if keep:
        for k in ("obj_feats", "obj_angles", "obj_poses", "obj_ids"):
            w = min(Ow, stale[k].shape[1])
            o[k][:, :w] = stale[k][:, :w]
    anomalies = 0
    for b in range(B):
        s, here, vw = int(ep_scan[b]), int(cur[b]), int(view[b])
        row = ((0 if mutate == "vp_base_ignored" else int(tab["vp_base"][s])) + here) if 0 <= s < S else -1
        ok = 0 <= s < S and 0 <= here < tab["scan_n"][s] and 0 <= vw < VIEWS and 0 <= row < NV
        ok = ok and 0 <= off[row] <= off[row + 1] <= len(feat)
        if not ok:
            anomalies += 1
            for k in ("obj_feats", "obj_angles", "obj_poses"):
                o[k][b] = 0
            o["obj_ids"][b], o["obj_masks"][b, 0] = -1, 1
            continue
        first = int(off[row])
        n = min(int(off[row + 1]) - first, Ow)
        for k in range(n):
            j = first + k
            v = min(max(int(oview[j]), 0), VIEWS - 1)
            o["obj_feats"][b, k] = feat[j]
            o["obj_angles"][b, k] = ang36[v, vw] if mutate == "angle_transposed" else ang36[vw % 12 if mutate == "view_mod12" else vw, v]
            o["obj_poses"][b, k] = pos[j]
            if mutate in ("x2_is_w", "area_unnormalised"):
                x1, y1, w, h = src["obj_box"][j]
                o["obj_poses"][b, k, 2 if mutate == "x2_is_w" else 4] = w / 640 if mutate == "x2_is_w" else w * h
            o["obj_ids"][b, k] = k if mutate == "ids_by_slot" else oid[j]
        if not keep:
            for k in ("obj_feats", "obj_angles", "obj_poses"):
                o[k][b, n:] = 0
            o["obj_ids"][b, n:] = -1
        o["obj_masks"][b, :(n if mutate == "empty_unmasked" else max(n, 1))] = 1
        o["obj_lens"][b] = max(n, 1) if mutate == "len_padded" else n
    return o, anomalies


def positions(boxes):
    """[x1/640, y1/480, (x1+w)/640, (y1+h)/480, w*h/(640*480)] at the boxes' dtype, then fp32 (include/hamt.h: obj_pos)"""
    x1, y1, w, h = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    return np.stack([x1 / 640, y1 / 480, (x1 + w) / 640, (y1 + h) / 480, w * h / (640 * 480)], 1).astype(np.float32)


def random_obj_tables(seed, scan_n=(5, 3, 4), Fo=16, A=4, max_objects=5):
    """a small synthetic store: every count from 0 to max_objects occurs, object views from all 36"""
    rng = np.random.Generator(np.random.PCG64(seed))
    scan_n = np.asarray(scan_n, np.int32)
    NV = int(scan_n.sum())
    cnt = ((np.arange(NV) + 2) % (max_objects + 1)).astype(np.int64)
    assert set(cnt.tolist()) == set(range(max_objects + 1)), cnt
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    N = int(off[-1])
    box = np.concatenate([rng.integers(0, 400, (N, 2)), rng.integers(8, 200, (N, 2))], 1).astype(np.float64)
    return {"obj_off": off, "obj_feat": rng.standard_normal((N, Fo)).astype(np.float32), "obj_view": rng.integers(0, VIEWS, N).astype(np.int32),
            "obj_pos": positions(box), "obj_id": rng.permutation(N).astype(np.int32) + 40, "obj_box": box,
            "ang36": rng.standard_normal((VIEWS, VIEWS, A)).astype(np.float32), "scan_n": scan_n,
            "vp_base": np.concatenate([[0], np.cumsum(scan_n.astype(np.int64))[:-1]]).astype(np.int64)}
