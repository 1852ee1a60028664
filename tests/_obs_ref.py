"""A numpy restatement of csrc/obs.hip (what include/hamt.h says of hamt_obs_gather / hamt_obs_turn), serial:
tests/test_obs_ref.py holds it to the reference's own functions (tests/golden/obs_tiny.npz, tools/gen_obs_golden.py), the GPU tests use
it for the shapes the golden does not hold.  `mutate` names one deliberate error; the CPU test shows that each changes the result on
the golden's inputs, i.e. that the golden's cases can tell them apart."""
import numpy as np

VIEWS = 36
TABLES = ("feat", "ang36", "cand_cnt", "cand_point", "cand_node", "cand_ang", "vp_base", "scan_n")
MUTATIONS = ("view_not_mod12", "rest_descending", "shared_removed_per_candidate", "stop_nonzero", "stale_padding", "vp_base_ignored",
             "turn_on_stop")
OUTPUTS = ("ob_img", "ob_ang", "ob_nav", "ob_mask", "ob_len", "cand_len", "cand_nodes", "cand_points", "hist_img", "hist_pano_img", "hist_pano_ang")


def golden_tables(store):
    return {k: store["table/" + k] for k in TABLES}


def gather_ref(tab, ep_scan, cur, view, W, layout="pano", mutate=None, stale=None):
    """-> ({name: array} for OUTPUTS, anomalies).  `stale` (with mutate='stale_padding'): the outputs of the step before, which the
    padding slots then keep."""
    feat, ang36, C = tab["feat"], tab["ang36"], tab["cand_point"].shape[1]
    B, F, A = len(cur), feat.shape[2], ang36.shape[2]
    o = {"ob_img": np.zeros((B, W, F), np.float32), "ob_ang": np.zeros((B, W, A), np.float32), "ob_nav": np.zeros((B, W), np.int64),
         "ob_mask": np.zeros((B, W), np.uint8), "ob_len": np.zeros(B, np.int32), "cand_len": np.zeros(B, np.int32),
         "cand_nodes": np.full((B, W), -1, np.int32), "cand_points": np.full((B, W), -1, np.int32), "hist_img": np.zeros((B, F), np.float32),
         "hist_pano_img": np.zeros((B, VIEWS, F), np.float32), "hist_pano_ang": np.zeros((B, VIEWS, A), np.float32)}
    if mutate == "stale_padding" and stale is not None:
        for k in ("ob_img", "ob_ang", "ob_nav"):
            o[k][:, :min(W, stale[k].shape[1])] = stale[k][:, :W]
    anomalies = 0
    for b in range(B):
        s, here, vw = int(ep_scan[b]), int(cur[b]), int(view[b])
        if not (0 <= here < tab["scan_n"][s] and 0 <= vw < VIEWS):
            anomalies += 1
            for k in ("ob_img", "ob_ang", "ob_nav"):
                o[k][b] = 0
            o["ob_nav"][b, 0], o["ob_mask"][b, 0], o["ob_len"][b], o["cand_len"][b] = 2, 1, 1, 1
            continue
        row = (0 if mutate == "vp_base_ignored" else int(tab["vp_base"][s])) + here
        n = min(max(int(tab["cand_cnt"][row]), 0), C, W - 1)
        free = list(range(VIEWS))
        for c in range(n):
            p = min(max(int(tab["cand_point"][row, c]), 0), VIEWS - 1)
            o["ob_img"][b, c] = feat[row, p]
            if mutate == "view_not_mod12":                   # (the flat read a kernel would make: into the next candidate's block)
                flat = tab["cand_ang"].reshape(-1, A)
                o["ob_ang"][b, c] = flat[min((row * C + c) * 12 + vw, len(flat) - 1)]
            else:
                o["ob_ang"][b, c] = tab["cand_ang"][row, c, vw % 12]
            o["ob_nav"][b, c] = 1
            o["cand_nodes"][b, c], o["cand_points"][b, c] = tab["cand_node"][row, c], p
            if p in free:
                free.remove(p)
            elif mutate == "shared_removed_per_candidate" and free:
                free.pop(0)                                  # (a view counted once per candidate that points to it)
        o["ob_img"][b, n], o["ob_ang"][b, n], o["ob_nav"][b, n] = (1.0 if mutate == "stop_nonzero" else 0.0), 0.0, 2
        if layout != "pano":
            free = []
        if mutate == "rest_descending":
            free = free[::-1]
        length = min(n + 1 + len(free), W)
        for k, v in enumerate(free[:length - n - 1]):
            o["ob_img"][b, n + 1 + k], o["ob_ang"][b, n + 1 + k], o["ob_nav"][b, n + 1 + k] = feat[row, v], ang36[vw, v], 0
        if not (mutate == "stale_padding" and stale is not None):
            for k in ("ob_img", "ob_ang", "ob_nav"):
                o[k][b, length:] = 0
        o["ob_mask"][b, :length] = 1
        o["ob_len"][b], o["cand_len"][b] = length, n + 1
        o["hist_img"][b], o["hist_pano_img"][b], o["hist_pano_ang"][b] = feat[row, vw], feat[row], ang36[vw]
    return o, anomalies


def turn_ref(cand_points, env_action, view, mutate=None):
    """-> the views after the step"""
    out = np.array(view, np.int32)
    W = cand_points.shape[1]
    for b, a in enumerate(env_action):
        a = int(a)
        if mutate == "turn_on_stop" and a == -1:
            out[b] = cand_points[b, a]                       # (numpy's reading of index -1: the last slot, whatever it holds)
            continue
        if 0 <= a < W and 0 <= cand_points[b, a] < VIEWS:
            out[b] = cand_points[b, a]
    return out


def random_tables(seed, scan_n=(5, 3), F=16, A=4, C=5):
    """a small synthetic store: every candidate count from 0 to C occurs, shared views included"""
    rng = np.random.Generator(np.random.PCG64(seed))
    scan_n = np.asarray(scan_n, np.int32)
    NV = int(scan_n.sum())
    cnt = (np.arange(NV) % (C + 1)).astype(np.int32)
    point = np.full((NV, C), -1, np.int32)
    node = np.full((NV, C), -1, np.int32)
    bases = np.concatenate([[0], np.cumsum(scan_n)[:-1]])
    of_scan = np.repeat(np.arange(len(scan_n)), scan_n)
    for r in range(NV):
        point[r, :cnt[r]] = rng.integers(0, VIEWS, cnt[r]) if r % 2 else rng.integers(0, 3, cnt[r]) * 12    # (even rows: few views, shared)
        node[r, :cnt[r]] = rng.integers(0, scan_n[of_scan[r]], cnt[r])
    return {"feat": rng.standard_normal((NV, VIEWS, F)).astype(np.float32), "ang36": rng.standard_normal((VIEWS, VIEWS, A)).astype(np.float32),
            "cand_cnt": cnt, "cand_point": point, "cand_node": node, "cand_ang": rng.standard_normal((NV, C, 12, A)).astype(np.float32),
            "vp_base": bases.astype(np.int64), "scan_n": scan_n}


def max_ob_len(tab):
    return max(int(n) + 1 + VIEWS - len(set(int(p) for p in tab["cand_point"][r, :n])) for r, n in enumerate(tab["cand_cnt"]))
