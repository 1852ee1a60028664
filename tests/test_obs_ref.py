"""Not gpu: the numpy restatement of csrc/obs.hip (tests/_obs_ref.py) against the reference's own functions (tests/golden/obs_tiny.npz,
written by tools/gen_obs_golden.py), the host side of agent.ObsStore against the golden's table, the two new entry points in header,
binding and library, and the gather kernel's code object.  A pure gather: every comparison is bit for bit."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from _obs_ref import MUTATIONS, OUTPUTS, TABLES, VIEWS, gather_ref, golden_tables, max_ob_len, turn_ref
from _util import load_npz

T, B = 6, 6


@pytest.fixture(scope="module")
def store():
    return load_npz("obs_tiny.npz")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_step(store, t, o, W, layout):
    """the restatement's (or the kernel's) outputs `o` of step t at width W >= the reference's against the golden"""
    g = lambda k: store[f"{layout}/{t}/{k}"]
    L = g("ob_img").shape[1]
    assert W >= L
    for k in ("ob_img", "ob_ang", "ob_nav"):
        assert same(np.ascontiguousarray(o[k][:, :L]), g(k)), (layout, t, k)
        assert not o[k][:, L:].any(), (layout, t, k)                                   # beyond the reference's columns: zero ...
    length = g("ob_len") if layout == "pano" else g("cand_len")
    assert same(o["ob_len"], length) and same(o["cand_len"], g("cand_len"))
    assert np.array_equal(o["ob_mask"], (np.arange(W)[None] < length[:, None]).astype(np.uint8))        # ... and masked
    C = store["walk/cand_node"].shape[2]
    for k, w in (("cand_nodes", "cand_node"), ("cand_points", "cand_point")):
        assert np.array_equal(o[k][:, :C], store["walk/" + w][t][:, :min(C, W)]) and (o[k][:, C:] == -1).all(), (t, k)
    for k in ("hist_img", "hist_pano_img", "hist_pano_ang"):
        assert same(o[k], store[f"hist/{t}/{k}"]), (t, k)


@pytest.mark.parametrize("layout", ["pano", "cand"])
@pytest.mark.parametrize("extra", [0, 3])
def test_restatement_equals_the_reference(store, layout, extra):
    tab = golden_tables(store)
    for t in range(T):
        W = store[f"{layout}/{t}/ob_img"].shape[1] + extra
        o, anomalies = gather_ref(tab, store["walk/scan"], store["walk/cur"][t], store["walk/view"][t], W, layout)
        assert anomalies == 0
        check_step(store, t, o, W, layout)
        assert np.array_equal(turn_ref(o["cand_points"], store["walk/env_action"][t], store["walk/view"][t]), store["walk/view"][t + 1]), t


def test_the_golden_holds_the_cases_it_is_meant_to(store):
    tab, w = golden_tables(store), {k: store["walk/" + k] for k in ("scan", "cur", "view", "ended", "env_action")}
    rows = tab["vp_base"][w["scan"]][None] + w["cur"]
    cnt = tab["cand_cnt"][rows]
    C = tab["cand_point"].shape[1]
    assert {0, C} <= set(cnt.ravel().tolist())
    shared = {int(n) - len(set(tab["cand_point"][r, :n].tolist())) for r, n in zip(rows.ravel(), cnt.ravel())}
    assert {1, 2} <= shared                                   # two and three candidates on one view
    assert len(set(w["scan"].tolist())) == 3 and (rows[0, 0] == rows[0, 1]) and w["ended"].any()
    assert {0, 11, 12, 35} <= set(w["view"].ravel().tolist()) and {v // 12 for v in w["view"].ravel().tolist()} == {0, 1, 2}
    assert max_ob_len(tab) == max(store[f"pano/{t}/ob_img"].shape[1] for t in range(T))


def _walk(store, layout, W, mutate=None):
    """every output of every step of the golden's walk (its recorded positions), and the views the turns give, under one mutation"""
    tab, outs, views, stale = golden_tables(store), [], [], None
    for t in range(T):
        o, _ = gather_ref(tab, store["walk/scan"], store["walk/cur"][t], store["walk/view"][t], W, layout, mutate=mutate, stale=stale)
        outs.append(o)
        stale = o
        views.append(turn_ref(o["cand_points"], store["walk/env_action"][t], store["walk/view"][t], mutate=mutate))
    return outs, views


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_each_mutation_is_seen_on_the_golden_inputs(store, mutate):
    """the cases are sensitive: one deliberate error in the restatement changes what it returns on the golden's walk, and the changed
    result no longer equals the golden"""
    W = max(store[f"pano/{t}/ob_img"].shape[1] for t in range(T))
    want, want_views = _walk(store, "pano", W)
    got, got_views = _walk(store, "pano", W, mutate)
    differs = any(not same(w[k], g[k]) for w, g in zip(want, got) for k in OUTPUTS) or any(not np.array_equal(w, g) for w, g in zip(want_views, got_views))
    assert differs, mutate
    caught = False
    for t in range(T):
        try:
            check_step(store, t, got[t], W, "pano")
            assert np.array_equal(got_views[t], store["walk/view"][t + 1])
        except AssertionError:
            caught = True
    assert caught, mutate


def test_out_of_range_episodes_are_stop_alone(store):
    tab = golden_tables(store)
    scan, cur, view = np.array([0, 1, 2, 0], np.int32), np.array([7, -1, 3, 2], np.int32), np.array([0, 5, 36, 35], np.int32)
    o, anomalies = gather_ref(tab, scan, cur, view, 40)
    assert anomalies == 3
    for b in range(3):
        assert not o["ob_img"][b].any() and not o["ob_ang"][b].any() and o["ob_nav"][b].tolist() == [2] + [0] * 39
        assert o["ob_len"][b] == o["cand_len"][b] == 1 and o["ob_mask"][b].sum() == 1 and not o["hist_pano_img"][b].any()
    assert o["cand_len"][3] == tab["cand_cnt"][2] + 1 and o["ob_img"][3].any()


def _graphs_of(store):
    """what agent.obs.build_tables reads of a NavGraphs, over the golden's three scans (scanS has no connectivity file)"""
    scans = [str(s) for s in store["meta/scans"]]
    nodes = {"scanA": ["a%02d" % i for i in range(7)], "scanB": ["b%02d" % i for i in range(5)], "scanS": ["s%02d" % i for i in range(9)]}
    return types.SimpleNamespace(scans=scans, nodes=nodes, scan_n_host=np.array([len(nodes[s]) for s in scans], np.int32),
                                 node_id=lambda scan, vp: nodes[scan].index(vp))


def test_host_tables_equal_the_references(store):
    """agent.obs.build_tables (ObsStore's host side) from the golden's candidate lists: every table bit for bit, cand_ang included --
    the golden's is the reference's own make_candidate (cached branch) for each of the 12 base headings"""
    from vln_hamt_amd.agent.obs import build_tables
    tab, g = golden_tables(store), _graphs_of(store)
    cands, feats = {}, {}
    for si, scan in enumerate(g.scans):
        for li, vp in enumerate(g.nodes[scan]):
            row = int(tab["vp_base"][si]) + li
            feats[(scan, vp)] = np.concatenate([tab["feat"][row], np.ones((VIEWS, 3), np.float32)], 1)       # (wider than F: the first F columns count)
            cands[f"{scan}_{vp}"] = [{"viewpointId": g.nodes[scan][tab["cand_node"][row, c]], "pointId": int(tab["cand_point"][row, c]),
                                      "normalized_heading": float(store["table/cand_nh"][row, c]), "elevation": float(store["table/cand_el"][row, c])}
                                     for c in range(tab["cand_cnt"][row])]
    features = types.SimpleNamespace(get_image_feature=lambda scan, vp: feats[(scan, vp)])
    got = build_tables(g, features, cands, image_feat_size=16, angle_feat_size=4)
    for k in TABLES:
        assert same(got[k], tab[k]), k
    assert got["max_cands"] == 7 and got["max_ob_len"] == max_ob_len(tab)


def test_candidates_from_scanvp_keeps_file_order_and_adds_the_view_angles():
    import json
    from vln_hamt_amd.agent import ObsStore
    from vln_hamt_amd.data.r2r_data import _view_angles
    from _util import GOLDEN
    with open(os.path.join(GOLDEN, "r2r_tiny", "scanvp_cands.json")) as f:
        raw = json.load(f)
    got = ObsStore.candidates_from_scanvp(raw)
    views = _view_angles()
    assert list(got) == list(raw)
    for key, cands in raw.items():
        assert [c["viewpointId"] for c in got[key]] == list(cands)
        for c, v in zip(got[key], cands.values()):
            assert c["pointId"] == v[0] and c["normalized_heading"] == views[v[0]][0] + v[2] and c["elevation"] == views[v[0]][1] + v[3]


def test_header_binding_and_library_agree_on_the_new_symbols():
    from test_abi import _header_protos
    from vln_hamt_amd import _lib
    protos = _header_protos()
    assert protos.get("hamt_obs_gather") == 30 and protos.get("hamt_obs_turn") == 7
    assert len(_lib.SIGNATURES["hamt_obs_gather"]) == 30 and len(_lib.SIGNATURES["hamt_obs_turn"]) == 7
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert hasattr(lib, "hamt_obs_gather") and hasattr(lib, "hamt_obs_turn") and lib.hamt_version() == 2
    from vln_hamt_amd import ops
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hamt.h")).read()
    assert int(re.search(r"#define HAMT_OBS_MAX_CAND (\d+)", src).group(1)) == ops.OBS_MAX_CAND
    assert {k: int(re.search(rf"#define HAMT_OBS_{k.upper()} (\d+)", src).group(1)) for k in ops.OBS_LAYOUTS} == ops.OBS_LAYOUTS


def test_gather_kernel_uses_no_scratch(tmp_path):
    from test_kernel_resources import OBJCOPY, READELF, _code_objects
    if not (os.path.exists(READELF) and os.path.exists(OBJCOPY)):
        pytest.skip("ROCm LLVM tools not installed")
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = []
    for co in _code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and ("obs_gather_kernel" in name.group(1) or "obs_turn_kernel" in name.group(1)):
                seen.append((name.group(1), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                             int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                             int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))))
    assert len(seen) == 2, seen
    assert all(v == 0 and s == 0 and p == 0 for _, v, s, p in seen), seen
