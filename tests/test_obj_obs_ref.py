"""Not gpu: the numpy restatement of csrc/obs.hip's object gather (tests/_obj_obs_ref.py) against the reference's own functions
(tests/golden/obj_obs_tiny.npz, written by tools/gen_obj_obs_golden.py), the host side of agent.ObjStore and the loader against the
golden's database and tables, the new entry point in header, binding and library, and the kernel's code object.  A pure gather: every
comparison is bit for bit."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from _obj_obs_ref import MUTATIONS, OBJ_TABLES, OUTPUTS, golden_obj_tables, obj_gather_ref, positions, random_obj_tables
from _util import GOLDEN, load_npz

T, B = 4, 6


@pytest.fixture(scope="module")
def store():
    return load_npz("obj_obs_tiny.npz")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_step(store, t, o, Ow):
    """the restatement's (or the kernel's) outputs `o` of step t at width Ow >= the reference's against the golden"""
    g = lambda k: store[f"step/{t}/{k}"]
    L = g("obj_feats").shape[1]
    assert Ow >= L
    for k in ("obj_feats", "obj_angles", "obj_poses"):
        assert same(np.ascontiguousarray(o[k][:, :L]), g(k)), (t, k)
        assert not o[k][:, L:].any(), (t, k)                                            # beyond the reference's columns: zero ...
    assert same(o["obj_lens"], g("true_len")) and np.array_equal(np.maximum(o["obj_lens"], 1), g("obj_lens")), t
    assert np.array_equal(o["obj_masks"], (np.arange(Ow)[None] < g("obj_lens")[:, None]).astype(np.uint8)), t      # ... masked ...
    assert np.array_equal(o["obj_ids"][:, :L], g("obj_ids")) and (o["obj_ids"][:, L:] == -1).all(), t    # ... and without an id


def ref_target_of(o, goal, target, stop_column, ignoreid):
    """include/hamt.h on hamt_policy_ref_step_fwd's obj_id / goal_obj: the first k < obj_len with obj_id[k] == goal where the teacher
    says STOP (an ended episode's target is ignoreid), else ignored"""
    out = np.full(len(goal), ignoreid, np.int64)
    for b in range(len(goal)):
        if target[b] == stop_column:
            hits = np.flatnonzero(o["obj_ids"][b, :o["obj_lens"][b]] == goal[b])
            if hits.size:
                out[b] = hits[0]
    return out


@pytest.mark.parametrize("extra", [0, 3])
def test_restatement_equals_the_reference(store, extra):
    tab = golden_obj_tables(store)
    ignoreid, stop = int(store["meta/ignoreid"]), int(store["meta/ob_img_max_len"])
    for t in range(T):
        Ow = store[f"step/{t}/obj_feats"].shape[1] + extra
        o, anomalies = obj_gather_ref(tab, store["walk/scan"], store["walk/cur"][t], store["walk/view"][t], Ow)
        assert anomalies == 0
        check_step(store, t, o, Ow)
        assert np.array_equal(store[f"step/{t}/target"] == stop, store["walk/teacher_stop"][t])
        assert np.array_equal(ref_target_of(o, store["walk/goal"], store[f"step/{t}/target"], stop, ignoreid), store[f"step/{t}/ref_target"]), t


def test_the_golden_holds_the_cases_it_is_meant_to(store):
    tab = golden_obj_tables(store)
    M = int(store["meta/max_objects"])
    rows = tab["vp_base"][store["walk/scan"]][None] + store["walk/cur"]
    cnt = np.diff(tab["obj_off"])[rows]
    full = np.diff(tab["untruncated"]["obj_off"])[rows]
    widths = [store[f"step/{t}/obj_feats"].shape[1] for t in range(T)]
    assert {0, 1, M} <= set(cnt.ravel().tolist()) and (full > M).any() and int(np.diff(tab["obj_off"]).max()) == M
    assert any(w == M and cnt[t].min() >= 1 for t, w in enumerate(widths)) and min(widths) < M
    seen = store["walk/view"][cnt > 0]
    assert (seen < 12).any() and (seen >= 12).any() and (tab["obj_view"] < 12).any() and (tab["obj_view"] >= 12).any()
    assert len(set(store["walk/scan"].tolist())) == 2 and store["walk/ended"].any() and (store["walk/goal"] == -1).sum() == 1
    refs = np.stack([store[f"step/{t}/ref_target"] for t in range(T)])
    assert {0, 1, 2, int(store["meta/ignoreid"])} <= set(refs.ravel().tolist())
    # the goal of episode 2 sits among the objects the cut drops at the viewpoint it stops on
    r = int(rows[3, 2])
    u = tab["untruncated"]
    assert store["walk/teacher_stop"][3, 2] and store["walk/goal"][2] in u["obj_id"][u["obj_off"][r] + M:u["obj_off"][r + 1]]
    assert {str(store[f"db/{k}/bboxes"].dtype) for k in store["meta/db_keys"]} == {"int64", "float32"}


def _walk(store, Ow, mutate=None):
    """every output of every step of the golden's walk under one mutation"""
    tab, outs, stale = golden_obj_tables(store), [], None
    for t in range(T):
        o, _ = obj_gather_ref(tab, store["walk/scan"], store["walk/cur"][t], store["walk/view"][t], Ow, mutate=mutate, stale=stale)
        outs.append(o)
        stale = o
    return outs


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_each_mutation_is_seen_on_the_golden_inputs(store, mutate):
    """the cases are sensitive: one deliberate error in the restatement changes what it returns on the golden's walk, and the changed
    result no longer equals the golden"""
    Ow = int(store["meta/max_objects"]) + 3
    want, got = _walk(store, Ow), _walk(store, Ow, mutate)
    assert any(not same(w[k], g[k]) for w, g in zip(want, got) for k in OUTPUTS), mutate
    caught = False
    for t in range(T):
        check_step(store, t, want[t], Ow)
        try:
            check_step(store, t, got[t], Ow)
        except AssertionError:
            caught = True
    assert caught, mutate


def test_out_of_range_episodes_get_one_live_zero_slot(store):
    tab = golden_obj_tables(store)
    scan, cur, view = np.array([0, 1, 1, 2, -1, 0], np.int32), np.array([7, -1, 1, 0, 0, 1], np.int32), np.array([0, 5, 36, 3, 3, 35], np.int32)
    o, anomalies = obj_gather_ref(tab, scan, cur, view, 5)
    assert anomalies == 5
    for b in range(5):
        assert not o["obj_feats"][b].any() and not o["obj_angles"][b].any() and not o["obj_poses"][b].any()
        assert o["obj_masks"][b].tolist() == [1, 0, 0, 0, 0] and o["obj_lens"][b] == 0 and (o["obj_ids"][b] == -1).all()
    assert o["obj_lens"][5] == 3 and o["obj_feats"][5].any()


def _database(store):
    """the generator's object database, in the form reverie.data_utils.load_obj_database returns"""
    return {str(k): {"obj_ids": [str(x) for x in store[f"db/{k}/obj_ids"]], "fts": store[f"db/{k}/fts"], "bboxes": store[f"db/{k}/bboxes"],
                     "viewindexs": store[f"db/{k}/viewindexs"]} for k in store["meta/db_keys"]}


def _graphs():
    from vln_hamt_amd.agent import NavGraphs
    return NavGraphs(os.path.join(GOLDEN, "r2r_tiny"))            # (host only: no device is needed to build the tables)


def test_host_tables_equal_the_references(store):
    """agent.build_obj_tables (ObjStore's host side) on the generator's database: every table bit for bit -- obj_pos is the reference's
    own get_obj_local_pos on int64 and on float32 boxes, stored into float32"""
    from vln_hamt_amd.agent import build_obj_tables
    tab, db = golden_obj_tables(store), _database(store)
    got = build_obj_tables(_graphs(), db, obj_feat_size=16, max_objects=3)
    for k in OBJ_TABLES:
        assert same(got[k], tab[k]), k
    assert got["max_objs"] == 3
    wide = {k: dict(e, fts=np.concatenate([e["fts"], np.ones((len(e["fts"]), 2), np.float32)], 1)) for k, e in db.items()}
    assert same(build_obj_tables(_graphs(), wide, 16, 3)["obj_feat"], tab["obj_feat"])       # (wider than Fo: the first Fo columns count)
    full = build_obj_tables(_graphs(), db, 16, 20)
    for k in OBJ_TABLES:
        assert same(full[k], tab["untruncated"][k]), k
    assert full["max_objs"] == 5
    empty = build_obj_tables(_graphs(), {}, 16, 3)
    assert empty["max_objs"] == 0 and not empty["obj_off"].any() and empty["obj_feat"].shape == (0, 16)


def test_load_obj_database_round_trips_an_npz(store, tmp_path):
    from vln_hamt_amd.agent import build_obj_tables
    from vln_hamt_amd.reverie.data_utils import load_obj_database
    db = _database(store)
    path = str(tmp_path / "objs.npz")
    np.savez(path, **{f"{k}/{f}": (np.array(e[f]) if f == "obj_ids" else e[f]) for k, e in db.items() for f in ("obj_ids", "fts", "bboxes", "viewindexs")})
    got = load_obj_database(path, 16)
    assert set(got) == set(db)
    for k, e in db.items():
        assert got[k]["obj_ids"] == e["obj_ids"] and all(isinstance(i, str) for i in got[k]["obj_ids"])
        for f in ("fts", "bboxes", "viewindexs"):
            assert same(got[k][f], e[f]), (k, f)
    assert all(e["fts"].shape[1] == 7 for e in load_obj_database(path, 7).values())          # (the reference's [:, :image_feat_size])
    tab = golden_obj_tables(store)
    built = build_obj_tables(_graphs(), got, 16, 3)
    assert all(same(built[k], tab[k]) for k in OBJ_TABLES)
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="h5py"):
            load_obj_database(str(tmp_path / "objs.hdf5"), 16)


def test_host_side_refusals(store):
    from vln_hamt_amd._lib import HamtError
    from vln_hamt_amd.agent import ObjEpisodes, build_obj_tables, goal_objects
    g, db = _graphs(), _database(store)
    first = str(store["meta/db_keys"][0])
    for field, bad in (("obj_ids", ["12a"] + db[first]["obj_ids"][1:]), ("obj_ids", ["-4"] + db[first]["obj_ids"][1:]),
                       ("viewindexs", np.full_like(db[first]["viewindexs"], 36)), ("viewindexs", np.full_like(db[first]["viewindexs"], -1)),
                       ("fts", db[first]["fts"][:, :15]), ("bboxes", db[first]["bboxes"][:, :3])):
        with pytest.raises(HamtError):
            build_obj_tables(g, {**db, first: dict(db[first], **{field: bad})}, 16, 3)
    with pytest.raises(HamtError):
        build_obj_tables(g, db, 16, 257)
    narrow = types.SimpleNamespace(max_objs=3)
    with pytest.raises(ValueError, match="below"):
        ObjEpisodes(narrow, None, width=2)                    # a width below the store's
    with pytest.raises(ValueError, match="above"):
        ObjEpisodes(narrow, None, width=257)                  # more object slots than a rollout step takes
    with pytest.raises(HamtError):
        goal_objects([{"objId": "chair"}])
    assert goal_objects([{"objId": 7}, {"objId": None}, {"objId": "12"}, {}]).tolist() == [7, -1, 12, -1]
    assert goal_objects([{"objId": None if x < 0 else int(x)} for x in store["walk/goal"]]).numpy().tolist() == store["walk/goal"].tolist()


def test_random_tables_hold_every_count():
    tab = random_obj_tables(3, max_objects=5)
    assert set(np.diff(tab["obj_off"]).tolist()) == set(range(6)) and same(positions(tab["obj_box"]), tab["obj_pos"])


def test_header_binding_and_library_agree_on_the_new_symbol():
    from test_abi import _header_protos
    from vln_hamt_amd import _lib, ops
    protos = _header_protos()
    assert protos.get("hamt_obj_gather") == 26 and len(_lib.SIGNATURES["hamt_obj_gather"]) == 26
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert hasattr(lib, "hamt_obj_gather") and lib.hamt_version() == 2
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hamt.h")).read()
    assert int(re.search(r"#define HAMT_OBJ_MAX_WIDTH (\d+)", src).group(1)) == ops.OBJ_MAX_WIDTH == 256


def test_ops_obj_gather_fails_loudly_on_the_cpu():
    import torch
    from vln_hamt_amd import ops
    from vln_hamt_amd._lib import HamtError
    out = types.SimpleNamespace(obj_feats=torch.zeros(1, 3, 16), obj_angles=torch.zeros(1, 3, 4))
    with pytest.raises(HamtError):
        ops.obj_gather(None, None, None, None, out, None)


def test_obj_gather_kernel_uses_no_scratch_and_no_lds(tmp_path):
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
            if name and "obj_gather_kernel" in name.group(1):
                seen.append((name.group(1), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                             int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                             int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                             int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))))
    assert len(seen) == 1, seen
    assert all(v == 0 and s == 0 and p == 0 and lds == 0 for _, v, s, p, lds in seen), seen
