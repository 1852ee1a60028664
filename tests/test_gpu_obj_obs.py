"""-m gpu: REVERIE's object gather on the device (csrc/obs.hip -> ops.obj_gather -> agent.ObjStore / ObjEpisodes) against the reference's
own functions (tests/golden/obj_obs_tiny.npz) and the numpy restatement (tests/_obj_obs_ref.py), and a rollout of the tiny NavRef model
fed by it against the same rollout fed by host-built object tensors.  A pure gather: every comparison is bit for bit."""
import json
import os
import types

import numpy as np
import pytest
import torch

from _obj_obs_ref import OBJ_TABLES, OUTPUTS, golden_obj_tables, obj_gather_ref, random_obj_tables
from _util import GOLDEN, load_npz
from test_obj_obs_ref import check_step, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 4


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _store(tab, misalign=False):
    """an ObjStore over the restatement's tables; the viewpoint store is a stand-in holding what the object store shares with it"""
    from vln_hamt_amd.agent import ObjStore
    dev = {k: d(tab[k]) for k in OBJ_TABLES}
    if misalign:                                              # obj_feat 4 bytes off a 16-byte boundary, inside a larger allocation
        buf = torch.empty(tab["obj_feat"].size + 4, dtype=torch.float32, device=DEV)
        dev["obj_feat"] = buf[1:1 + tab["obj_feat"].size].view(tab["obj_feat"].shape).copy_(dev["obj_feat"])
        assert dev["obj_feat"].data_ptr() % 16 == 4
    obs_store = types.SimpleNamespace(device=torch.device(DEV, torch.cuda.current_device()), NV=len(tab["obj_off"]) - 1, A=tab["ang36"].shape[2],
                                      ang36=d(tab["ang36"]), vp_base=d(tab["vp_base"]), scan_n=d(tab["scan_n"]), graphs=None)
    return ObjStore.from_tensors(obs_store, *(dev[k] for k in OBJ_TABLES))


def _episodes(store, scan, cur, view, Ow=None, misalign=False):
    """ObjEpisodes over stand-in episodes (scan, current node and view as device tensors: all that the gather reads of them), every
    output buffer pre-filled with NaN / 0x7f bytes"""
    from vln_hamt_amd.agent import ObjEpisodes, ObjObservation
    nav = types.SimpleNamespace(scan=d(np.asarray(scan, np.int32)), cur=d(np.asarray(cur, np.int32)), B=len(cur))
    obs = types.SimpleNamespace(store=store.obs_store, nav=nav, B=len(cur), view=d(np.asarray(view, np.int32)))
    ep = ObjEpisodes(store, obs, width=Ow)
    if misalign:                                              # obj_feats 4 bytes off a 16-byte boundary as well
        buf = torch.empty(ep.obj_feats.numel() + 4, dtype=torch.float32, device=DEV)
        ep.obj_feats = buf[1:1 + ep.obj_feats.numel()].view(ep.obj_feats.shape)
        ep._obs = ObjObservation(ep.obj_feats, *ep._obs[1:])
        assert ep.obj_feats.data_ptr() % 16 == 4
    _poison(ep)
    return ep


def _poison(ep):
    for k in OUTPUTS:
        t_ = getattr(ep, k)
        t_.fill_(float("nan")) if t_.dtype.is_floating_point else t_.view(torch.uint8).fill_(0x7F)


def _host(ep, o):
    """an ObjObservation as the restatement's dict (obj_masks as the uint8 the kernel wrote)"""
    assert o.obj_masks.dtype == torch.bool and o.obj_lens.dtype == o.obj_ids.dtype == torch.int32
    out = {k: v.cpu().numpy() for k, v in o._asdict().items()}
    out["obj_masks"] = ep.obj_masks.cpu().numpy()
    return out


def _equal(got, want):
    for k in OUTPUTS:
        assert same(got[k], want[k]), k


@pytest.mark.parametrize("extra", [0, 3])
def test_golden_steps(extra):
    """every step of the golden's walk (B = 6, Fo = 16: the 16-byte path, A = 4) at Ow = the store's width and 3 above it: the
    reference's own arrays on its columns, zero, unmasked and -1 beyond them; == the restatement"""
    g = load_npz("obj_obs_tiny.npz")
    tab = golden_obj_tables(g)
    store = _store(tab)
    assert store.max_objs == int(g["meta/max_objects"]) == 3
    Ow = store.max_objs + extra
    ep = _episodes(store, g["walk/scan"], g["walk/cur"][0], g["walk/view"][0], Ow)
    for t in range(T):
        ep.nav.cur.copy_(d(g["walk/cur"][t]))
        ep.obs.view.copy_(d(g["walk/view"][t]))
        _poison(ep)
        got = _host(ep, ep.observe())
        _equal(got, obj_gather_ref(tab, g["walk/scan"], g["walk/cur"][t], g["walk/view"][t], Ow)[0])
        check_step(g, t, got, Ow)
    assert int(ep.anomalies.item()) == 0


@pytest.mark.parametrize("B,Fo,A,misalign", [(1, 16, 4, False), (5, 16, 4, False), (5, 6, 4, False), (5, 16, 8, False), (5, 6, 8, False),
                                             (5, 16, 4, True)])
def test_shapes_vs_restatement(B, Fo, A, misalign):
    """B = 1 and 5, Fo = 16 (16 bytes per lane) and Fo = 6 (element by element), A = 4 and 8, and an Fo = 16 store whose `obj_feat` and
    output `obj_feats` start 4 bytes off a 16-byte boundary (element by element again), on a synthetic store holding every count from 0
    to max_objects = 5 (three scans; 5 slots and more: two row blocks of 4 waves); every output element must be overwritten"""
    tab = random_obj_tables(31 + Fo + A, Fo=Fo, A=A, max_objects=5)
    store = _store(tab, misalign)
    assert store.max_objs == 5
    rng = np.random.Generator(np.random.PCG64(B))
    places = [(s, c) for s, n in enumerate(tab["scan_n"]) for c in range(n)]       # B = 5: the four trials visit every viewpoint
    seen = set()
    for trial in range(4):
        scan, cur = (np.array(x, np.int32) for x in zip(*(places[(7 * (trial * B + b)) % len(places)] for b in range(B))))
        view = rng.integers(0, 36, B).astype(np.int32)
        Ow = 5 + trial
        ep = _episodes(store, scan, cur, view, Ow, misalign)
        got = _host(ep, ep.observe())
        _equal(got, obj_gather_ref(tab, scan, cur, view, Ow)[0])
        assert not np.isnan(got["obj_feats"]).any() and (got["obj_masks"] <= 1).all() and int(ep.anomalies.item()) == 0
        seen |= set(got["obj_lens"].tolist())
    if B > 1:
        assert seen == set(range(6)), seen


def test_offsets_beyond_2_31_elements():
    """an uninitialised `obj_feat` of more than 2^31 elements (8.6 GB; 524290 viewpoints of 256 objects each, which is also the widest
    observation a step takes) with only the addressed objects filled: those of the last two viewpoints and of the first; 32-bit offset
    arithmetic would read elsewhere"""
    Fo, A, M = 16, 4, 256
    NV = (2 ** 31) // (Fo * M) + 2
    NObj = NV * M
    assert NObj * Fo > 2 ** 31
    small = random_obj_tables(5, scan_n=(3,), Fo=Fo, A=A, max_objects=2)           # its tables are replaced: 3 viewpoints of M objects
    rng = np.random.Generator(np.random.PCG64(9))
    small.update(obj_off=np.arange(4, dtype=np.int64) * M, obj_feat=rng.standard_normal((3 * M, Fo)).astype(np.float32),
                 obj_view=rng.integers(0, 36, 3 * M).astype(np.int32), obj_pos=rng.random((3 * M, 5)).astype(np.float32),
                 obj_id=rng.permutation(3 * M).astype(np.int32))
    rows = [0, NV - 2, NV - 1]                                                      # small's viewpoints 0, 1, 2 stand for these
    feat, pos = torch.empty(NObj, Fo, dtype=torch.float32, device=DEV), torch.empty(NObj, 5, dtype=torch.float32, device=DEV)
    view, ids = torch.zeros(NObj, dtype=torch.int32, device=DEV), torch.zeros(NObj, dtype=torch.int32, device=DEV)
    for i, r in enumerate(rows):
        sl, src = slice(r * M, (r + 1) * M), slice(i * M, (i + 1) * M)
        feat[sl], pos[sl], view[sl], ids[sl] = d(small["obj_feat"][src]), d(small["obj_pos"][src]), d(small["obj_view"][src]), d(small["obj_id"][src])
    from vln_hamt_amd.agent import ObjStore
    obs_store = types.SimpleNamespace(device=feat.device, NV=NV, A=A, ang36=d(small["ang36"]), vp_base=torch.zeros(1, dtype=torch.int64, device=DEV),
                                      scan_n=torch.tensor([NV], dtype=torch.int32, device=DEV), graphs=None)
    store = ObjStore.from_tensors(obs_store, torch.arange(NV + 1, dtype=torch.int64, device=DEV) * M, feat, view, pos, ids)
    assert store.max_objs == M
    look = np.array([35, 0, 12], np.int32)
    ep = _episodes(store, [0, 0, 0], [NV - 1, 0, NV - 2], look, M)
    got = _host(ep, ep.observe())
    want, _ = obj_gather_ref(small, [0, 0, 0], [2, 0, 1], look, M)
    _equal(got, want)
    assert int(ep.anomalies.item()) == 0 and got["obj_lens"].tolist() == [M, M, M]


def test_out_of_range_episodes_are_counted_and_zeroed():
    """a scan outside the store, a current node outside its scan (above, below) and a view outside [0, 36) (above, below): one live zero
    slot, count 0, ids -1, one anomaly each, the neighbours untouched -- and nothing written beyond the outputs: each buffer lies
    between guard bands of NaN / 0x7f bytes inside a larger allocation"""
    from vln_hamt_amd import ops
    g = load_npz("obj_obs_tiny.npz")
    tab = golden_obj_tables(g)
    store = _store(tab)
    scan, cur, view = [0, 1, 1, 2, -1, 0, 1], [7, -1, 1, 0, 0, 1, 2], [0, 5, 36, 3, 3, 35, -1]
    B, Ow, GUARD = len(cur), 5, 64
    shapes = {"obj_feats": ((B, Ow, 16), torch.float32), "obj_angles": ((B, Ow, 4), torch.float32), "obj_poses": ((B, Ow, 5), torch.float32),
              "obj_masks": ((B, Ow), torch.uint8), "obj_lens": ((B,), torch.int32), "obj_ids": ((B, Ow), torch.int32)}
    bufs, out = {}, types.SimpleNamespace()
    for k, (shape, dt) in shapes.items():
        n = int(np.prod(shape))
        big = torch.empty(n + 2 * GUARD, dtype=dt, device=DEV)
        big.fill_(float("nan")) if dt.is_floating_point else big.view(torch.uint8).fill_(0x7F)
        bufs[k] = (big, n)
        setattr(out, k, big[GUARD:GUARD + n].view(shape))
    anomalies = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = (d(np.asarray(scan, np.int32)), d(np.asarray(cur, np.int32)), d(np.asarray(view, np.int32)))
    ops.obj_gather(store, *args, out, anomalies)
    got = {k: getattr(out, k).cpu().numpy() for k in OUTPUTS}
    want, n_bad = obj_gather_ref(tab, scan, cur, view, Ow)
    _equal(got, want)
    assert n_bad == 6 and int(anomalies.item()) == 6
    for b in (0, 1, 2, 3, 4, 6):
        assert not got["obj_feats"][b].any() and got["obj_masks"][b].tolist() == [1, 0, 0, 0, 0] and got["obj_lens"][b] == 0 and (got["obj_ids"][b] == -1).all()
    assert got["obj_lens"][5] == 3 and got["obj_feats"][5].any()
    for k, (big, n) in bufs.items():
        for band in (big[:GUARD], big[GUARD + n:]):
            assert bool(torch.isnan(band).all()) if band.dtype.is_floating_point else bool((band.view(torch.uint8) == 0x7F).all()), k
    ops.obj_gather(store, *args, out, anomalies)
    assert int(anomalies.item()) == 12                        # (counted per call, as the viewpoint gather's)


def test_device_side_refusals():
    from vln_hamt_amd import _lib, ops
    from vln_hamt_amd._lib import HamtError
    from vln_hamt_amd.agent import ObjEpisodes, ObjStore
    g = load_npz("obj_obs_tiny.npz")
    tab = golden_obj_tables(g)
    store = _store(tab)
    ep = _episodes(store, g["walk/scan"], g["walk/cur"][0], g["walk/view"][0])
    assert ep.Ow == 3 and ep.state_tensors()[0] is ep.anomalies
    with pytest.raises(ValueError):
        ObjEpisodes(store, ep.obs, width=2)
    with pytest.raises(ValueError):
        ObjEpisodes(store, ep.obs, width=257)
    with pytest.raises(ValueError):
        ObjEpisodes(store, types.SimpleNamespace(store=object(), nav=ep.nav, B=6, view=ep.obs.view))
    with pytest.raises(HamtError):                            # tables on the host
        ObjStore.from_tensors(store.obs_store, *(torch.from_numpy(tab[k]) for k in OBJ_TABLES))
    bad = dict(tab, obj_off=tab["obj_off"][:-1])
    with pytest.raises(HamtError):                            # one offset short of the viewpoint store's rows
        ObjStore.from_tensors(store.obs_store, *(d(bad[k]) for k in OBJ_TABLES))
    bad = dict(tab, obj_off=tab["obj_off"] + 1)
    with pytest.raises(HamtError):                            # offsets that do not start at 0
        ObjStore.from_tensors(store.obs_store, *(d(bad[k]) for k in OBJ_TABLES))
    with pytest.raises(HamtError):                            # a view vector of the wrong dtype
        ops.obj_gather(store, ep.nav.scan, ep.nav.cur, ep.obs.view.long(), ep, ep.anomalies)
    # the C entry point itself: a width above HAMT_OBJ_MAX_WIDTH is unsupported, and nothing is launched
    wide = types.SimpleNamespace(**{k: getattr(ep, k) for k in OUTPUTS})
    _poison(ep)
    p = ops._p
    rc = _lib.load().hamt_obj_gather(6, 257, 16, 4, 2, store.NV, store.NObj, p(store.obj_off), p(store.obj_feat), p(store.obj_view), p(store.obj_pos),
                                     p(store.obj_id), p(store.ang36), p(store.vp_base), p(store.scan_n), p(ep.nav.scan), p(ep.nav.cur), p(ep.obs.view),
                                     p(wide.obj_feats), p(wide.obj_angles), p(wide.obj_poses), p(wide.obj_masks), p(wide.obj_lens), p(wide.obj_ids),
                                     p(ep.anomalies), ops._stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool(torch.isnan(ep.obj_feats).all()) and int(ep.anomalies.item()) == 0


# ------------------------------------------------------------------------------------------------ end to end on the tiny NavRef model
STEPS, MAX_OBJECTS = 4, 3
COUNTS = {"scanA_a00": 1, "scanA_a01": 3, "scanA_a02": 5, "scanA_a04": 2, "scanA_a05": 3, "scanA_a06": 1,
          "scanB_b00": 2, "scanB_b01": 3, "scanB_b02": 4, "scanB_b04": 1}                      # a03 and b03: no objects
SCANS = ["scanA", "scanA", "scanB", "scanB"]
STARTS = {"one": (["a00", "a02", "b00", "b03"], [0, 13, 26, 35]), "two": (["a04", "a01", "b01", "b02"], [7, 24, 11, 12])}


def _database(Fo):
    rng = np.random.Generator(np.random.PCG64(83))
    db = {}
    for i, (key, n) in enumerate(COUNTS.items()):
        boxes = np.concatenate([rng.integers(0, 400, (n, 2)), rng.integers(8, 200, (n, 2))], 1)
        db[key] = {"obj_ids": [str(100 * (i + 1) + j) for j in range(n)], "fts": (rng.standard_normal((n, Fo + 3)) * 0.5).astype(np.float32),
                   "bboxes": boxes.astype(np.int64) if i % 2 else boxes.astype(np.float32), "viewindexs": rng.integers(0, 36, n)}
    return db


class _HostObjFeed:
    """the host path: the restatement on the host tables at the same width, uploaded every step"""

    def __init__(self, tab, obs, Ow):
        self.tab, self.obs, self.Ow, self.anomalies = tab, obs, Ow, torch.zeros(1, dtype=torch.int32, device=DEV)

    def reset(self):
        return self

    def observe(self):
        from vln_hamt_amd.agent import ObjObservation
        nav = self.obs.nav
        o, bad = obj_gather_ref(self.tab, nav.scan.cpu().numpy(), nav.cur.cpu().numpy(), self.obs.view.cpu().numpy(), self.Ow)
        assert bad == 0
        o["obj_masks"] = o["obj_masks"].astype(bool)
        return ObjObservation(*(d(o[k]) for k in OUTPUTS))

    def state_tensors(self):
        return (self.anomalies,)


def _world():
    from test_gpu_obs import F_E2E, _Features
    from test_gpu_reverie import G, _navref
    from vln_hamt_amd.agent import NavGraphs, ObjStore, ObsStore, build_obj_tables
    from vln_hamt_amd.reverie.model_navref import NavRefModel
    tiny = os.path.join(GOLDEN, "r2r_tiny")
    graphs = NavGraphs(tiny, device=DEV)
    with open(os.path.join(tiny, "scanvp_cands.json")) as f:
        cands = ObsStore.candidates_from_scanvp(json.load(f))
    store = ObsStore(graphs, _Features(), cands, image_feat_size=F_E2E, angle_feat_size=4)
    cfg = G.tiny_cfg(True)
    Fo = G.obj_feat_size(cfg)
    db = _database(Fo)
    objs = ObjStore(store, db, obj_feat_size=Fo, max_objects=MAX_OBJECTS)
    tab = build_obj_tables(graphs, db, Fo, MAX_OBJECTS)
    for k in OBJ_TABLES:
        assert same(getattr(objs, k).cpu().numpy(), tab[k]), k
    assert objs.max_objs == MAX_OBJECTS and objs.ang36 is store.ang36
    tab.update(ang36=store.ang36.cpu().numpy(), vp_base=store.vp_base.cpu().numpy(), scan_n=store.scan_n.cpu().numpy())
    agent = NavRefModel.__new__(NavRefModel)
    torch.nn.Module.__init__(agent)
    agent.args = types.SimpleNamespace(no_lang_ca=True, feat_dropout=0.0)
    agent.vln_bert = _navref(cfg, "bf16")
    agent.drop_env = torch.nn.Dropout(0.0)
    agent.eval()
    x = G.inputs(cfg, G.TINY)
    b = {k: x[k].to(DEV) for k in ("txt_ids", "txt_masks")}
    assert b["txt_ids"].shape[0] == 4
    return graphs, cands, db, store, objs, tab, agent, b


def _reset(which, cands, db, nav, rec, cache, obs, feed, cls):
    """-> the goal objects (int32 [B] on the device): the LAST object kept at the viewpoint each ground-truth path ends on, -1 if none"""
    from vln_hamt_amd.agent import goal_objects
    starts, views = STARTS[which]
    first = lambda s, vp: cands[f"{s}_{vp}"][0]["viewpointId"]
    gts = [[vp, first(s, vp)] for s, vp in zip(SCANS, starts)]
    items = [{"objId": db[f"{s}_{gt[-1]}"]["obj_ids"][:MAX_OBJECTS][-1] if f"{s}_{gt[-1]}" in db else None} for s, gt in zip(SCANS, gts)]
    nav.reset(SCANS, starts, gts, [[gt[-1]] for gt in gts])
    rec.reset(fresh_draws=False)
    cache.reset(cls)
    obs.reset(views)
    feed.reset()
    return goal_objects(items).to(DEV)


def _make_step(agent, lang, b, nav, rec, cache, obs, feed, goal, sids):
    def step(t):
        cache.n = t + 1                                       # (the history's length is the host's: one captured graph per step)
        o, j = obs.observe(), feed.observe()                  # (the objects before obs.turn: seen from this step's view)
        # REVERIE's observation has no STOP slot among the views (its STOP is the object column): the slot the viewpoint gather marks
        # as nav type 2 is demoted to a plain, all-zero view, whose action logit the model sets to -inf
        outs = agent("visual", txt_embeds=lang, txt_masks=b["txt_masks"], hist_embeds=cache, hist_lens=rec.hist_len, ob_img_feats=o.ob_img,
                     ob_ang_feats=o.ob_ang, ob_nav_types=o.ob_nav * (o.ob_nav == 1), ob_masks=o.ob_mask, obj_feats=j.obj_feats,
                     obj_angles=j.obj_angles, obj_poses=j.obj_poses, obj_masks=j.obj_masks)
        a_t, env, prev = rec.step(t, outs["act_logits"], outs["obj_logits"], j.obj_lens, cand_lens=o.cand_len, ob_ang_feats=o.ob_ang,
                                  feedback="argmax", sync=False, nav=nav, cand_nodes=o.cand_nodes, teacher_mode="shortest", stop_logit="value",
                                  obj_ids=j.obj_ids, goal_obj=goal)
        obs.turn(env, t)
        cache.append(agent.vln_bert("history", hist_img_feats=o.hist_img, hist_ang_feats=prev, ob_step_ids=sids[t],
                                    hist_pano_img_feats=o.hist_pano_img, hist_pano_ang_feats=o.hist_pano_ang))
        return outs["act_logits"], outs["obj_logits"], a_t, env
    return step


def _run(step, nav, rec, call=None):
    out = []
    for t in range(STEPS):
        res = step(t) if call is None else call(t)
        out.append([r.clone() for r in res])
    slots, ids = rec.predicted_objects()
    return out, nav.path.clone(), nav.path_len.clone(), rec.ended.clone(), rec.ref.clone(), slots, ids


def _same_rollout(want, got, what):
    for t, (w, g_) in enumerate(zip(want[0], got[0])):
        for i in (0, 1):
            fin = torch.isfinite(w[i])
            assert torch.equal(torch.isfinite(g_[i]), fin) and torch.equal(w[i][fin], g_[i][fin]), (what, t, ("act_logits", "obj_logits")[i])
        assert torch.equal(w[2], g_[2]) and torch.equal(w[3], g_[3]), (what, t, "actions")
    for w, g_, k in zip(want[1:5], got[1:5], ("path", "path_len", "ended", "ref")):
        assert torch.equal(w, g_), (what, k)
    assert np.array_equal(want[5], got[5]) and np.array_equal(want[6], got[6]), (what, "predicted objects")


def test_rollout_fed_by_the_device_equals_the_host_fed_rollout():
    """The tiny NavRef model in argmax feedback over r2r_tiny (B = 4, two scans, 4 steps): observe (views and objects) -> visual ->
    rec.step(nav=..., obj_ids=..., goal_obj=...) -> turn -> history.  Fed by host-built object tensors at the same width, fed by
    ObjEpisodes eagerly, and with the device loop captured by graph.GraphedInference with no tensor input per step -- captured on one
    set of start positions and replayed, after reset, on another: both logit rows bit-identical at the finite positions; actions,
    paths, `ended`, `rec.ref` and the predicted objects identical; no anomaly."""
    from vln_hamt_amd.agent import GoalSetEpisodes, ObjEpisodes, ObsEpisodes, ReverieRolloutRecorder
    from vln_hamt_amd.graph import GraphedInference
    from vln_hamt_amd.models.model_HAMT import HistoryCache
    graphs, cands, db, store, objs, tab, agent, b = _world()
    B, H = 4, 128
    sids = [torch.tensor([t], dtype=torch.long, device=DEV) for t in range(STEPS)]
    goal = torch.zeros(B, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        lang = agent("language", txt_ids=b["txt_ids"], txt_masks=b["txt_masks"])
        cls = agent("history")
        runs = {}
        for name in ("host", "device", "graph"):
            nav, rec, cache = GoalSetEpisodes(graphs, STEPS, B, max_gt=8, max_goals=4), ReverieRolloutRecorder(STEPS, B, DEV), HistoryCache(B, STEPS + 1, H, DEV)
            obs = ObsEpisodes(store, nav)
            feed = _HostObjFeed(tab, obs, objs.max_objs) if name == "host" else ObjEpisodes(objs, obs)
            step = _make_step(agent, lang, b, nav, rec, cache, obs, feed, goal, sids)
            call = None
            if name == "graph":
                gi = GraphedInference(step, state=(rec.ended, rec.hist_len, rec._pred, *nav.state_tensors(), *obs.state_tensors(),
                                                   *feed.state_tensors(), cache.buf))
                call = lambda t, gi=gi: gi(("step", t), t)
            for which in ("one", "two"):
                goal.copy_(_reset(which, cands, db, nav, rec, cache, obs, feed, cls))
                runs[name, which] = _run(step, nav, rec, call)
                assert int(feed.anomalies.item()) == 0 and int(obs.anomalies.item()) == 0
            if name == "graph":
                assert len(gi.graphs) == STEPS                # (the second rollout replayed the first one's graphs)
    # what the host-fed run alone must show: a move, and a stop that predicts an object at a viewpoint that has objects
    host = [runs["host", w] for w in ("one", "two")]
    moved = sum(int((r[0][t][3] >= 0).sum()) for r in host for t in range(STEPS))
    grounded = sum(int((r[5] >= 0).sum()) for r in host)
    refs = sum(int((r[4] != 0).sum()) for r in host)
    print(f"[obj rollout] {moved} moves in {2 * STEPS * B} episode steps; {grounded} of {2 * B} episodes predict an object; {refs} object losses; "
          f"slots {[r[5].tolist() for r in host]} ids {[r[6].tolist() for r in host]} actions {[[r[0][t][2].tolist() for t in range(STEPS)] for r in host]}")
    assert moved >= 1 and grounded >= 1, (moved, grounded)
    V = host[0][0][0][0].shape[1]
    stops = [(w, t, b_) for w, r in enumerate(host) for t in range(STEPS) for b_ in range(B) if int(r[0][t][2][b_]) >= V and r[5][b_] >= 0]
    assert stops, "no stop the policy chose predicts an object"       # (an episode stops once: its prediction is that stop's)
    for r in host:
        assert all(i == -1 or str(i) in {x for e in db.values() for x in e["obj_ids"]} for i in r[6].tolist())
    assert not torch.equal(host[0][0][0][0], host[1][0][0][0])
    for which in ("one", "two"):
        _same_rollout(runs["host", which], runs["device", which], ("device", which))
        _same_rollout(runs["host", which], runs["graph", which], ("graph", which))
