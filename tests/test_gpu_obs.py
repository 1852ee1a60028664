"""-m gpu: the observation gather on the device (csrc/obs.hip -> ops.obs_gather / obs_turn -> agent.ObsStore / ObsEpisodes) against the
reference's own functions (tests/golden/obs_tiny.npz) and the numpy restatement (tests/_obs_ref.py), and a rollout of the tiny finetune
model fed by it against the same rollout fed by host-built observations.  A pure gather: every comparison is bit for bit."""
import json
import os
import types

import numpy as np
import pytest
import torch

from _obs_ref import OUTPUTS, TABLES, VIEWS, gather_ref, golden_tables, max_ob_len, random_tables, turn_ref
from _util import GOLDEN, load_npz, sub
from test_obs_ref import check_step, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 6


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _store(tab):
    from vln_hamt_amd.agent import ObsStore
    return ObsStore.from_tensors(*(d(tab[k]) for k in TABLES))


def _episodes(store, scan, cur, view, W=None, layout="pano", hist_pano=True, steps=T):
    """ObsEpisodes over stand-in episodes (scan and current node as device tensors: all that the gather reads of a NavEpisodes), every
    output buffer pre-filled with NaN / -1"""
    from vln_hamt_amd.agent import ObsEpisodes
    nav = types.SimpleNamespace(scan=d(np.asarray(scan, np.int32)), cur=d(np.asarray(cur, np.int32)), B=len(cur), T_max=steps)
    ep = ObsEpisodes(store, nav, width=W, layout=layout, hist_pano=hist_pano)
    ep.view.copy_(d(np.asarray(view, np.int32)))             # (not reset(): the out-of-range views of one test must get through)
    _poison(ep)
    return ep


def _poison(ep):
    for k in ("ob_img", "ob_ang", "ob_nav", "ob_mask", "ob_len", "cand_len", "cand_nodes", "cand_points", "hist_img", "hist_pano_img", "hist_pano_ang"):
        t_ = getattr(ep, k)
        if t_ is not None:
            t_.fill_(float("nan")) if t_.dtype.is_floating_point else t_.view(torch.uint8).fill_(0xFF)


def _host(ep, o):
    """an Observation as the restatement's dict (ob_mask as the uint8 the kernel wrote)"""
    assert o.ob_mask.dtype == torch.bool and o.ob_nav.dtype == torch.int64 and o.ob_len.dtype == o.cand_len.dtype == torch.int32
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in o._asdict().items()}
    out["ob_mask"] = ep.ob_mask.cpu().numpy()
    return out


def _equal(got, want, hist_pano=True):
    for k in OUTPUTS:
        if k.startswith("hist_pano") and not hist_pano:
            assert got[k] is None
        else:
            assert same(got[k], want[k]), k


@pytest.mark.parametrize("hist_pano", [True, False])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("layout", ["pano", "cand"])
def test_golden_steps(layout, extra, hist_pano):
    """every step of the golden's walk (B = 6, F = 16: the 16-byte path, A = 4) at W = the store's maximum and 3 above it, with and
    without the panorama history outputs: the reference's own arrays on its columns, zero and masked beyond them; == the restatement"""
    g = load_npz("obs_tiny.npz")
    tab = golden_tables(g)
    store = _store(tab)
    assert store.max_ob_len == max_ob_len(tab) and store.max_cands == 7
    W = (store.max_ob_len if layout == "pano" else store.max_cands + 1) + extra
    ep = _episodes(store, g["walk/scan"], g["walk/cur"][0], g["walk/view"][0], W, layout, hist_pano)
    for t in range(T):
        ep.nav.cur.copy_(d(g["walk/cur"][t]))
        ep.view.copy_(d(g["walk/view"][t]))
        _poison(ep)
        got = _host(ep, ep.observe())
        want, _ = gather_ref(tab, g["walk/scan"], g["walk/cur"][t], g["walk/view"][t], W, layout)
        _equal(got, want, hist_pano)
        if not hist_pano:
            got.update({k: g[f"hist/{t}/{k}"] for k in ("hist_pano_img", "hist_pano_ang")})
        check_step(g, t, got, W, layout)
    assert int(ep.anomalies.item()) == 0


@pytest.mark.parametrize("B,F,A,misalign", [(1, 16, 4, False), (5, 16, 4, False), (5, 6, 4, False), (5, 16, 8, False), (5, 6, 8, False),
                                            (5, 16, 4, True)])
@pytest.mark.parametrize("layout", ["pano", "cand"])
def test_shapes_vs_restatement(layout, B, F, A, misalign):
    """B = 1 and 5, F = 16 (16 bytes per lane) and F = 6 (element by element), A = 4 and 8, and an F = 16 store whose `feat` starts 4
    bytes off a 16-byte boundary (element by element again), on a synthetic store holding every candidate count from 0 to C"""
    from vln_hamt_amd.agent import ObsStore
    tab = random_tables(31 + F + A, scan_n=(5, 3), F=F, A=A, C=5)
    dev_tab = {k: d(tab[k]) for k in TABLES}
    if misalign:
        buf = torch.empty(tab["feat"].size + 4, dtype=torch.float32, device=DEV)
        dev_tab["feat"] = buf[1:1 + tab["feat"].size].view(tab["feat"].shape).copy_(dev_tab["feat"])
        assert dev_tab["feat"].data_ptr() % 16 == 4
    store = ObsStore.from_tensors(*(dev_tab[k] for k in TABLES))
    rng = np.random.Generator(np.random.PCG64(B))
    scan = rng.integers(0, 2, B).astype(np.int32)
    for trial in range(3):
        cur = np.array([rng.integers(0, tab["scan_n"][s]) for s in scan], np.int32)
        view = rng.integers(0, VIEWS, B).astype(np.int32)
        W = (store.max_ob_len if layout == "pano" else store.max_cands + 1) + trial
        ep = _episodes(store, scan, cur, view, W, layout)
        _equal(_host(ep, ep.observe()), gather_ref(tab, scan, cur, view, W, layout)[0])


def test_offsets_beyond_2_31_elements():
    """an uninitialised `feat` of more than 2^31 elements (8.6 GB) with only the addressed rows filled: the last two rows and the first;
    32-bit offset arithmetic would read elsewhere"""
    from vln_hamt_amd.agent import ObsStore
    F, A, C = 16, 4, 2
    NV = (2 ** 31) // (VIEWS * F) + 8
    assert NV * VIEWS * F > 2 ** 31
    small = random_tables(5, scan_n=(3,), F=F, A=A, C=C)              # rows 0, 1, 2 stand for rows 0, NV - 2, NV - 1
    small["cand_cnt"][:] = [2, 1, 2]
    small["cand_point"][:] = [[35, 0], [17, -1], [35, 35]]
    small["cand_node"][:] = [[1, 2], [0, -1], [2, 1]]
    rows = torch.tensor([0, NV - 2, NV - 1], device=DEV)
    feat = torch.empty(NV, VIEWS, F, dtype=torch.float32, device=DEV)
    feat[rows] = d(small["feat"])
    cnt, point, node = (torch.zeros(NV, dtype=torch.int32, device=DEV), torch.full((NV, C), -1, dtype=torch.int32, device=DEV),
                        torch.full((NV, C), -1, dtype=torch.int32, device=DEV))
    ang = torch.zeros(NV, C, 12, A, dtype=torch.float32, device=DEV)
    cnt[rows], point[rows], node[rows], ang[rows] = d(small["cand_cnt"]), d(small["cand_point"]), d(small["cand_node"]), d(small["cand_ang"])
    store = ObsStore.from_tensors(feat, d(small["ang36"]), cnt, point, node, ang, torch.zeros(1, dtype=torch.int64, device=DEV),
                                  torch.tensor([NV], dtype=torch.int32, device=DEV))
    assert store.max_cands == 2 and store.max_ob_len == 38
    view = np.array([35, 0, 12], np.int32)
    ep = _episodes(store, [0, 0, 0], [NV - 1, 0, NV - 2], view, 38)
    got = _host(ep, ep.observe())
    want, _ = gather_ref(small, [0, 0, 0], [2, 0, 1], view, 38)
    _equal(got, want)
    assert int(ep.anomalies.item()) == 0


def test_out_of_range_episodes_are_counted_and_zeroed():
    """a current node outside its scan (above, below) and a view outside [0, 36) (above, below): STOP alone, zero rows, one anomaly
    each, and the neighbours untouched -- inputs with a defined result (include/hamt.h)"""
    g = load_npz("obs_tiny.npz")
    tab = golden_tables(g)
    store = _store(tab)
    scan, cur, view = [0, 1, 2, 0, 2, 1], [7, -1, 3, 2, 3, 4], [0, 5, 36, 35, -1, 2]
    for layout in ("pano", "cand"):
        ep = _episodes(store, scan, cur, view, 40, layout)
        got = _host(ep, ep.observe())
        want, anomalies = gather_ref(tab, scan, cur, view, 40, layout)
        _equal(got, want)
        assert anomalies == 4 and int(ep.anomalies.item()) == 4
        for b in (0, 1, 2, 4):
            assert not got["ob_img"][b].any() and got["cand_len"][b] == 1 and got["ob_len"][b] == 1 and not got["hist_img"][b].any()
        ep.observe()
        assert int(ep.anomalies.item()) == 8                  # (counted per call, as nav.hip's)


def test_walk_of_gather_and_turn():
    """the golden's 6-step walk driven by the device's own views: observe, then turn with the recorded environment actions; the recorded
    nodes stand in for nav_advance.  Every step's outputs == the golden, views() == the recorded views"""
    g = load_npz("obs_tiny.npz")
    tab = golden_tables(g)
    ep = _episodes(_store(tab), g["walk/scan"], g["walk/cur"][0], g["walk/view"][0])
    ep.reset(g["walk/view"][0])
    for t in range(T):
        ep.nav.cur.copy_(d(g["walk/cur"][t]))
        _poison(ep)
        check_step(g, t, _host(ep, ep.observe()), ep.W, "pano")
        ep.turn(d(g["walk/env_action"][t]), t)
        assert np.array_equal(ep.view.cpu().numpy(), g["walk/view"][t + 1]), t
    assert np.array_equal(ep.views().cpu().numpy(), g["walk/view"])
    with pytest.raises(ValueError):
        ep.turn(d(g["walk/env_action"][0]), T)


def test_host_side_refusals():
    from vln_hamt_amd._lib import HamtError
    from vln_hamt_amd.agent import ObsEpisodes, ObsStore
    g = load_npz("obs_tiny.npz")
    tab = golden_tables(g)
    store = _store(tab)
    nav = types.SimpleNamespace(scan=d(g["walk/scan"]), cur=d(g["walk/cur"][0]), B=6, T_max=T)
    with pytest.raises(ValueError):
        ObsEpisodes(store, nav, width=store.max_ob_len - 1)
    with pytest.raises(ValueError):
        ObsEpisodes(store, nav, width=store.max_cands, layout="cand")
    with pytest.raises(ValueError):
        ObsEpisodes(store, nav).reset([0, 1, 2, 3, 4, 36])
    wide = random_tables(3, scan_n=(2,), C=65)
    with pytest.raises(HamtError):
        ObsStore.from_tensors(*(d(wide[k]) for k in TABLES))
    with pytest.raises(HamtError):
        ObsStore.from_tensors(*(torch.from_numpy(tab[k]) for k in TABLES))


# ------------------------------------------------------------------------------------------------ end to end on the tiny finetune model
F_E2E, STEPS = 64, 4
STARTS = {"one": (["a00", "a02", "b00", "b03"], [0, 13, 26, 35]), "two": (["a04", "a01", "b01", "b00"], [7, 24, 11, 12])}


class _Features:
    """random image features per viewpoint, wider than the model's 64 (the first 64 columns count)"""

    def __init__(self):
        self.rng, self.seen = np.random.Generator(np.random.PCG64(77)), {}

    def get_image_feature(self, scan, vp):
        if (scan, vp) not in self.seen:
            self.seen[(scan, vp)] = (self.rng.standard_normal((VIEWS, F_E2E + 5)) * 0.5).astype(np.float32)
        return self.seen[(scan, vp)]


class _HostFeed:
    """the host path: the restatement on the host tables, padded to W, uploaded every step"""

    def __init__(self, tab, nav, W):
        self.tab, self.nav, self.W = tab, nav, W

    def reset(self, views):
        self.view = np.asarray(views, np.int32)
        return self

    def observe(self):
        from vln_hamt_amd.agent import Observation
        o, _ = gather_ref(self.tab, self.nav.scan.cpu().numpy(), self.nav.cur.cpu().numpy(), self.view, self.W)
        self.points = o["cand_points"]
        o["ob_mask"] = o["ob_mask"].astype(bool)
        return Observation(*(d(o[k]) for k in OUTPUTS))

    def turn(self, env_action, t):
        self.view = turn_ref(self.points, env_action.cpu().numpy(), self.view)


def _world():
    from test_gpu_policy_step import _tiny_agent
    from vln_hamt_amd.agent import NavGraphs, ObsStore
    from vln_hamt_amd.agent.obs import build_tables
    tiny = os.path.join(GOLDEN, "r2r_tiny")
    graphs = NavGraphs(tiny, device=DEV)
    with open(os.path.join(tiny, "scanvp_cands.json")) as f:
        cands = ObsStore.candidates_from_scanvp(json.load(f))
    feats = _Features()
    store = ObsStore(graphs, feats, cands, image_feat_size=F_E2E, angle_feat_size=4)
    tab = build_tables(graphs, feats, cands, image_feat_size=F_E2E, angle_feat_size=4)
    for k in TABLES:
        assert same(getattr(store, k).cpu().numpy(), tab[k]), k
    agent, _, _ = _tiny_agent("bf16", True)
    b = {k: torch.from_numpy(v).to(DEV) for k, v in sub(load_npz("tiny_finetune.npz"), "nolangca/in/").items()}
    assert b["txt_ids"].shape[0] == 4
    return graphs, cands, store, tab, agent, b


def _reset(which, graphs, cands, nav, rec, cache, feed, cls):
    starts, views = STARTS[which]
    scans = ["scanA", "scanA", "scanB", "scanB"]
    gts = [[vp, cands[f"{s}_{vp}"][0]["viewpointId"], cands[f"{s}_{cands[f'{s}_{vp}'][0]['viewpointId']}"][-1]["viewpointId"]] for s, vp in zip(scans, starts)]
    nav.reset(scans, starts, gts)
    rec.reset(fresh_draws=False)
    cache.reset(cls)
    feed.reset(views)


def _make_step(agent, lang, b, nav, rec, cache, feed, sids):
    def step(t):
        cache.n = t + 1                                       # (the history's length is the host's: one captured graph per step)
        o = feed.observe()
        (logit,) = agent("visual", txt_embeds=lang, txt_masks=b["txt_masks"], hist_embeds=cache, hist_lens=rec.hist_len, ob_img_feats=o.ob_img,
                         ob_ang_feats=o.ob_ang, ob_nav_types=o.ob_nav, ob_masks=o.ob_mask)
        a_t, env, prev = rec.step(t, logit, cand_lens=o.cand_len, ob_ang_feats=o.ob_ang, feedback="argmax", sync=False, nav=nav,
                                  cand_nodes=o.cand_nodes)
        feed.turn(env, t)
        cache.append(agent.vln_bert("history", hist_img_feats=o.hist_img, hist_ang_feats=prev, ob_step_ids=sids[t],
                                    hist_pano_img_feats=o.hist_pano_img, hist_pano_ang_feats=o.hist_pano_ang))
        return logit, a_t, env
    return step


def _run(step, nav, rec, call=None):
    out = []
    for t in range(STEPS):
        res = step(t) if call is None else call(t)
        out.append([r.clone() for r in res])
    return out, nav.path.clone(), nav.path_len.clone(), rec.ended.clone()


def _same_rollout(want, got, what):
    for t, (w, g_) in enumerate(zip(want[0], got[0])):
        fin = torch.isfinite(w[0])
        assert torch.equal(torch.isfinite(g_[0]), fin) and torch.equal(w[0][fin], g_[0][fin]), (what, t, "logits")
        assert torch.equal(w[1], g_[1]) and torch.equal(w[2], g_[2]), (what, t, "actions")
    for w, g_, k in zip(want[1:], got[1:], ("path", "path_len", "ended")):
        assert torch.equal(w, g_), (what, k)


def test_rollout_fed_by_the_device_equals_the_host_fed_rollout():
    """The tiny finetune model in argmax feedback over r2r_tiny (B = 4, two scans, 4 steps): observe -> visual -> rec.step(nav=...) -> turn ->
    history.  Fed by host-built observations padded to the same W, fed by ObsEpisodes eagerly, and with the device loop captured by
    graph.GraphedInference with no tensor input per step -- captured on one set of start positions and replayed, after reset, on another:
    logits bit-identical, actions, paths and `ended` identical."""
    from vln_hamt_amd.agent import NavEpisodes, ObsEpisodes, RolloutRecorder
    from vln_hamt_amd.graph import GraphedInference
    from vln_hamt_amd.models.model_HAMT import HistoryCache
    graphs, cands, store, tab, agent, b = _world()
    B, H = 4, 128
    sids = [torch.tensor([t], dtype=torch.long, device=DEV) for t in range(STEPS)]
    with torch.no_grad():
        lang = agent("language", txt_ids=b["txt_ids"], txt_masks=b["txt_masks"])
        cls = agent("history")
        runs = {}
        for name in ("host", "device", "graph"):
            nav, rec, cache = NavEpisodes(graphs, STEPS, B, max_gt=8), RolloutRecorder(STEPS, B, DEV), HistoryCache(B, STEPS + 1, H, DEV)
            feed = _HostFeed(tab, nav, store.max_ob_len) if name == "host" else ObsEpisodes(store, nav)
            step = _make_step(agent, lang, b, nav, rec, cache, feed, sids)
            call = None
            if name == "graph":
                gi = GraphedInference(step, state=(rec.ended, rec.hist_len, *nav.state_tensors(), *feed.state_tensors(), cache.buf))
                call = lambda t, gi=gi: gi(("step", t), t)
            for which in ("one", "two"):
                _reset(which, graphs, cands, nav, rec, cache, feed, cls)
                runs[name, which] = _run(step, nav, rec, call)
                if name != "host":
                    assert int(feed.anomalies.item()) == 0
                    views = feed.views().cpu().numpy()
                    runs[name, which] += (views,)
            if name == "graph":
                assert len(gi.graphs) == STEPS                # (the second rollout replayed the first one's graphs)
    moved = sum(int((runs["host", w][0][t][2] >= 0).sum()) for w in ("one", "two") for t in range(STEPS))
    print(f"[obs rollout] {moved} moves in {2 * STEPS * 4} episode steps")
    assert moved >= 1, moved                                  # (the rollouts do walk)
    assert not torch.equal(runs["host", "one"][0][0][0], runs["host", "two"][0][0][0])
    for which in ("one", "two"):
        _same_rollout(runs["host", which], runs["device", which][:4], ("device", which))
        _same_rollout(runs["host", which], runs["graph", which][:4], ("graph", which))
        assert np.array_equal(runs["device", which][4], runs["graph", which][4])
