"""CPU: the device-resident pretraining batches without a device.  `build_pretrain_tables` + the index-only datasets' records, pushed
through a numpy restatement of `hamt_pretrain_gather` (tests/_device_batch_ref.py), must reproduce the host pipeline's collated batch
bit for bit on tests/golden/r2r_tiny (F = 16, P = 10, A = 4): six tasks, both observation layouts, with and without panorama history,
batches of 1 and 5, equal seeds on both sides.  tests/test_gpu_device_batches.py holds the kernel to the same restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _device_batch_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def tables():
    from vln_hamt_amd.data import build_pretrain_tables
    return {cfg: build_pretrain_tables(R.nav_db(*cfg)) for cfg in R.CONFIGS}


def _both(cfg, task, idxs, seed):
    """-> (host pipeline's PackedBatch, IndexedBatch, the two RNG end states) of one case"""
    from vln_hamt_amd import data as D
    host, index = R.datasets(R.nav_db(*cfg), task)
    hi, hs = R.draw(host, idxs, seed)
    xi, xs = R.draw(index, idxs, seed)
    return D.COLLATE[task](hi), D.INDEX_COLLATE[task](xi), hs, xs


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=lambda c: f"pano{int(c[0])}-cand{int(c[1])}")
@pytest.mark.parametrize("task,idxs,seed", R.CASES, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, int) else str(v))
def test_restated_gather_reproduces_the_host_batches(tables, cfg, task, idxs, seed):
    host_pb, index_pb, hs, xs = _both(cfg, task, idxs, seed)
    want = R.numpy_unpack(host_pb)
    got = R.restate(tables[cfg], index_pb)
    R.assert_same_batch(got, want, (cfg, task, seed))
    assert R.same_state(hs, xs), "the index-only dataset left python's / numpy's stream elsewhere than the host dataset"
    assert index_pb.nbytes < 4096 and not any(k.startswith(("hist_", "ob_")) for k in index_pb.fields)          # tokens and records only


def test_cases_cover_the_edges(tables):
    """read off the records themselves, so that a change of seeds or indices cannot silently lose an edge"""
    cfg = (True, False)
    tb, A = tables[cfg], R.DIMS["angle_feat_size"]
    recs = {(task, seed): _both(cfg, task, idxs, seed)[1] for task, idxs, seed in R.CASES}
    ob = [pb for (task, _), pb in recs.items() if task in R.OB_TASKS]
    assert any(pb.hist_none and pb.B > 1 for pb in ob) and any(pb.hist_none and pb.B == 1 for pb in ob)             # entirely at step 0
    assert any(not pb.hist_none and min(pb.hist_lens) == 0 < max(pb.hist_lens) for pb in ob)                      # mixed
    allr = np.concatenate([pb.host_records() for pb in recs.values()], 0)
    flags = np.concatenate([pb.host_records()[:, 2] for pb in ob])
    assert (flags & 1).any() and (flags & 2).any() and (flags == 0).any()                                         # kill_v, kill_a, neither
    stop_in_hist = [any(not tb["step_val"][b + s, :A].any() for s in range(t)) for b, t in allr[:, :2]]
    assert any(stop_in_hist) and not all(stop_in_hist)                                                            # the STOP step's zero angle
    base_long = int(tb["traj_base"][1])                  # trajectory 1: six viewpoints on file, five steps under max_act_len = 6
    assert len(R.nav_db(*cfg).traj_data[1]["path"]) == 6 and tb["traj_base"][2] - base_long == 5
    assert any(b == base_long and t == 5 for b, t in allr[:, :2])                                                 # its whole (cut) history
    assert any(b == base_long and t == 4 for b, t in np.concatenate([pb.host_records()[:, :2] for pb in ob]))     # observed at the cut
    # an MRC item where no view was picked: replay its draws
    task, idxs, seed = next(c for c in R.CASES if c[0] == "mrc" and len(c[1]) == 1)
    n = int(recs[task, seed].host_records()[0, 1])
    np.random.seed(seed)
    assert all(np.random.rand() >= R.MRC_PROB for _ in range(n))
    assert int(recs[task, seed].host_records()[0, 3]) == 1 << np.random.randint(n)                                # the forced one alone
    assert any(bin(int(m) & 0xFFFFFFFF).count("1") > 1 for m in allr[:, 3])                                       # and ordinary masks


def test_softmax_table_equals_the_per_sample_softmax(tables):
    """prob[row, view] is what get_history_feature(..., return_img_probs=True) computes per sample -- bit for bit, also at P = 1000"""
    from vln_hamt_amd.data.r2r_data import softmax
    db, tb = R.nav_db(True, False), tables[True, False]
    for i, td in enumerate(db.traj_data):
        path = td["path"][:db.max_act_len - 1]
        t = len(path)
        want = db.get_history_feature(td["scan"], path, td["path_viewindex"], td["rel_act_angles"], t, return_img_probs=True)[4]
        rows = tb["step_idx"][tb["traj_base"][i]:tb["traj_base"][i] + t]
        got = tb["prob"][rows[:, 0], rows[:, 1]]
        assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), i
    rng = np.random.default_rng(5)
    F, P = 16, 1000
    blocks = (rng.standard_normal((7, 36, F + P)) * 3).astype(np.float32)
    table = np.stack([softmax(np.ascontiguousarray(b[:, F:F + P])) for b in blocks], 0)          # build_pretrain_tables' expression
    for t in (1, 3, 7):
        vidx = rng.integers(0, 36, t)
        want = softmax(blocks[:t][np.arange(t), vidx, F:])                                       # get_history_feature's expression
        assert np.array_equal(table[np.arange(t), vidx].view(np.uint32), want.view(np.uint32)), t


def test_the_restatement_sees_every_record_field(tables):
    """a comparison that a wrong record or table entry cannot fail shows nothing: perturb each class of field, expect a different batch"""
    cfg = (True, False)
    tb = tables[cfg]

    def differs(task, recs, recs2, tb2=None, **kw):
        a, _ = R.gather_ref(tb, recs, task, 0, True, **kw)
        b, _ = R.gather_ref(tb2 or tb, recs2, task, 0, True, **kw)
        return [k for k in a if a[k] is not None and not np.array_equal(a[k], b[k])]

    mrc = next(_both(cfg, t, i, s)[1] for t, i, s in R.CASES if t == "mrc" and len(i) == 5).host_records().copy()
    dropped = mrc.copy()
    bit = int(mrc[0, 3]) & -int(mrc[0, 3])
    dropped[0, 3] &= ~bit                                                                        # a dropped mask bit
    assert set(differs("mrc", mrc, dropped)) == {"hist_img_fts", "hist_pano_img_fts", "hist_mrc_masks"}
    sprel = next(_both(cfg, t, i, s)[1] for t, i, s in R.CASES if t == "sprel" and len(i) == 5 and s == 62).host_records().copy()
    moved = sprel.copy()
    moved[2, 4] = (moved[2, 4] + 1) % 36                                                         # anchor + 1
    assert set(differs("sprel", sprel, moved)) == {"sp_anchor_idxs", "sp_targets"}
    for bit_, field in ((1, "ob_img_fts"), (2, "ob_ang_fts")):                                   # a flipped kill flag
        flipped = sprel.copy()
        flipped[2, 2] ^= bit_
        assert set(differs("sprel", sprel, flipped)) == {field}, bit_
    wrong = dict(tb, step_idx=tb["step_idx"].copy())
    s = int(sprel[2, 0])                                                                         # a wrong view in the sample's first history step
    wrong["step_idx"][s, 1] = (wrong["step_idx"][s, 1] + 1) % 36
    assert {"hist_img_fts", "hist_pano_ang_fts"} <= set(differs("sprel", sprel, sprel, wrong))
    later = sprel.copy()
    later[2, 1] -= 1                                                                             # one step earlier: another observation
    assert {"ob_img_fts", "hist_lens", "hist_masks"} <= set(differs("sprel", sprel, later, Hmax=4))
    off = sprel.copy()
    off[2, 0] += 1                                                                               # a wrong step base
    assert {"ob_img_fts", "hist_img_fts"} <= set(differs("sprel", sprel, off))


def test_tables_refuse_what_the_kernel_cannot_carry(tmp_path):
    import copy
    from vln_hamt_amd._lib import HamtError
    from vln_hamt_amd.data import PretrainStore, build_pretrain_tables
    db = copy.copy(R.nav_db(True, False))
    db.traj_data = copy.deepcopy(db.traj_data)
    db.max_act_len = 40                                                                          # (the class caps at 30; a future cap above 33 must not pass)
    db.traj_data[0]["path"] = (db.traj_data[0]["path"] * 9)[:34]
    with pytest.raises(HamtError, match="history steps"):
        build_pretrain_tables(db)
    db = copy.copy(R.nav_db(True, False))
    db.scanvp_cands = dict(db.scanvp_cands, scanA_a00={f"n{i}": [i % 36, 1.0, 0.0, 0.0] for i in range(65)})
    with pytest.raises(HamtError, match="candidates"):
        build_pretrain_tables(db)
    db = copy.copy(R.nav_db(True, False))
    db.traj_data = copy.deepcopy(db.traj_data)
    db.traj_data[0]["path"][1] = "nowhere"
    db.scanvp_cands = dict(db.scanvp_cands, scanA_nowhere={})
    with pytest.raises(HamtError, match="no view features"):
        build_pretrain_tables(db)
    with pytest.raises(HamtError, match="no CPU path"):
        PretrainStore(R.nav_db(True, False), "cpu")
    with pytest.raises(HamtError, match="no CPU path"):
        PretrainStore(R.nav_db(True, False), None)
