"""GPU: `IndexedBatch.to_device` -- one small H2D copy, the text unpack, ONE `hamt_pretrain_gather` launch over a `PretrainStore` -- against
the numpy restatement of the gather (tests/_device_batch_ref.py) and against the host pipeline's `PackedBatch.to_device` of the same
samples: every key, `None`-ness, dtype, shape and bit.  Same cases as tests/test_device_batches.py, then the real widths, refused
records, and the loader protocol."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _device_batch_ref as R  # noqa: E402

_state = {}


def _store(cfg):
    """one PretrainStore (and its host tables) per configuration and process"""
    from vln_hamt_amd.data import PretrainStore, build_pretrain_tables
    if cfg not in _state:
        _state[cfg] = (PretrainStore(R.nav_db(*cfg), "cuda"), build_pretrain_tables(R.nav_db(*cfg)))
    return _state[cfg]


def _prefill(t):
    """NaN in a float tensor, 0xFF bytes in any other"""
    if t.is_floating_point():
        return torch.full_like(t, float("nan"))
    return torch.full((t.numel() * t.element_size(),), 0xFF, dtype=torch.uint8, device=t.device).view(t.dtype).view(t.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", R.CONFIGS, ids=lambda c: f"pano{int(c[0])}-cand{int(c[1])}")
@pytest.mark.parametrize("task,idxs,seed", R.CASES, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, int) else str(v))
def test_kernel_equals_restatement_and_host_pipeline(cfg, task, idxs, seed):
    from vln_hamt_amd import data as D
    store, tb = _store(cfg)
    host_ds, index_ds = R.datasets(R.nav_db(*cfg), task)
    host = D.COLLATE[task](R.draw(host_ds, idxs, seed)[0]).to_device("cuda")
    pb = D.INDEX_COLLATE[task](R.draw(index_ds, idxs, seed)[0])
    assert pb.store_id == store.id
    want = R.restate(tb, pb)
    got = pb.to_device("cuda")                                               # into fresh tensors
    assert all(v is None or isinstance(v, list) or v.is_cuda for v in got.values())
    R.assert_same_batch(got, want, "kernel vs restatement")
    R.assert_same_batch(got, host, "kernel vs host pipeline")
    static = {k: _prefill(v) for k, v in got.items() if torch.is_tensor(v)}  # into static inputs prefilled with NaN / 0xFF
    got2 = D.INDEX_COLLATE[task](R.draw(index_ds, idxs, seed)[0]).to_device("cuda", out=static)
    R.assert_same_batch(got2, host, "out= vs host pipeline")
    for k, v in got2.items():
        if not torch.is_tensor(v):
            continue
        assert v.data_ptr() == static[k].data_ptr(), k                       # written in place
        if v.is_floating_point():
            assert not torch.isnan(v).any(), k
        elif k != "txt_labels":                                              # (whose pad IS 0xFF bytes: -1)
            assert not (v.contiguous().view(-1).view(torch.uint8) == 0xFF).any(), k
    assert store.check() == 0


def _synthetic(NV=6, F=768, P=1000, A=4, C=3, NS=32, seed=3):
    """random tables at the real widths; step 29's viewpoint (row 2) has two candidates that share view 5"""
    rng = np.random.default_rng(seed)
    tb = {"feat": rng.standard_normal((NV, 36, F), dtype=np.float32), "prob": rng.random((NV, 36, P), dtype=np.float32),
          "ang36": rng.standard_normal((36, 36, A), dtype=np.float32), "cand_cnt": rng.integers(1, C + 1, NV).astype(np.int32),
          "cand_view": rng.integers(0, 36, (NV, C)).astype(np.int32), "cand_ang": rng.standard_normal((NV, C, 12, A), dtype=np.float32),
          "step_idx": np.stack([rng.integers(0, NV, NS), rng.integers(0, 36, NS), rng.integers(0, 37, NS), rng.integers(0, 4, NS)], 1).astype(np.int32),
          "step_val": rng.standard_normal((NS, A + 5), dtype=np.float32), "sp_targets": rng.standard_normal((36, 36, 2), dtype=np.float32)}
    tb["cand_cnt"][:] = 1
    tb["step_idx"][29, 0], tb["cand_cnt"][2], tb["cand_view"][2, :2] = 2, 2, 5
    return tb


def _upload(tb):
    from vln_hamt_amd.data import PretrainStore
    from vln_hamt_amd.data.device_store import TABLES
    return PretrainStore.from_tensors(*(torch.from_numpy(tb[k]).cuda() for k in TABLES))


def _launch_all(store, recs, Hmax, Omax, layout):
    """one launch with every output the kernel has -> {name: tensor}"""
    from vln_hamt_amd import ops
    B, F, A, P = recs.shape[0], store.F, store.A, store.P
    e = lambda dt, *s: _prefill(torch.empty(*s, dtype=dt, device="cuda"))
    f, i, b = torch.float32, torch.int64, torch.bool
    out = {"hist_img_fts": e(f, B, Hmax, F), "hist_ang_fts": e(f, B, Hmax, A), "hist_pano_img_fts": e(f, B, Hmax, 36, F),
           "hist_pano_ang_fts": e(f, B, Hmax, 36, A), "hist_img_probs": e(f, B, Hmax, P), "hist_mrc_masks": e(b, B, Hmax), "hist_masks": e(b, B, Hmax + 1),
           "hist_lens": e(i, B), "ob_img_fts": e(f, B, Omax, F), "ob_ang_fts": e(f, B, Omax, A), "ob_nav_types": e(i, B, Omax), "ob_masks": e(b, B, Omax),
           "ob_lens": e(i, B), "ob_action_viewindex": e(i, B), "ob_action_angles": e(f, B, 2), "ob_progress": e(f, B), "sp_anchor_idxs": e(i, B),
           "sp_targets": e(f, B, 36, 2)}
    return ops.pretrain_gather(store, torch.from_numpy(recs).cuda(), out, Hmax, Omax, layout)


def _ref_all(tb, recs, Hmax, Omax, layout):
    """the restatement of every output: the union over the tasks (the records of a launch serve them all)"""
    want, bad = {}, None
    for task in ("mrc", "sap", "sar", "sprel"):
        o, bad = R.gather_ref(tb, recs, task, layout, True, Hmax=Hmax, Omax=Omax, hist_none=False, has_ob=True)
        want.update(o)
    return want, bad


@pytest.mark.gpu
def test_synthetic_store_at_the_real_widths():
    """F = 768 and P = 1000 (the 16-byte path), history lengths 0, 1 and 29 with mask bits up to bit 28, the candidates-first layout with a
    shared view (Omax = 38), a killed view and a killed angle: one launch with every output, bit for bit against the restatement"""
    tb = _synthetic()
    store = _upload(tb)
    try:
        recs = np.zeros((3, 8), np.int32)
        recs[:, 1] = (0, 1, 29)
        recs[:, 2] = (1, 2, 0)
        recs[:, 3] = (0, 1, (1 << 28) | (1 << 13) | 1)
        recs[:, 4] = (0, 35, 17)
        want, bad = _ref_all(tb, recs, 29, 38, 1)
        assert bad == 0 and want["ob_lens"].tolist()[2] == 38 and want["hist_mrc_masks"][2, 28]
        R.assert_same_batch(_launch_all(store, recs, 29, 38, 1), want, "synthetic")
        assert store.check() == 0 and store.nbytes == sum(a.nbytes for a in tb.values())
    finally:
        store.close()


@pytest.mark.gpu
def test_records_outside_the_tables_give_zero_samples_and_are_counted():
    """an argument check, not a fault: the kernel compares every index with the table sizes before it loads through it"""
    tb = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _store((True, False))[1].items()}
    NV, NS = tb["feat"].shape[0], tb["step_idx"].shape[0]
    tb["step_idx"][NS - 1, 0] = NV + 5                                       # the last step row names a viewpoint row the store does not have
    store = _upload(tb)
    try:
        recs = np.zeros((5, 8), np.int32)
        recs[:, 0] = (0, 1 << 30, 4, NS - 3, 9)                              # sample 1: a step base far outside; sample 3: reaches the bad row
        recs[:, 1] = (2, 1, 3, 2, 1)
        recs[:, 4] = (3, 4, 5, 6, 7)
        want, bad = _ref_all(tb, recs, 3, 37, 0)
        assert bad == 2
        got = _launch_all(store, recs, 3, 37, 0)
        torch.cuda.synchronize()
        assert store.check() == 2 and store.check() == 0                     # counted once, reset by the read
        R.assert_same_batch(got, want, "bad records")                        # the neighbours are untouched
        for k, v in got.items():
            for b in (1, 3):
                z = v[b].cpu()
                if k == "hist_masks":
                    assert z.tolist() == [True, False, False, False], k
                elif k == "hist_lens":
                    assert int(z) == 1
                else:
                    assert not z.any(), (k, b)
            assert k == "hist_mrc_masks" or (v[0].cpu().any() and v[4].cpu().any()), k      # (no record carries a mask here)
    finally:
        store.close()


@pytest.mark.gpu
def test_loader_protocol_with_pinning():
    """build_dataloader(pin_mem) -> PrefetchLoader over the index-only dataset: three batches equal to the host pipeline's under equal seeds"""
    from vln_hamt_amd import data as D
    cfg = (True, True)
    store, _ = _store(cfg)
    opts = types.SimpleNamespace(train_batch_size=4, val_batch_size=4, local_rank=-1, n_workers=0, pin_mem=True)
    host_ds, index_ds = R.datasets(R.nav_db(*cfg), "sap")

    def three(ds, collate):
        loader, pre_epoch = D.build_dataloader("sap", ds, collate, False, opts)
        assert pre_epoch(1) is None
        random.seed(7)
        np.random.seed(7)
        out = []
        for batch in D.PrefetchLoader(loader, torch.device("cuda"), text_pack=True):
            out.append(batch)
            if len(out) == 3:
                break
        torch.cuda.synchronize()
        return out

    seen = []
    collate = lambda items: seen.append(D.sap_index_collate(items)) or seen[-1]
    want, got = three(host_ds, D.sap_collate), three(index_ds, collate)
    assert all(isinstance(pb, D.IndexedBatch) and pb.buf.is_pinned() and pb.nbytes < 4096 for pb in seen)
    for i, (g, w) in enumerate(zip(got, want)):
        R.assert_same_batch(g, w, f"batch {i}")
    assert store.check() == 0


def test_no_cpu_path():
    from vln_hamt_amd import data as D
    from vln_hamt_amd._lib import HamtError
    _, index_ds = R.datasets(R.nav_db(True, False), "sap")
    pb = D.sap_index_collate(R.draw(index_ds, [0, 3], 1)[0])
    with pytest.raises(HamtError):
        pb.to_device("cpu")
    with pytest.raises(HamtError):
        D.PretrainStore(R.nav_db(True, False), "cpu")
    with pytest.raises(HamtError):
        D.get_store(None)
