"""GPU half of the view-feature extraction tests: `hamt_attn_cls_fwd` at op level against float64 (cases and bound of
tests/_attn_cls_ref.py, shown sound by test_attn_cls_ref.py), the backbone's cls-only tail against the reference golden and against
the full last block, and `build_feature_file` end to end through the writer and `ViewFeatureStore`."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _attn_cls_ref as A
import _vit_extract_ref as R
from _util import load_npz

pytestmark = pytest.mark.gpu
TOL = {"fp32": 1e-3, "bf16": 1e-2}                     # test_vit.py's own bounds


def _rel(a, b):                                         # test_vit.py's _rel
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


@functools.lru_cache(None)
def _golden():
    return load_npz("vit_extract.npz")


@functools.lru_cache(None)
def _model(tag, prec):
    from vln_hamt_amd.model.vision_transformer import VisionTransformer
    m = VisionTransformer(**R.vit_kwargs(tag), hamt_precision=prec, num_classes=R.CONFIGS[tag]["classes"])
    m.load_state_dict(R.state_dict(tag), strict=True)
    return m.cuda().eval()


@functools.lru_cache(None)
def _images(tag):
    return torch.from_numpy(R.images(tag)).cuda()


# ---------------------------------------------------------------------------------------------- the kernel
def _device_case(c):
    """q / k / v as strided views into NaN-filled buffers with the case's padded row strides: [q | pad], [k | v | pad]"""
    dt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
    qb = torch.full((A.N_IMG, A.H + c["pad_q"]), float("nan"), dtype=dt, device="cuda")
    kvb = torch.full((A.N_IMG * c["Sk"], 2 * A.H + c["pad_kv"]), float("nan"), dtype=dt, device="cuda")
    qb[:, :A.H] = torch.from_numpy(c["q"]).to(dt)
    kvb[:, :A.H] = torch.from_numpy(c["k"]).to(dt)
    kvb[:, A.H:2 * A.H] = torch.from_numpy(c["v"]).to(dt)
    return qb[:, :A.H], kvb[:, :A.H], kvb[:, A.H:2 * A.H]


@pytest.mark.parametrize("c", A.cases(), ids=lambda c: c["name"].replace(" ", "_"))
def test_attn_cls_against_float64(c):
    from vln_hamt_amd import ops
    q, k, v = _device_case(c)
    assert np.array_equal(q.float().cpu().numpy(), c["q"]) and np.array_equal(v.float().cpu().numpy(), c["v"])      # identical inputs
    with torch.no_grad():
        o = ops.attn_cls(q, k, v, A.HEADS)
    torch.cuda.synchronize()
    e = A.errors(c, o.cpu().numpy())
    print(f"[attn_cls {c['name']}] worst error {e.max():.3f} units (bound {A.BOUND})")
    assert o.dtype == torch.float32 and o.shape == (A.N_IMG, A.H) and e.max() <= A.BOUND, (c["name"], e)


def test_attn_cls_refuses_more_than_256_keys():
    from vln_hamt_amd import _lib as L, ops
    Sk = 257
    q = torch.zeros(A.N_IMG, A.H, device="cuda")
    kv = torch.zeros(A.N_IMG * Sk, 2 * A.H, device="cuda")
    out = torch.full((A.N_IMG, A.H), 7.0, device="cuda")
    for sk, want in ((Sk, -2), (0, -1)):                                                     # HAMT_ERR_UNSUPPORTED / HAMT_ERR_ARG
        d = L.AttnDesc(A.N_IMG, A.HEADS, 1, sk, 64, A.H, 2 * A.H, 2 * A.H, A.H, L.HAMT_F32, L.HAMT_F32, 0.125, 0.0, 0, L.PREC_F32)
        rc = L.load().hamt_attn_cls_fwd(C.byref(d), ops._p(q), ops._p(kv[:, :A.H]), ops._p(kv[:, A.H:]), ops._p(out), ops._stream())
        assert rc == want, (sk, rc)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                          # nothing was launched
    with pytest.raises(L.HamtError, match="hamt_attn_cls_fwd"), torch.no_grad():
        ops.attn_cls(q, kv[:, :A.H], kv[:, A.H:], A.HEADS)
    x = torch.zeros(A.N_IMG, A.H, device="cuda", requires_grad=True)
    with pytest.raises(L.HamtError, match="forward-only"):                                   # no backward: never inside a recorded graph
        ops.attn_cls(x, kv[:A.N_IMG * 5, :A.H], kv[:A.N_IMG * 5, A.H:], A.HEADS)


# ---------------------------------------------------------------------------------------------- the backbone
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["tiny", "b16"])
def test_cls_tail_matches_reference_golden_and_full_block(tag, prec):
    model, imgs = _model(tag, prec), _images(tag)
    with torch.no_grad():
        tail = model.forward_features(imgs, cls_tail=True)
        full = model.forward_features(imgs)
        same = model(imgs)
    want = _golden()[f"{tag}/feats"]
    e_t, e_f, e_tf = _rel(tail, want), _rel(full, want), _rel(tail, full.cpu())
    print(f"[vit {tag} {prec}] cls_tail vs golden {e_t:.2e}, full vs golden {e_f:.2e}, cls_tail vs full {e_tf:.2e}")
    assert tail.shape == full.shape == want.shape and tail.dtype == torch.float32
    assert torch.equal(full, same)                                   # forward stays forward_features
    assert e_t <= TOL[prec] and e_f <= TOL[prec] and e_tf <= TOL[prec]


def test_cls_tail_raises_outside_a_no_grad_eval_forward():
    from vln_hamt_amd._lib import HamtError
    from vln_hamt_amd.model.vision_transformer import VisionTransformer
    m = VisionTransformer(**R.vit_kwargs("tiny"), hamt_precision="bf16", drop_rate=0.1, attn_drop_rate=0.1)
    m.load_state_dict({k: v for k, v in R.state_dict("tiny").items() if not k.startswith("head.")}, strict=True)
    m = m.cuda()
    imgs = _images("tiny")[:2]
    m.train()
    with pytest.raises(HamtError, match=r"train\(\) mode"), torch.no_grad():
        m.forward_features(imgs, cls_tail=True)
    m.eval()
    with pytest.raises(HamtError, match="grad mode"):
        m.forward_features(imgs, cls_tail=True)
    m.blocks[-1].mlp.drop.train()                                     # one dropout of the last block switched on by hand
    with pytest.raises(HamtError, match="train|active"), torch.no_grad():
        m.forward_features(imgs, cls_tail=True)
    m.eval()
    with torch.no_grad():
        a, b = m.forward_features(imgs, cls_tail=True), m.forward_features(imgs)
    assert _rel(a, b.cpu()) <= TOL["bf16"]
    m.train()
    assert m.forward_features(imgs).requires_grad                     # the default path trains as before


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_cls_tail_uninitialised_memory_never_reaches_a_result(prec):
    """ViT-B/16, 3 images (591 token rows), the cls-only tail with every scratch / output buffer of the package pre-filled with NaN:
    the same features bit for bit (the pattern of test_vit_uninitialised_memory_never_reaches_a_result)."""
    from test_gpu_model import _NanScratch
    model = _model("b16", prec)
    g = torch.Generator().manual_seed(5)
    imgs = torch.randn(3, 3, 224, 224, generator=g).cuda()
    res = []
    for poisoned in (False, True):
        with _NanScratch(poisoned), torch.no_grad():
            res.append(model.forward_features(imgs, cls_tail=True).clone())
            torch.cuda.synchronize()
    assert bool(torch.isfinite(res[1]).all()) and torch.equal(res[0], res[1])


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_build_feature_file_end_to_end(tmp_path, prec):
    from vln_hamt_amd.data.image_data import SyntheticPanoStore
    from vln_hamt_amd.data.r2r_data import ViewFeatureStore
    from vln_hamt_amd.preprocess import build_feature_extractor, build_feature_file
    c = R.CONFIGS["tiny"]
    D, Cn = c["vit"]["embed_dim"], c["classes"]
    sd = R.state_dict("tiny")
    ex = build_feature_extractor(checkpoint_file={"state_dict": sd}, num_classes=Cn, hamt_precision=prec, vit_kwargs=R.vit_kwargs("tiny"))
    assert ex.cls_tail and ex.has_head
    store = SyntheticPanoStore(R.STORE_SEED)
    out = str(tmp_path / "fts")
    assert build_feature_file(store, R.SCANVPS, out, ex, out_image_logits=True, batch_size=7, num_workers=2) == 2   # 72 views: 10 batches of 7 + 2
    assert sorted(os.listdir(out)) == ["scanA_vp0.npy", "scanB_vp1.npy"]
    fs = ViewFeatureStore(out)
    W64, b64 = sd["head.weight"].double().numpy(), sd["head.bias"].double().numpy()
    gold = _golden()
    for k, (scan, vp) in enumerate(R.SCANVPS):
        blk = fs.get(f"{scan}_{vp}")
        assert np.load(os.path.join(out, f"{scan}_{vp}.npy")).dtype == np.float32 and blk.shape == (36, D + Cn) and np.isfinite(blk).all()
        fts, logits = ex(store.get(f"{scan}_{vp}"))                  # the panorama alone, one batch of 36
        assert fts.shape == (36, D) and logits.shape == (36, Cn) and fts.dtype == logits.dtype == torch.float32
        e_f, e_l = _rel(blk[:, :D], fts.cpu()), _rel(blk[:, D:], logits.cpu())
        want = blk[:, :D].astype(np.float64) @ W64.T + b64
        e_h = float(np.abs(blk[:, D:] - want).max() / np.abs(want).max())
        rows = [i for i, (kk, _) in enumerate(c["views"]) if kk == k]
        e_g = _rel(blk[[c["views"][i][1] for i in rows], :D], gold["tiny/feats"][rows])
        e_gl = _rel(blk[[c["views"][i][1] for i in rows], D:], gold["tiny/logits"][rows])
        print(f"[extract {prec} {scan}_{vp}] file vs one-panorama batches {e_f:.2e} / {e_l:.2e}, head vs float64 {e_h:.2e}, vs golden {e_g:.2e} / {e_gl:.2e}")
        assert e_f <= TOL[prec] and e_l <= TOL[prec] and e_h <= 1e-5 and e_g <= TOL[prec] and e_gl <= TOL[prec]
    out2 = str(tmp_path / "fts_only.npz")
    build_feature_file(store, R.SCANVPS, out2, ex, out_image_logits=False, batch_size=64)
    f2 = ViewFeatureStore(out2)
    for scan, vp in R.SCANVPS:
        b2 = f2.get(f"{scan}_{vp}")
        assert b2.shape == (36, D) and b2.dtype == np.float32 and _rel(b2, fs.get(f"{scan}_{vp}")[:, :D]) <= TOL[prec]
    with pytest.raises(ValueError, match="short side"):              # raw 480 x 640 renders need a real resize: out of scope, loudly
        ex(np.zeros((1, 480, 640, 3), np.uint8))
