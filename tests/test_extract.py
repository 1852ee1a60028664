"""CPU half of the view-feature extraction tests (vln_hamt_amd/preprocess): the golden made by the reference's own VisionTransformer
+ head against the oracle composition, the writer -> reader round trip, the viewpoint list, the checkpoint layouts, and the opt-in
classifier head leaving the default module tree alone."""
import os

import numpy as np
import pytest
import torch

import _vit_extract_ref as R
from _util import GOLDEN, load_npz


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("tag", ["tiny", "b16"])
def test_oracle_composition_matches_reference_golden(tag):
    """vit_forward_features + feats @ W.T + b reproduces the reference's forward_features / head (eval mode) at the 1e-6 of
    test_vit_oracle_matches_reference_goldens"""
    from oracle.hamt_oracle import vit_forward_features
    store = load_npz("vit_extract.npz")
    if tag == "b16":
        torch.set_num_threads(8)
    sd = R.state_dict(tag)
    with torch.no_grad():
        feats = vit_forward_features(sd, R.vit_config(tag), torch.from_numpy(R.images(tag)))
        logits = feats @ sd["head.weight"].t() + sd["head.bias"]
    c = R.CONFIGS[tag]
    assert store[f"{tag}/feats"].shape == (len(c["views"]), c["vit"]["embed_dim"]) and store[f"{tag}/logits"].shape == (len(c["views"]), c["classes"])
    assert _rel(feats, store[f"{tag}/feats"]) <= 1e-6 and _rel(logits, store[f"{tag}/logits"]) <= 1e-6


def test_golden_holds_outputs_only():
    store = load_npz("vit_extract.npz")
    assert sorted(store) == ["b16/feats", "b16/logits", "tiny/feats", "tiny/logits"]
    assert os.path.getsize(os.path.join(GOLDEN, "vit_extract.npz")) < 64 * 1024


@pytest.mark.parametrize("kind", ["dir", "npz"])
def test_writer_reader_round_trip_is_bitwise(tmp_path, kind):
    from vln_hamt_amd.data.r2r_data import ViewFeatureStore
    from vln_hamt_amd.preprocess import ViewFeatureWriter
    rng = np.random.Generator(np.random.PCG64(4))
    blocks = {("scanA", "vp0"): rng.standard_normal((36, 128 + 40), dtype=np.float32), ("scanB", "vp_1"): rng.standard_normal((36, 128 + 40), dtype=np.float32)}
    blocks[("scanA", "vp0")][3, 5] = np.float32(1e-42)          # a denormal and a signed zero survive too
    blocks[("scanB", "vp_1")][0, 0] = np.float32(-0.0)
    path = str(tmp_path / ("fts" if kind == "dir" else "sub/fts.npz"))
    with ViewFeatureWriter(path) as w:
        for (s, v), b in blocks.items():
            w.put(s, v, b)
    st = ViewFeatureStore(path)
    assert st.kind == ("npy_dir" if kind == "dir" else "npz")
    for (s, v), b in blocks.items():
        got = st.get(f"{s}_{v}")
        assert f"{s}_{v}" in st and got.dtype == np.float32 and got.shape == b.shape and got.tobytes() == b.tobytes()
    assert "scanA_nope" not in st


def test_hdf5_writer_is_loud_without_h5py(tmp_path):
    from vln_hamt_amd.preprocess import ViewFeatureWriter
    try:
        import h5py  # noqa: F401
    except ImportError:
        for name in ("f.hdf5", "f.h5"):
            with pytest.raises(ImportError, match="h5py is not installed"):
                ViewFeatureWriter(str(tmp_path / name))
            assert not os.path.exists(str(tmp_path / name))
        return
    from vln_hamt_amd.data.r2r_data import ViewFeatureStore
    b = np.arange(36 * 4, dtype=np.float32).reshape(36, 4)
    with ViewFeatureWriter(str(tmp_path / "f.hdf5")) as w:
        w.put("s", "v", b)
    import h5py
    with h5py.File(str(tmp_path / "f.hdf5"), "r") as f:
        assert dict(f["s_v"].attrs) == {"scanId": "s", "viewpointId": "v", "image_w": 640, "image_h": 480, "vfov": 60}
    assert ViewFeatureStore(str(tmp_path / "f.hdf5")).get("s_v").tobytes() == b.tobytes()


def test_load_viewpoint_ids_on_the_tiny_graphs():
    import json
    from vln_hamt_amd.preprocess import load_viewpoint_ids
    d = os.path.join(GOLDEN, "r2r_tiny")
    ids = load_viewpoint_ids(d)
    want = []
    for scan in ("scanA", "scanB"):                              # scans.txt order, then file order, `included` only
        want += [(scan, x["image_id"]) for x in json.load(open(os.path.join(d, f"{scan}_connectivity.json"))) if x["included"]]
    assert ids == want and ids[0] == ("scanA", "a00") and ("scanA", "excluded") not in ids and len({s for s, _ in ids}) == 2


def _build(ckpt, **kw):
    from vln_hamt_amd.preprocess import build_feature_extractor
    return build_feature_extractor(checkpoint_file=ckpt, num_classes=R.CONFIGS["tiny"]["classes"], vit_kwargs=R.vit_kwargs("tiny"), device="cpu", **kw)


def test_checkpoint_layouts(tmp_path):
    from vln_hamt_amd.preprocess import build_feature_extractor, build_feature_file
    sd = R.state_dict("tiny")
    backbone = {k: v for k, v in sd.items() if not k.startswith("head.")}
    with pytest.raises(ValueError, match="checkpoint_file is required"):
        build_feature_extractor(checkpoint_file=None)
    with pytest.raises(ValueError, match="unknown model_name"):
        build_feature_extractor("resnet152", checkpoint_file=sd)
    torch.save({"state_dict": sd}, str(tmp_path / "ref.pt"))           # the reference's layout, from a file
    layouts = {"reference": str(tmp_path / "ref.pt"), "bare": dict(sd),
               "pretrain": {**{"bert.vision_backbone." + k: v for k, v in backbone.items()}, "bert.embeddings.word_embeddings.weight": torch.zeros(3, 4)},
               "pretrain2": {"vision_backbone." + k: v for k, v in backbone.items()}}
    for name, ck in layouts.items():
        ex = _build(ck)
        got = ex.model.state_dict()
        assert ex.has_head == (name in ("reference", "bare")) and ex.feat_size == 128 and not ex.model.training, name
        assert set(got) == set(sd if ex.has_head else backbone), name
        for k, v in got.items():
            assert torch.equal(v, sd[k]), (name, k)
    ex = _build(layouts["pretrain"])
    assert ex.num_classes == 0
    with pytest.raises(ValueError, match="no classifier head"):       # asked for logits: refused before anything is read or written
        build_feature_file(None, [("scanA", "vp0")], str(tmp_path / "never"), ex, out_image_logits=True)
    assert not os.path.exists(str(tmp_path / "never"))
    with pytest.raises(ValueError, match=r"unknown keys \['blocks.0.stray.weight'\]"):
        _build({**sd, "blocks.0.stray.weight": torch.zeros(1)})
    short = dict(sd)
    del short["blocks.1.mlp.fc2.bias"]
    with pytest.raises(ValueError, match=r"missing keys \['blocks.1.mlp.fc2.bias'\]"):
        _build(short)


def test_default_backbone_has_no_head():
    from oracle.hamt_oracle import vit_param_shapes
    from vln_hamt_amd.model.vision_transformer import VisionTransformer
    c = R.vit_config("tiny")
    m0 = VisionTransformer(**R.vit_kwargs("tiny"))
    assert list(m0.state_dict()) == list(vit_param_shapes(c)) and not hasattr(m0, "head") and m0.num_classes == 0
    m1 = VisionTransformer(**R.vit_kwargs("tiny"), num_classes=40)
    assert list(m1.state_dict()) == list(vit_param_shapes(c)) + ["head.weight", "head.bias"] and m1.head.weight.shape == (40, 128)
    import inspect
    sig = inspect.signature(VisionTransformer.forward_features)
    assert sig.parameters["cls_tail"].default is False
