"""CPU: the image-input data pipeline.  The chain of equalities is PIL == numpy host transform (here, when PIL is installed) ==
committed fixture (here, always) == HIP kernel (tests/test_gpu_image_pipeline.py); then the parameter draws, the stores, the six
image task datasets against the feature-input ones, the packed batch layout, the ABI structs and the kernels' resources."""
import ctypes
import importlib.util
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from vln_hamt_amd.data import image_transform as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TINY = os.path.join(GOLD, "r2r_tiny")
DIMS = dict(image_feat_size=16, image_prob_size=10, angle_feat_size=4)
TOK = types.SimpleNamespace(cls_token_id=101, sep_token_id=102, mask_token_id=103, pad_token_id=0)


def _gen():
    spec = importlib.util.spec_from_file_location("gen_image_prep_golden", os.path.join(ROOT, "tools", "gen_image_prep_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _view(i, H=248, W=330):
    g = np.random.default_rng(100 + i)
    if i % 2:
        return g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([127 + 120 * np.sin(xx / (5.0 + i + c) + yy / (9.0 + 2 * c) + i) for c in range(3)], -1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. numpy == PIL
def test_numpy_transform_equals_pil_exactly():
    pytest.importorskip("PIL")
    pil_apply = _gen().pil_apply
    rng = random.Random(12)
    recs = [T.draw_eval_params()]
    while len(recs) < 31:
        recs.append(T.draw_train_params(rng))
    # make sure the required ground is covered whatever the draws were: extreme areas, narrow / low boxes, every order, both flips
    recs.append(T.make_record((7, 9, 330 - 7, 248 - 9), True, (0, 1, 2), (1.4, 0.6, 1.4)))
    recs.append(T.make_record((150, 100, 76, 86), False, (2, 1, 0), (0.6, 1.4, 0.6)))            # 0.08 of the area
    recs.append(T.make_record((10, 10, 120, 230), True, (1, 0, 2), (0.95, 1.05, 1.0)))           # narrower than 224
    recs.append(T.make_record((10, 10, 300, 150), False, (1, 2, 0), (1.2, 0.8, 1.3)))            # lower than 224
    recs.append(T.make_record((0, 0, 330, 248), False, (0, 2, 1), (0.7, 1.3, 0.9)))              # the whole view
    recs.append(T.make_record((20, 20, 200, 200), True, (2, 0, 1), (1.0, 1.0, 1.0)))
    orders = {T.unpack_order(int(r["order"])) for r in recs[1:]}
    assert orders >= set(T.ORDERS) and {int(r["flip"]) for r in recs} == {0, 1}
    assert any(r["width"] < 224 for r in recs) and any(r["height"] < 224 for r in recs)
    assert any(f < 1 for r in recs[1:] for f in (r["brightness"], r["contrast"], r["saturation"]))
    assert any(f > 1 for r in recs[1:] for f in (r["brightness"], r["contrast"], r["saturation"]))
    for i, r in enumerate(recs):
        v = _view(i)
        got, want = T.apply_view(v, r), pil_apply(v, r)
        assert got.dtype == np.uint8 and got.shape == (224, 224, 3)
        assert np.array_equal(got, want), (i, r, int((got != want).sum()), int(np.abs(got.astype(int) - want).max()))


# ------------------------------------------------------------------------------------------------ 2. fixture
def _fixture():
    from vln_hamt_amd.data.image_data import SyntheticPanoStore
    z = np.load(os.path.join(GOLD, "image_prep.npz"))
    recs = np.ascontiguousarray(z["recs"]).view(T.VIEW_DTYPE).reshape(-1)
    store = SyntheticPanoStore(int(z["store_seed"]))
    views = np.stack([store.get(str(k))[int(v)] for k, v in zip(z["keys"], z["view"])], 0)
    return z, views, recs


def test_fixture_equals_numpy_path():
    z, views, recs = _fixture()
    assert os.path.getsize(os.path.join(GOLD, "image_prep.npz")) < 1024 * 1024 and len(recs) >= 6
    for i, r in enumerate(recs):
        assert np.array_equal(T.apply_view(views[int(r["src"])], r), z["out"][i]), i


def test_fixture_matches_its_generator():
    pytest.importorskip("PIL")
    z = np.load(os.path.join(GOLD, "image_prep.npz"))
    fresh = _gen().build()
    assert set(fresh) == set(z.files)
    for k, v in fresh.items():
        assert np.array_equal(z[k], v), k


# ------------------------------------------------------------------------------------------------ 3. normalisation
def test_normalisation_is_torchs_expression_bitwise():
    u8 = np.random.default_rng(0).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    u8[0, 0, :, 0], u8[0, 1, :32, 0] = np.arange(224), np.arange(224, 256)      # every byte value at least once
    want = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)
    got = torch.from_numpy(T.normalize(u8))
    assert got.dtype == torch.float32 and got.shape == (2, 3, 224, 224)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    lut = torch.from_numpy(T.norm_table())
    assert torch.equal(lut.view(torch.int32), torch.arange(256, dtype=torch.uint8).float().div(255).sub(0.5).div(0.5).view(torch.int32))
    # zero slots are 0.0, not the normalised byte 0
    out = T.transform_views(u8[:, :224, :224], np.array([T.zero_record(), T.make_record(src=-1), T.make_record(src=1)], T.VIEW_DTYPE))
    assert not out[0].any() and not out[1].any() and np.array_equal(out[2], T.normalize(u8[1]))


# ------------------------------------------------------------------------------------------------ 4. draws
@pytest.mark.parametrize("make", [lambda s: random.Random(s), lambda s: np.random.default_rng(s)])
def test_train_draw_supports(make):
    H, W = 248, 330
    rng = make(3)
    recs = np.array([T.draw_train_params(rng, H, W) for _ in range(10000)], T.VIEW_DTYPE)
    l, t, w, h = (recs[k].astype(np.int64) for k in ("left", "top", "width", "height"))
    assert (w >= 1).all() and (h >= 1).all() and (l >= 0).all() and (t >= 0).all() and (l + w <= W).all() and (t + h <= H).all()
    # w = round(sqrt(area * ratio)), h = round(sqrt(area / ratio)) with area in [0.08, 1] H W and ratio in [3/4, 4/3]: each side is
    # within half a pixel of a real pair (w', h') that satisfies both bounds (the fallback box, the whole view here, does too)
    wl, wh, hl, hh = w - 0.5, w + 0.5, h - 0.5, h + 0.5
    assert (wh * hh >= 0.08 * H * W).all() and (wl * hl <= 1.0 * H * W).all()
    assert (wh / hl >= 3 / 4).all() and (wl / hh <= 4 / 3).all()
    for k in ("brightness", "contrast", "saturation"):
        assert (recs[k] >= np.float32(0.6)).all() and (recs[k] <= np.float32(1.4)).all() and recs[k].min() < 0.65 and recs[k].max() > 1.35
    assert {T.unpack_order(int(o)) for o in recs["order"]} == set(T.ORDERS)
    assert set(recs["flip"].tolist()) == {0, 1} and 0.45 < recs["flip"].mean() < 0.55
    assert not recs["zero"].any() and (recs["src"] == 0).all()
    again = np.array([T.draw_train_params(make(3), H, W) for _ in range(1)], T.VIEW_DTYPE)
    assert again[0] == recs[0]
    rng2 = make(3)
    assert np.array_equal(np.array([T.draw_train_params(rng2, H, W) for _ in range(50)], T.VIEW_DTYPE), recs[:50])
    assert (w.min() < 120) and (w * h).max() > 0.9 * H * W


def test_fallback_branch_and_eval_draw():
    rng = random.Random(5)
    fell = 0
    for _ in range(1000):
        box, fb = T.draw_box(rng, 100, 1000)
        assert 0 <= box[0] and box[0] + box[2] <= 1000 and 0 <= box[1] and box[1] + box[3] <= 100
        if fb:
            fell += 1
            assert box == ((1000 - 133) // 2, 0, 133, 100) and int(round(100 * 4 / 3)) == 133
    assert fell >= 1
    box, fb = T.draw_box(random.Random(1), 1000, 100)           # the tall case: ratio clamped to 3/4
    r = T.draw_eval_params(248, 330)
    assert (int(r["left"]), int(r["top"]), int(r["width"]), int(r["height"])) == (53, 12, 224, 224)
    assert (int(round((330 - 224) / 2)), int(round((248 - 224) / 2))) == (53, 12)
    assert int(r["flip"]) == 0 and T.unpack_order(int(r["order"])) == (3, 3, 3) and int(r["zero"]) == 0
    with pytest.raises(ValueError):
        T.draw_eval_params(300, 400)


# ------------------------------------------------------------------------------------------------ 5. stores and datasets
def _kw(**extra):
    d = dict(traj_files=[os.path.join(TINY, "traj.jsonl"), os.path.join(TINY, "traj2.jsonl")], img_ft_file=os.path.join(TINY, "img_fts.npz"),
             scanvp_cands_file=os.path.join(TINY, "scanvp_cands.json"), connectivity_dir=TINY, max_txt_len=12, max_act_len=6, **DIMS)
    d.update(extra)
    return d


def test_store_back_ends_agree(tmp_path):
    from vln_hamt_amd.data.image_data import PanoImageStore, SyntheticPanoStore
    syn = SyntheticPanoStore(3, height=40, width=52)
    keys = ["s1_a", "s1_b", "s2_a"]
    blocks = {k: syn.get(k) for k in keys}
    assert blocks["s1_a"].shape == (36, 40, 52, 3) and blocks["s1_a"].dtype == np.uint8
    assert np.array_equal(SyntheticPanoStore(3, height=40, width=52).get("s1_b"), blocks["s1_b"])       # deterministic in (seed, key)
    assert not np.array_equal(blocks["s1_a"], blocks["s1_b"]) and not np.array_equal(SyntheticPanoStore(4, height=40, width=52).get("s1_a"), blocks["s1_a"])
    assert len(np.unique(blocks["s1_a"])) > 100
    d = tmp_path / "npy"
    d.mkdir()
    for k, v in blocks.items():
        np.save(d / f"{k}.npy", v)
    np.savez(tmp_path / "views.npz", **blocks)

    class Txn:                                                   # stand-in for lmdb: the module is not installed here
        def get(self, key):
            assert isinstance(key, bytes)
            k = key.decode("ascii")
            return blocks[k].tobytes() if k in blocks else None

    class Env:
        def begin(self):
            return Txn()
    stores = [PanoImageStore(str(d), 40, 52), PanoImageStore(str(tmp_path / "views.npz"), 40, 52), PanoImageStore(env=Env(), height=40, width=52)]
    for s in stores:
        for k in keys:
            assert np.array_equal(s.get(k), blocks[k]), (s.kind, k)
    import pickle
    st = stores[0]
    st.get("s1_a")
    assert pickle.loads(pickle.dumps(st))._h is None              # handles are not shared across workers
    with pytest.raises(KeyError):
        stores[2].get("nope")
    with pytest.raises(ValueError):
        PanoImageStore(str(d), 41, 52).get("s1_a")
    (tmp_path / "db.lmdb").mkdir()
    try:
        import lmdb  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="lmdb"):
            PanoImageStore(str(tmp_path / "db.lmdb")).get("s1_a")


def _datasets(image):
    from vln_hamt_amd import data as D
    if image:
        db = D.MultiStepNavImageData(img_db=D.SyntheticPanoStore(1, height=64, width=80), is_training=True, rng=random.Random(77), **_kw())
        return db, {"mlm": D.MlmImageDataset(db, TOK), "mrc": D.MrcImageDataset(db, TOK, 0.5), "itm": D.ItmImageDataset(db, TOK),
                    "sap": D.SapImageDataset(db, TOK, 0.3, 0.43), "sar": D.SarImageDataset(db, TOK, 0.3, 0.43),
                    "sprel": D.SprelImageDataset(db, TOK, 0.3, 0.43)}
    db = D.MultiStepNavData(**_kw())
    return db, {"mlm": D.MlmDataset(db, TOK), "mrc": D.MrcDataset(db, TOK, 0.5), "itm": D.ItmDataset(db, TOK),
                "sap": D.SapDataset(db, TOK, 0.3, 0.43), "sar": D.SarDataset(db, TOK, 0.3, 0.43), "sprel": D.SprelDataset(db, TOK, 0.3, 0.43)}


FEATURE_KEYS = {"hist_img_fts", "hist_pano_img_fts", "ob_img_fts"}
IMAGE_KEYS = {"hist_images", "hist_pano_images", "ob_images", "ob_v_exists", "image_views"}


@pytest.mark.parametrize("task", ["mlm", "mrc", "itm", "sap", "sar", "sprel"])
def test_image_datasets_follow_the_feature_datasets(task):
    """same seeds -> every non-image key equals the feature-input dataset's (which tests/test_data_pipeline.py pins to the reference);
    the kill draws are the reference's (image_tasks.py:180-187), replayed by hand"""
    fdb, fsets = _datasets(False)
    idb, isets = _datasets(True)
    assert len(fsets[task]) == len(isets[task])
    n_killed_v = n_killed_a = 0
    for i in range(len(fsets[task])):
        random.seed(1000 + i); np.random.seed(2000 + i)
        f = fsets[task][i]
        random.seed(1000 + i); np.random.seed(2000 + i)
        g = isets[task][i]
        assert set(f) - FEATURE_KEYS == set(g) - IMAGE_KEYS, (set(f) ^ set(g))
        assert IMAGE_KEYS - {"ob_images", "ob_v_exists"} <= set(g)
        for k in set(f) - FEATURE_KEYS:
            a, b = f[k], g[k]
            if task == "mrc" and k == "hist_mrc_masks":
                assert torch.equal(a, b)
            elif torch.is_tensor(a):
                assert a.dtype == b.dtype and torch.equal(a, b), k
            else:
                assert np.array_equal(np.asarray(a), np.asarray(b)), k
        T_ = int(g["hist_lens"])
        ref = (idb.traj_step_refer if task in ("sap", "sar", "sprel") else idb.traj_refer)[i]
        vidx = idb.traj_data[ref[0]]["path_viewindex"]
        assert g["hist_pano_images"].shape == (T_, 36) and g["hist_images"].shape == (T_,) and g["hist_pano_images"].dtype == T.VIEW_DTYPE
        for t in range(T_):
            assert g["hist_images"][t] == g["hist_pano_images"][t, vidx[t]]              # THE record of the panorama's view
            assert np.array_equal(g["hist_pano_images"][t]["src"], t * 36 + np.arange(36))
            assert len({r.tobytes() for r in g["hist_pano_images"][t]}) == 36              # one independent draw per view
        assert len(g["image_views"]) == T_ + (task in ("sap", "sar", "sprel"))
        assert all(v.shape == (36, 64, 80, 3) and v.dtype == np.uint8 for v in g["image_views"])
        if "ob_images" in g:
            r = random.Random(1000 + i)                                                    # image_tasks.py:180-187 by hand
            v_exists = not (r.random() < 0.3)
            a_killed = v_exists and r.random() < 0.43
            assert g["ob_v_exists"] is v_exists and g["ob_lens"] == 37 and g["ob_images"].shape == (36,)
            assert bool(g["ob_images"]["zero"].all()) == (not v_exists) and bool(g["ob_images"]["zero"].any()) == (not v_exists)
            assert bool((g["ob_ang_fts"] == 0).all()) == a_killed
            assert np.array_equal(g["ob_images"]["src"], T_ * 36 + np.arange(36))
            assert bool((f["ob_img_fts"] == 0).all()) == (not v_exists)
            n_killed_v += not v_exists
            n_killed_a += a_killed
    if task in ("sap", "sar", "sprel"):
        assert n_killed_v > 0 and n_killed_a > 0


def test_validation_subsampling_and_eval_records():
    from vln_hamt_amd import data as D
    np.random.seed(5)
    db = D.MultiStepNavImageData(img_db=D.SyntheticPanoStore(1), is_training=False, **_kw())
    np.random.seed(5)
    n = len(db.traj_data)
    want_refer, want_step = [], []
    for sel in np.random.permutation(n):                       # image_data.py:82-93
        item = db.traj_data[sel]
        pl = min(len(item["path"]), 5)
        j = np.random.randint(len(item["instr_encodings"]))
        t = np.random.randint(pl)
        want_refer.append((sel, j, pl))
        want_step.append((sel, j, t))
    assert db.traj_refer == want_refer and db.traj_step_refer == want_step and len(db.traj_refer) == n
    out = db.get_input(*db.traj_refer[0], return_ob=False)
    assert out["hist_pano_images"].shape[0] == db.traj_refer[0][2]
    r = out["hist_pano_images"][0, 5]
    assert (int(r["left"]), int(r["top"]), int(r["width"]), int(r["height"]), int(r["flip"])) == (53, 12, 224, 224, 0)


# ------------------------------------------------------------------------------------------------ 6. layout, ABI, resources
def test_packed_image_batch_layout():
    from vln_hamt_amd import data as D
    _, isets = _datasets(True)
    random.seed(3); np.random.seed(3)
    items = [isets["sap"][i] for i in (0, 4, 9, 13)]
    pb = D.sap_image_collate(items)
    assert isinstance(pb, D.PackedImageBatch) and isinstance(pb, D.PackedBatch)
    assert pb.buf.dtype == torch.uint8 and pb.buf.dim() == 1
    offs = [o for o, *_ in pb.fields.values()] + [o for o, *_ in pb.per_sample.values()] + list(pb.prefix_off.values()) + \
        [o for o, *_ in pb.image.values()] + [pb.views_off, pb.tail_off]
    assert all(o % 64 == 0 for o in offs), offs
    H, W = pb.view_hw
    assert (H, W) == (64, 80) and pb.views_off + pb.n_src * H * W * 3 <= pb.buf.numel()
    hist = [int(x["hist_lens"]) for x in items]
    kept_ob = sum(bool(x["ob_v_exists"]) for x in items)
    assert pb.n_src == 36 * (sum(hist) + kept_ob)                 # killed observations do not cross PCIe
    Tmax = max(hist)
    assert pb.image["hist_images"][1:] == (4 * Tmax, (4, Tmax)) and pb.image["hist_pano_images"][1:] == (4 * Tmax * 36, (4, Tmax, 36))
    assert pb.image["ob_images"][1:] == (4 * 36, (4, 36))
    recs = pb.host_records("hist_pano_images").reshape(4, Tmax, 36)
    views = pb.host_views()
    for b, x in enumerate(items):
        for t in range(Tmax):
            if t >= hist[b]:
                assert (recs[b, t]["zero"] == 1).all() and (recs[b, t]["src"] == -1).all()
            else:
                for v in (0, 17, 35):
                    assert np.array_equal(views[recs[b, t, v]["src"]], x["image_views"][t][v])
                    assert recs[b, t, v]["left"] == x["hist_pano_images"][t, v]["left"]
    assert "image_views" not in pb.lists and "hist_images" not in pb.lists
    assert type(pb.pin_memory() if torch.cuda.is_available() else pb) is D.PackedImageBatch
    with pytest.raises(Exception):
        pb.to_device("cpu")                                       # no CPU path for the collation kernels: loud


def test_image_structs_match_header():
    from vln_hamt_amd import _lib
    assert ctypes.sizeof(_lib.ImageView) == 48 == T.VIEW_DTYPE.itemsize
    for name, _ in _lib.ImageView._fields_:
        assert getattr(_lib.ImageView, name).offset == T.VIEW_DTYPE.fields[name][1], name
    assert [n for n, _ in _lib.ImageView._fields_] == list(T.VIEW_DTYPE.names)
    assert ctypes.sizeof(_lib.ImagePrepDesc) == 8 * 4 and _lib.ImagePrepDesc.layout.offset == 16 and _lib.ImagePrepDesc.Rpad.offset == 28
    hdr = open(os.path.join(ROOT, "include", "hamt.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*hamt_image_view;", hdr)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == list(T.VIEW_DTYPE.names), fields
    m = re.search(r"typedef struct \{([^}]*)\}\s*hamt_image_prep_desc;", hdr)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == [n for n, _ in _lib.ImagePrepDesc._fields_], fields
    assert (_lib.JIT_BRIGHTNESS, _lib.JIT_CONTRAST, _lib.JIT_SATURATION, _lib.JIT_SKIP) == (T.OP_BRIGHTNESS, T.OP_CONTRAST, T.OP_SATURATION, T.OP_SKIP)
    for name, val in (("HAMT_JIT_SKIP", 3), ("HAMT_IMAGE_PATCHES", 1), ("HAMT_WS_IMAGE_PREP", 9)):
        assert re.search(rf"{name} = {val}\b", hdr), name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert _lib.workspace_bytes(_lib.WS_IMAGE_PREP, 3) == 3 * (224 * 224 * 3 + 64) and _lib.workspace_bytes(_lib.WS_IMAGE_PREP, 0) == 0


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="ROCm LLVM tools not installed")
def test_prep_kernels_do_not_spill(tmp_path):
    from test_kernel_resources import READELF, _code_objects
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = []
    for co in _code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or "image_prep" not in name.group(1):
                continue
            spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
            sspill = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
            seen.append(name.group(1))
            assert spill == 0 and sspill == 0 and scratch == 0, (name.group(1), spill, sspill, scratch)
    assert len(seen) == 4, seen                 # the resize kernel and three instantiations of the store kernel
