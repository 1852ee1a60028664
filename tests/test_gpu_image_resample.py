"""GPU half of the whole-view resample tests: `hamt_image_resample` bit for bit against PIL's outputs (tests/golden/
image_resample.npz; the numpy restatement is chained to the same fixture by test_image_resample.py), its output discipline and
argument checks, and the two paths built on it: feature extraction from raw renders and `build_image_store`."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import _image_resample_ref as R
import _vit_extract_ref as V
from _util import load_npz

pytestmark = pytest.mark.gpu
TOL = {"fp32": 1e-3, "bf16": 1e-2}                     # test_gpu_extract.py's own bounds
GUARD = 256


@functools.lru_cache(None)
def _golden():
    return load_npz("image_resample.npz")


def _rel(a, b):                                         # test_gpu_extract.py's _rel
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def _guarded(n, h, w, fill):
    """an output of n * h * w * 3 bytes inside a buffer pre-filled with `fill`, GUARD bytes behind it"""
    total = n * h * w * 3
    buf = torch.full((total + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[:total].view(n, h, w, 3)


class _RenderStore:
    """raw renders: uint8 (36, 480, 640, 3) random bytes made from the key"""

    def __init__(self):
        self._c = {}

    def get(self, key):
        if key not in self._c:
            g = np.random.Generator(np.random.PCG64([R.SEED, zlib.crc32(key.encode("ascii"))]))
            self._c[key] = g.integers(0, 256, (36, 480, 640, 3), dtype=np.uint8)
        return self._c[key]


_RENDERS = _RenderStore()


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name,filt", R.keys(), ids=lambda v: str(v))
def test_image_resample_equals_pil(name, filt):
    """three views in one launch, the middle one the fixture's; output pre-filled (0xAA, then 0x55: a byte that is never written
    shows under one of the two) with guard bytes behind it; then the same launch on a side stream"""
    from vln_hamt_amd.data.image_resample import image_resample
    from vln_hamt_amd.data.image_transform import resample_u8
    H, W, OH, OW, win, _ = R.CASES[name]
    views = R.batch_input(name, n=3, at=1)
    want = np.stack([resample_u8(views[0], (OH, OW), filt, win), _golden()[f"{name}/{filt}"], resample_u8(views[2], (OH, OW), filt, win)])
    src = torch.from_numpy(views).cuda()
    n, h, w = want.shape[:3]
    for fill in (0xAA, 0x55):
        buf, out = _guarded(n, h, w, fill)
        got = image_resample(src, (OH, OW), filt, win, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        bad = int((got.cpu().numpy() != want).sum())
        assert bad == 0, (name, filt, fill, bad)
        assert bool((buf[n * h * w * 3:] == fill).all())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = image_resample(src, (OH, OW), filt, win)
    side.synchronize()
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("H,W,OH,OW", [(48, 2000, 24, 1000), (24, 3000, 12, 1500), (24, 3300, 12, 1650), (40, 70, 40, 70)],
                         ids=["tile_8_rows", "tile_2_rows", "tile_1_row", "both_axes_unchanged"])
def test_image_resample_tile_heights(H, W, OH, OW):
    """wide views, whose column table and input rows leave room for 8 output rows per workgroup (137 238 bytes of LDS; 16 rows would
    need 185 286), for 2 (152 202) and for 1 (157 596; 2 rows would need 167 502 of 163 840), every one above the 64 KiB a launch gets
    without asking; and a view neither axis of which changes (a copy of the window).  The numpy restatement bit for bit."""
    from vln_hamt_amd.data.image_resample import image_resample
    from vln_hamt_amd.data.image_transform import resample_u8
    views = np.random.Generator(np.random.PCG64(R.SEED + 7)).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    win = (5, 3, OW - 9, OH - 4)
    want = resample_u8(views, (OH, OW), "lanczos", win)
    buf, out = _guarded(2, win[3], win[2], 0xAA)
    got = image_resample(torch.from_numpy(views).cuda(), (OH, OW), "lanczos", win, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want) and bool((buf[want.size:] == 0xAA).all())


def test_image_resample_refuses_bad_arguments():
    from vln_hamt_amd._lib import HamtError
    from vln_hamt_amd.data.image_resample import image_resample
    src = torch.zeros((2, 48, 64, 3), dtype=torch.uint8, device="cuda")
    buf, out = _guarded(2, 25, 33, 0xAA)
    with pytest.raises(HamtError, match="hamt_image_resample.*window"):
        image_resample(src, (25, 33), "bicubic", (10, 0, 33, 25), out=out)              # 10 + 33 columns of 33
    with pytest.raises(HamtError, match="hamt_image_resample.*window"):
        image_resample(src, (25, 33), "bicubic", (0, 0, 33, 0), out=out)                # empty
    with pytest.raises(HamtError, match="hamt_image_resample.*filter 9"):
        image_resample(src, (25, 33), 9, out=out)
    small = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    wbuf, wide = _guarded(1, 8, 60000, 0xAA)
    with pytest.raises(HamtError, match="hamt_image_resample.*LDS"):                    # the column table alone is 1.7 MB
        image_resample(small, (8, 60000), "bicubic", out=wide)
    with pytest.raises(HamtError, match="GPU"):
        image_resample(src.cpu(), (25, 33))
    torch.cuda.synchronize()
    assert bool((buf == 0xAA).all()) and bool((wbuf == 0xAA).all())                     # nothing was launched


# ---------------------------------------------------------------------------------------------- extraction from raw renders
def _extractor(prec, resize=None):
    from vln_hamt_amd.preprocess import build_feature_extractor
    return build_feature_extractor(checkpoint_file={"state_dict": V.state_dict("tiny")}, num_classes=V.CONFIGS["tiny"]["classes"],
                                   hamt_precision=prec, vit_kwargs=V.vit_kwargs("tiny"), resize=resize)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_extractor_on_raw_renders_equals_host_resize(prec):
    """Resize(248) + CenterCrop(224) on the device == the default extractor on the host-resized 248 x 330 views: the patch rows
    entering the backbone are the same bytes, so the features are the same bits"""
    from vln_hamt_amd.data.image_transform import resample_u8
    renders = _RENDERS.get("scanA_vp0")[[0, 17]]
    ex_raw, ex = _extractor(prec, "bicubic"), _extractor(prec)
    f_raw, l_raw = ex_raw(renders)
    f_ref, l_ref = ex(resample_u8(renders, (248, 330), "bicubic"))
    assert f_raw.shape == (2, V.CONFIGS["tiny"]["vit"]["embed_dim"]) and bool(torch.isfinite(f_raw).all())
    assert torch.equal(f_raw, f_ref) and torch.equal(l_raw, l_ref)
    stored = resample_u8(renders, (248, 330), "lanczos")               # views that are 248-short already take the old path
    assert torch.equal(ex_raw(stored)[0], ex(stored)[0])
    assert not torch.equal(ex(stored)[0], f_ref)                       # (and the two filters do give other features)
    with pytest.raises(ValueError, match="short side"):
        ex(renders)


def test_build_image_store_and_feature_file_from_raw_renders(tmp_path):
    from vln_hamt_amd.data.image_data import PanoImageStore
    from vln_hamt_amd.data.image_transform import resample_u8
    from vln_hamt_amd.data.r2r_data import ViewFeatureStore
    from vln_hamt_amd.preprocess import build_feature_file, build_image_store
    keys = ["%s_%s" % sv for sv in V.SCANVPS]
    # ---- the store: Lanczos to 248 x 330, read back through the reader
    out = str(tmp_path / "panos")
    assert build_image_store(_RENDERS, V.SCANVPS, out, batch_size=36, num_workers=2) == 2           # two batches: both staging slots
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in keys)
    store = PanoImageStore(out)
    for k in keys:
        blk = np.asarray(store.get(k))
        assert blk.dtype == np.uint8 and blk.shape == (36, 248, 330, 3)
        assert np.array_equal(blk, resample_u8(_RENDERS.get(k), (248, 330), "lanczos")), k
    # ---- the same through an LMDB-like environment, one batch of two panoramas
    class Env:
        def __init__(self):
            self.db, self.commits = {}, 0

        def begin(self, write=False):
            env = self

            class Txn:
                def put(self, key, value):
                    self.kv = (bytes(key), bytes(value))

                def get(self, key):
                    return env.db.get(bytes(key))

                def commit(self):
                    env.db[self.kv[0]] = self.kv[1]
                    env.commits += 1
            return Txn()
    env = Env()
    assert build_image_store(_RENDERS, V.SCANVPS, env=env, batch_size=72) == 2 and env.commits == 2
    for k in keys:
        assert np.array_equal(PanoImageStore(env=env).get(k), np.asarray(store.get(k))), k
    # ---- the feature file over the raw renders, batches of 7 views across the two panoramas
    for prec in ("fp32", "bf16"):
        ex = _extractor(prec, "bicubic")
        fts = str(tmp_path / f"fts_{prec}")
        assert build_feature_file(_RENDERS, V.SCANVPS, fts, ex, out_image_logits=True, batch_size=7, num_workers=2) == 2
        fs = ViewFeatureStore(fts)
        D = ex.feat_size
        for k in keys:
            blk = fs.get(k)
            f, l = ex(_RENDERS.get(k))                                  # the panorama alone, one batch of 36
            e_f, e_l = _rel(blk[:, :D], f.cpu()), _rel(blk[:, D:], l.cpu())
            print(f"[raw renders {prec} {k}] file vs one-panorama batches {e_f:.2e} / {e_l:.2e}")
            assert blk.shape == (36, D + ex.num_classes) and np.isfinite(blk).all() and e_f <= TOL[prec] and e_l <= TOL[prec]
