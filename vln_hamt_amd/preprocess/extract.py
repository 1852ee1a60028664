"""View-feature extraction (reference: preprocess/precompute_img_features_vit.py): stored uint8 panoramas -> the feature file
`"{scan}_{viewpoint}"` -> [36, image_feat (+ image_prob)] that `data.r2r_data.ViewFeatureStore` reads.

The reference renders 36 views per viewpoint in the simulator, runs timm's eval transform on the host view by view, and pushes them
through a timm ViT (`forward_features`, then `head`).  Here the views come from a `PanoImageStore` (the stored 248 x 330 uint8 views
of BASELINE config 4), the eval transform runs on the device (`hamt_image_prep`, patch rows), and the backbone is
`model.vision_transformer.VisionTransformer` in eval mode under `torch.no_grad()`, by default with the cls-only last block
(`forward_features(cls_tail=True)`).  The classifier head is one fp32 GEMM whatever the backbone's precision: n x D x C is ~0.004 %
of the work, and the logits -- the MRC task's soft labels, `hist_img_probs` -- then carry only the features' error.

Raw renders (480 x 640 from the simulator) need a real resize in front of the crop, which the reference's extraction lets timm's
`Resize(248)` do bicubically (precompute_img_features_vit.py:51-52, 96).  With `resize="bicubic"` the extractor does the same on the
device: `hamt_image_resample`, PIL's antialiased bicubic resample windowed to the centre 224 x 224, then `hamt_image_prep` with the
identity record, then the backbone.  The default (`resize=None`) accepts stored views only, whose short side is 248
(`draw_eval_params` raises on anything else).  The LMDB views were resized with ANTIALIAS, so features made from the LMDB are not
the reference's bit for bit; features made from the renders see the reference's own pixels.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from typing import Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from .. import ops, streams
from ..data.image_data import N_VIEWS, PanoImageStore
from ..data.image_prep import image_prep
from ..data.image_resample import image_resample
from ..data.image_transform import IMGSIZE, RESAMPLE_FILTERS, VIEW_DTYPE, draw_eval_params, eval_resize_geometry, make_record
from ..model.vision_transformer import VisionTransformer

MODEL_CONFIGS = {"vit_base_patch16_224": dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0)}
BACKBONE_PREFIXES = ("bert.vision_backbone.", "vision_backbone.")
# what the reference stores next to every block (precompute_img_features_vit.py:37-39, 155-159): its simulator's camera
REF_IMAGE_W, REF_IMAGE_H, REF_VFOV = 640, 480, 60
MAX_READERS = 16


def load_viewpoint_ids(connectivity_dir: str):
    """[(scan, viewpoint)] of every `included` viewpoint, scans in `scans.txt` order, viewpoints in file order (preprocess/utils.py:5-14)"""
    ids = []
    with open(os.path.join(connectivity_dir, "scans.txt")) as f:
        scans = [x.strip() for x in f if x.strip()]
    for scan in scans:
        with open(os.path.join(connectivity_dir, f"{scan}_connectivity.json")) as f:
            ids.extend((scan, x["image_id"]) for x in json.load(f) if x["included"])
    return ids


# ------------------------------------------------------------------------------------------------ checkpoint -> model
def backbone_state_dict(ckpt) -> "OrderedDict[str, torch.Tensor]":
    """The ViT's own keys out of one of the accepted layouts: the reference's `{'state_dict': timm keys incl. head.*}`
    (precompute_img_features_vit.py:47), a bare state dict, or a pretraining checkpoint whose backbone sits under
    `bert.vision_backbone.` / `vision_backbone.` (that one has no head)."""
    sd = ckpt
    if isinstance(sd, Mapping) and isinstance(sd.get("state_dict"), Mapping):
        sd = sd["state_dict"]
    if not isinstance(sd, Mapping) or not sd:
        raise ValueError("checkpoint: expected a state dict, or a mapping with one under 'state_dict'")
    for prefix in BACKBONE_PREFIXES:
        sub = OrderedDict((k[len(prefix):], v) for k, v in sd.items() if k.startswith(prefix))
        if sub:
            return sub
    return OrderedDict(sd.items())


def build_feature_extractor(model_name="vit_base_patch16_224", checkpoint_file=None, num_classes=1000, hamt_precision="bf16",
                            cls_tail=True, vit_kwargs: Optional[dict] = None, device="cuda", resize: Optional[str] = None) -> "ViewFeatureExtractor":
    """precompute_img_features_vit.py:42-54.  `checkpoint_file`: a path for `torch.load`, or the loaded object.  None raises: the
    reference downloads timm's pretrained weights in that case and there is no download here.  `vit_kwargs` overrides the named
    model's constructor arguments (tests use a 2-block model).  Loading is strict: unknown and missing keys are named in the error.
    A checkpoint without `head.*` gives an extractor without logits.  `resize`: see `ViewFeatureExtractor`."""
    if checkpoint_file is None:
        raise ValueError("build_feature_extractor: checkpoint_file is required (the reference would download timm's pretrained "
                         f"'{model_name}' here; this project never downloads)")
    if model_name not in MODEL_CONFIGS:
        raise ValueError(f"build_feature_extractor: unknown model_name '{model_name}' (known: {sorted(MODEL_CONFIGS)})")
    kw = dict(MODEL_CONFIGS[model_name])
    kw.update(vit_kwargs or {})
    ckpt = torch.load(checkpoint_file, map_location="cpu") if isinstance(checkpoint_file, (str, os.PathLike)) else checkpoint_file
    sd = backbone_state_dict(ckpt)
    has_head = "head.weight" in sd or "head.bias" in sd
    model = VisionTransformer(hamt_precision=hamt_precision, num_classes=int(num_classes) if has_head else 0, **kw)
    want = set(model.state_dict())
    unknown, missing = sorted(set(sd) - want), sorted(want - set(sd))
    if unknown or missing:
        raise ValueError(f"build_feature_extractor: checkpoint does not fit '{model_name}': unknown keys {unknown}, missing keys {missing}")
    model.load_state_dict(sd, strict=True)
    return ViewFeatureExtractor(model.to(device), cls_tail=cls_tail, resize=resize)


class ViewFeatureExtractor:
    """`extractor(views_u8)`: (n, 248, 330, 3) uint8 views (tensor or ndarray, host or device) -> (fts [n, D] fp32, logits [n, C] fp32
    or None), both on the model's device.  Eval records -> `hamt_image_prep` (patch rows) -> the backbone in eval mode under
    `torch.no_grad()` -> the head as an fp32 GEMM.  `resize`: None (views whose short side is not 248 raise) or "bicubic", timm's
    `Resize(248)`: such views, raw (n, 480, 640, 3) renders, are first resampled on the device (`hamt_image_resample`, only the
    centre 224 x 224 of the resized view is computed) and then take the same path with the identity record."""

    def __init__(self, model: VisionTransformer, cls_tail: bool = True, resize: Optional[str] = None):
        if resize is not None and resize not in RESAMPLE_FILTERS:
            raise ValueError(f"ViewFeatureExtractor: resize {resize!r}: None or one of {sorted(RESAMPLE_FILTERS)}")
        self.model = model.eval()
        self.resize = resize
        self.cls_tail = bool(cls_tail)
        self.prec = model.patch_embed.prec
        self.feat_size = model.embed_dim
        self.num_classes = model.num_classes
        self._recs: dict = {}

    @property
    def has_head(self) -> bool:
        return self.num_classes > 0

    @property
    def device(self):
        return self.model.cls_token.device

    def require_head(self):
        if not self.has_head:
            raise ValueError("image logits were asked for, and the checkpoint this extractor was built from has no classifier head "
                             "(`head.weight` / `head.bias`): a pretraining checkpoint carries the backbone only")

    def _records(self, n, H, W, dev, identity=False):
        key = (n, H, W, str(dev), identity)
        r = self._recs.get(key)
        if r is None:
            recs = np.zeros((n,), VIEW_DTYPE)
            # a 1:1 bicubic pass has the taps [0, 2^22, 0, 0] and copies: the centre crop of a stored view, or all of a resampled one
            recs[:] = make_record(box=(0, 0, IMGSIZE, IMGSIZE)) if identity else draw_eval_params(H, W)    # raises for a short side other than 248
            recs["src"] = np.arange(n)
            r = self._recs[key] = (recs, torch.from_numpy(recs.view(np.uint8).copy()).to(dev))
            torch.cuda.current_stream(dev).synchronize()       # (once per batch size: any stream may use the device copy next)
        return r

    @torch.no_grad()
    def extract(self, src: torch.Tensor, logits: Optional[bool] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """src: uint8 (n, H, W, 3) ON the device; logits: None = when there is a head, True = must (raises without a head)"""
        if logits:
            self.require_head()
        logits = self.has_head if logits is None else bool(logits)
        if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3:
            raise ValueError(f"views: expected uint8 (n, H, W, 3), got {src.dtype} {tuple(src.shape)}")
        n, H, W = src.shape[0], src.shape[1], src.shape[2]
        src = src.contiguous()
        OH, OW, window = eval_resize_geometry(H, W)
        resampled = self.resize is not None and (OH, OW) != (H, W)
        if resampled:                                          # Resize(248) + CenterCrop(224) in one launch
            src = image_resample(src, (OH, OW), self.resize, window)
            H = W = IMGSIZE
        recs, recs_dev = self._records(n, H, W, src.device, identity=resampled)
        self.model.eval()
        rows = image_prep(src, recs, recs_dev, layout="patches", dtype=torch.bfloat16 if self.prec == "bf16" else torch.float32)
        fts = self.model.forward_features(rows, cls_tail=self.cls_tail)
        out = None
        if logits:
            head = self.model.head
            out = ops.linear(fts, head.weight, head.bias, ops.ACT_NONE, "fp32")
        return fts, out

    def __call__(self, views_u8, logits: Optional[bool] = None):
        v = torch.from_numpy(np.ascontiguousarray(views_u8)) if isinstance(views_u8, np.ndarray) else views_u8
        if self.device.type != "cuda":
            raise L.HamtError("ViewFeatureExtractor: the model must live on the GPU (no CPU fallback)")
        return self.extract(v.to(self.device), logits)


# ------------------------------------------------------------------------------------------------ the feature file
class ViewFeatureWriter:
    """Writes what `ViewFeatureStore` reads: one float32 [36, D (+ C)] block per key.  Back ends by path, as the reader picks them:
    `.npz` (written when the writer closes), `.hdf5` / `.h5` (h5py, gzip, with the reference's five attrs scanId / viewpointId /
    image_w / image_h / vfov; the same loud ImportError as the reader when h5py is absent), anything else a directory of `<key>.npy`.
    The reference writes float64 (`dtype='float'`, precompute_img_features_vit.py:153); the values are float32 results either way and
    the reader casts to float32, so float32 is what is stored here."""

    def __init__(self, path: str):
        self.path = path
        self._h, self._npz = None, None
        if path.endswith(".npz"):
            self.kind, self._npz = "npz", {}
        elif path.endswith(".hdf5") or path.endswith(".h5"):
            self.kind = "hdf5"
            try:
                import h5py
            except ImportError as e:
                raise ImportError(f"ViewFeatureWriter: '{path}' is an HDF5 file and h5py is not installed; write an .npz archive or a "
                                  "directory of .npy files instead (ViewFeatureStore reads both), or install h5py") from e
            self._mkparent()
            self._h = h5py.File(path, "w")
        else:
            self.kind = "npy_dir"
            os.makedirs(path, exist_ok=True)

    def _mkparent(self):
        parent = os.path.dirname(os.path.abspath(self.path))
        os.makedirs(parent, exist_ok=True)

    def put(self, scan: str, viewpoint: str, block: np.ndarray):
        key = f"{scan}_{viewpoint}"
        block = np.ascontiguousarray(block, dtype=np.float32)
        assert block.ndim == 2 and block.shape[0] == N_VIEWS, block.shape
        if self.kind == "npz":
            self._npz[key] = block.copy()
        elif self.kind == "hdf5":
            ds = self._h.create_dataset(key, block.shape, dtype="float32", compression="gzip")
            ds[...] = block
            for k, v in (("scanId", scan), ("viewpointId", viewpoint), ("image_w", REF_IMAGE_W), ("image_h", REF_IMAGE_H), ("vfov", REF_VFOV)):
                ds.attrs[k] = v
        else:
            np.save(os.path.join(self.path, key + ".npy"), block)

    def close(self):
        if self.kind == "npz" and self._npz is not None:
            self._mkparent()
            np.savez(self.path, **self._npz)
            self._npz = None
        elif self._h is not None:
            self._h.close()
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None or self.kind != "npz":       # (a failed run leaves no half-written archive behind)
            self.close()


def build_feature_file(img_db, scanvp_list: Sequence[Tuple[str, str]], output_file: str, extractor: ViewFeatureExtractor,
                       out_image_logits: bool = False, batch_size: int = 64, num_workers: int = 8) -> int:
    """precompute_img_features_vit.py:113-166 without the simulator: `img_db` is a `PanoImageStore` path or any store with
    `get(key) -> uint8 (36, H, W, 3)`.  The 36 * len(scanvp_list) views are batched ACROSS viewpoints (`batch_size` views per
    backbone pass, whatever 36 divides into).  `num_workers` host threads (at most 16) read panoramas ahead; each batch is gathered
    into one of two pinned buffers and copied on the copy stream while the backbone works on the other.  One
    [36, D (+ C with `out_image_logits`)] float32 block per key goes to `ViewFeatureWriter(output_file)`.  -> the number of keys."""
    if out_image_logits:
        extractor.require_head()
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    store = PanoImageStore(img_db) if isinstance(img_db, (str, os.PathLike)) else img_db
    scanvp_list = [(str(s), str(v)) for s, v in scanvp_list]
    n_vp = len(scanvp_list)
    dev = extractor.device
    if dev.type != "cuda":
        raise L.HamtError("build_feature_file: the extractor must live on the GPU (no CPU fallback)")
    D = extractor.feat_size
    width = D + (extractor.num_classes if out_image_logits else 0)
    total = n_vp * N_VIEWS
    n_batches = (total + batch_size - 1) // batch_size
    readers = max(1, min(int(num_workers), MAX_READERS, max(n_vp, 1)))
    main, copy = torch.cuda.current_stream(dev), streams.role_stream(dev, "h2d")

    with ViewFeatureWriter(output_file) as writer, ThreadPoolExecutor(max_workers=readers) as pool:
        if n_vp == 0:
            return 0
        ahead = readers + (batch_size + N_VIEWS - 1) // N_VIEWS + 1          # panoramas in flight: the readers' plus two batches' worth
        panos: dict = {}                                                     # viewpoint index -> future of its (36, H, W, 3) block
        submitted = 0

        def pano(i):
            nonlocal submitted
            while submitted < min(n_vp, i + ahead):
                panos[submitted] = pool.submit(lambda k="%s_%s" % scanvp_list[submitted]: np.asarray(store.get(k)))
                submitted += 1
            return panos[i].result()

        first = pano(0)
        if first.dtype != np.uint8 or first.ndim != 4 or first.shape[0] != N_VIEWS or first.shape[3] != 3:
            raise ValueError(f"build_feature_file: a panorama is {first.dtype} {first.shape}, expected uint8 (36, H, W, 3)")
        H, W = first.shape[1], first.shape[2]
        pin = [torch.empty((batch_size, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        dbuf = [torch.empty((batch_size, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
        out_pin = [torch.empty((batch_size, width), dtype=torch.float32).pin_memory() for _ in range(2)]
        h2d_done, compute_done, out_done = [None, None], [None, None], [None, None]
        blocks: dict = {}

        def span(i):
            g0 = i * batch_size
            return g0, min(batch_size, total - g0)

        def stage(i):
            """gather batch i into its pinned buffer and start its copy"""
            s = i % 2
            g0, m = span(i)
            if h2d_done[s] is not None:
                h2d_done[s].synchronize()                    # the copy out of this pinned buffer (batch i - 2) has finished
            dst = pin[s].numpy()
            g = g0
            while g < g0 + m:
                vp, v0 = divmod(g, N_VIEWS)
                cnt = min(N_VIEWS - v0, g0 + m - g)
                dst[g - g0:g - g0 + cnt] = pano(vp)[v0:v0 + cnt]
                if v0 + cnt == N_VIEWS:
                    panos.pop(vp, None)
                g += cnt
            with torch.cuda.stream(copy):
                if compute_done[s] is not None:
                    copy.wait_event(compute_done[s])         # the backbone pass that read this device buffer (batch i - 2) has finished
                dbuf[s][:m].copy_(pin[s][:m], non_blocking=True)
                h2d_done[s] = torch.cuda.Event()
                h2d_done[s].record(copy)

        def run(i):
            s = i % 2
            _, m = span(i)
            main.wait_event(h2d_done[s])
            fts, logits = extractor.extract(dbuf[s][:m], logits=bool(out_image_logits))
            compute_done[s] = torch.cuda.Event()
            compute_done[s].record(main)
            out_pin[s][:m, :D].copy_(fts, non_blocking=True)
            if out_image_logits:
                out_pin[s][:m, D:].copy_(logits, non_blocking=True)
            out_done[s] = torch.cuda.Event()
            out_done[s].record(main)

        def drain(i):
            """batch i's rows -> their viewpoints' blocks; a completed block is written"""
            s = i % 2
            g0, m = span(i)
            out_done[s].synchronize()
            res = out_pin[s].numpy()
            g = g0
            while g < g0 + m:
                vp, v0 = divmod(g, N_VIEWS)
                cnt = min(N_VIEWS - v0, g0 + m - g)
                blk = blocks.get(vp)
                if blk is None:
                    blk = blocks[vp] = np.empty((N_VIEWS, width), np.float32)
                blk[v0:v0 + cnt] = res[g - g0:g - g0 + cnt]
                if v0 + cnt == N_VIEWS:
                    writer.put(scanvp_list[vp][0], scanvp_list[vp][1], blocks.pop(vp))
                g += cnt

        with torch.cuda.device(dev):
            stage(0)
            for i in range(n_batches):
                if i + 1 < n_batches:
                    stage(i + 1)
                run(i)
                if i >= 1:
                    drain(i - 1)
            drain(n_batches - 1)
        assert not blocks
    return n_vp
