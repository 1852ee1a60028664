"""R2R pretraining data with RAW panorama views (BASELINE config 4; reference: pretrain_src/data/image_data.py).

`MultiStepNavImageData.get_input` returns the reference's keys (`hist_images`, `hist_pano_images`, `ob_images` next to the unchanged
text / angle / label keys, image_data.py:98-173) -- but where the reference puts prepared float tensors (36 PIL transforms per
viewpoint on the host, :225-237) a sample here carries the stored uint8 views and one small parameter record per view
(`image_transform.VIEW_DTYPE`: crop box, flip, colour jitter, or "zero").  The transform itself runs later, for the whole batch at
once: on the GPU in `hamt_image_prep` (data/image_tasks.py `to_device`), or on the host in `image_transform.transform_views`.

Per sample:
    image_views        list of uint8 (36, H, W, 3) blocks: block t < T is the panorama of history step t, block T the observation
    hist_pano_images   records (T, 36), `src` = block * 36 + view
    hist_images        records (T,): THE record of `hist_pano_images[t, viewidx_t]` -- the reference takes the history-step image
                       out of the transformed panorama (:194-198), so it is the same transformed view, not a second draw
    ob_images          records (36,)   (no STOP row: image_data.py:142)
"""
from __future__ import annotations

import os
import random
import zlib
from typing import Dict, Optional

import numpy as np

from .image_transform import HEIGHT, WIDTH, VIEW_DTYPE, draw_eval_params, draw_train_params
from .r2r_data import MultiStepNavData

N_VIEWS = 36


class PanoImageStore:
    """`"{scan}_{viewpoint}"` -> uint8 (36, H, W, 3), the views of one panorama as the reference stores them (image_data.py:225-230).
    Back ends by path: a directory of `<key>.npy` (memory mapped), an `.npz` archive, or the reference's LMDB (key = the ascii key,
    value = the 36 * H * W * 3 raw bytes) -- a directory holding `data.mdb` or a path ending in `.lmdb`, opened through a guarded
    `import lmdb`.  `env=` takes an already opened LMDB-like environment (anything with `begin() -> txn`, `txn.get(bytes)`).
    The `lmdb` module is not part of this project's environment: that back end has been exercised with a stand-in environment only,
    never with the real module.  Handles are opened lazily and never shared across DataLoader workers."""

    def __init__(self, path: Optional[str] = None, height: int = HEIGHT, width: int = WIDTH, env=None):
        self.path, self.height, self.width = path, height, width
        self._env, self._h = env, None
        if env is not None:
            self.kind = "lmdb"
        elif not isinstance(path, str):
            raise ValueError("PanoImageStore: a path or an opened environment (env=) is needed")
        elif path.endswith(".npz"):
            self.kind = "npz"
        elif path.endswith(".lmdb") or os.path.exists(os.path.join(path, "data.mdb")):
            self.kind = "lmdb"
        elif os.path.isdir(path):
            self.kind = "npy_dir"
        else:
            raise ValueError(f"PanoImageStore: '{path}' is neither a directory of .npy files, an .npz archive nor an LMDB")

    def _handle(self):
        if self._h is None:
            if self.kind == "lmdb":
                env = self._env
                if env is None:
                    try:
                        import lmdb
                    except ImportError as e:
                        raise ImportError(f"PanoImageStore: '{self.path}' is an LMDB and the lmdb module is not installed; export it "
                                          "to a directory of .npy files, or install lmdb") from e
                    env = lmdb.open(self.path, map_size=int(1e12), readonly=True, create=False, readahead=False, max_readers=2000)
                self._h = env.begin()
            elif self.kind == "npz":
                self._h = np.load(self.path, mmap_mode="r")
            else:
                self._h = self.path
        return self._h

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_h"] = None
        if self.path is not None:            # a real LMDB is re-opened in the worker; a stand-in environment travels as it is
            st["_env"] = None
        return st

    def get(self, key: str) -> np.ndarray:
        h = self._handle()
        shape = (N_VIEWS, self.height, self.width, 3)
        if self.kind == "lmdb":
            buf = h.get(key.encode("ascii"))
            if buf is None:
                raise KeyError(key)
            return np.frombuffer(buf, dtype=np.uint8).reshape(shape)
        a = np.load(os.path.join(h, key + ".npy"), mmap_mode="r") if self.kind == "npy_dir" else np.asarray(h[key])
        if a.dtype != np.uint8 or a.shape != shape:
            raise ValueError(f"PanoImageStore: '{key}' is {a.dtype} {a.shape}, expected uint8 {shape}")
        return a


class SyntheticPanoStore:
    """Deterministic views made from the key: a smooth colour pattern plus noise, per view.  A real viewpoint is 8.8 MB, so tests,
    fixtures and the bench tool take their images from here.  `cache`: number of panoramas kept (generation costs tens of milliseconds)."""

    def __init__(self, seed: int = 0, height: int = HEIGHT, width: int = WIDTH, cache: int = 64):
        self.seed, self.height, self.width, self.cache = seed, height, width, cache
        self._cache: Dict[str, np.ndarray] = {}

    def get(self, key: str) -> np.ndarray:
        a = self._cache.get(key)
        if a is not None:
            return a
        H, W = self.height, self.width
        g = np.random.Generator(np.random.PCG64([self.seed, zlib.crc32(key.encode("ascii"))]))
        fx, fy, ph = (g.uniform(lo, hi, (N_VIEWS, 3)).astype(np.float32) for lo, hi in ((0.01, 0.12), (0.01, 0.12), (0, 6.28)))
        amp, base = g.uniform(20, 110, (N_VIEWS, 3)).astype(np.float32), g.uniform(60, 200, (N_VIEWS, 3)).astype(np.float32)
        ax = np.arange(W, dtype=np.float32)[None, :, None] * fx[:, None, :] + ph[:, None, :]          # (36, W, 3)
        ay = np.arange(H, dtype=np.float32)[None, :, None] * fy[:, None, :]                           # (36, H, 3)
        # sin(ax + ay) as two outer products
        smooth = np.sin(ay)[:, :, None, :] * np.cos(ax)[:, None, :, :] + np.cos(ay)[:, :, None, :] * np.sin(ax)[:, None, :, :]
        smooth = base[:, None, None, :] + amp[:, None, None, :] * smooth
        noise = g.integers(-24, 25, (N_VIEWS, H, W, 3), dtype=np.int8)
        a = np.clip(smooth + noise, 0, 255).astype(np.uint8)
        if len(self._cache) >= self.cache:
            self._cache.pop(next(iter(self._cache)))
        self._cache[key] = a
        return a


class MultiStepNavImageData(MultiStepNavData):
    """image_data.py:25-173.  `img_db`: a path for `PanoImageStore` or a store object (`get(key) -> uint8 (36, H, W, 3)`).
    `img_ft_file` is still read: the MRC soft labels are the class-probability columns of the feature file (:239-252).
    `is_training`: training draws per view (`draw_train_params`) or the eval centre crop; and, as in the reference (:82-93), a
    validation set is ONE random (instruction, step) per trajectory, drawn from numpy's global stream at construction.
    Draws come from `rng` (random.Random / numpy Generator) when given; otherwise from a generator of this object's own, seeded by
    `draw_seed` and, inside a DataLoader worker, by that worker's seed -- never from the global streams, which stay the task
    datasets' (word masking, kills, region masks), so the non-image part of a sample is the feature-input pipeline's draw for draw."""

    def __init__(self, traj_files, img_db, img_ft_file, scanvp_cands_file, connectivity_dir, is_training=False,
                 image_prob_size=1000, image_feat_size=2048, angle_feat_size=4, max_txt_len=80, max_act_len=100, in_memory=False,
                 rng=None, draw_seed: int = 0):
        super().__init__(traj_files, img_ft_file, scanvp_cands_file, connectivity_dir, image_prob_size=image_prob_size,
                         image_feat_size=image_feat_size, angle_feat_size=angle_feat_size, max_txt_len=max_txt_len, max_act_len=max_act_len,
                         in_memory=in_memory)
        self.images = PanoImageStore(img_db) if isinstance(img_db, str) else img_db
        self.is_training, self.draw_seed = is_training, draw_seed
        self._rng, self._rng_owner = rng, None if rng is None else "given"
        if not is_training:                       # "cannot evaluate all the samples as it takes too much time"
            self.traj_step_refer, self.traj_refer = [], []
            for sel in np.random.permutation(len(self.traj_data)):
                item = self.traj_data[sel]
                path_len = min(len(item["path"]), self.max_act_len - 1)
                j = np.random.randint(len(item["instr_encodings"]))
                t = np.random.randint(path_len)
                self.traj_refer.append((int(sel), int(j), path_len))
                self.traj_step_refer.append((int(sel), int(j), int(t)))

    def __getstate__(self):
        st = dict(self.__dict__)
        if st["_rng_owner"] != "given":
            st["_rng"], st["_rng_owner"] = None, None
        return st

    def _draw_rng(self):
        if self._rng_owner == "given":
            return self._rng
        from torch.utils.data import get_worker_info
        info = get_worker_info()
        owner = (os.getpid(), None if info is None else info.seed)
        if self._rng_owner != owner:
            self._rng, self._rng_owner = random.Random(f"{self.draw_seed}/{owner[1]}"), owner
        return self._rng

    def get_image(self, scan, viewpoint, block: int):
        """-> (uint8 (36, H, W, 3), records (36,) with src = block * 36 + view): one independent draw per view (:233-235)"""
        views = self.images.get(f"{scan}_{viewpoint}")
        H, W = views.shape[1:3]
        recs = np.zeros((N_VIEWS,), VIEW_DTYPE)
        if self.is_training:
            rng = self._draw_rng()
            for v in range(N_VIEWS):
                recs[v] = draw_train_params(rng, H, W)
        else:
            recs[:] = draw_eval_params(H, W)
        recs["src"] = block * N_VIEWS + np.arange(N_VIEWS)
        return views, recs

    def get_input(self, i_path, j_instr, t_cur, return_ob=False, return_hist_img_probs=False, return_ob_action=False,
                  return_ob_progress=False, ob_cand_pano_view=None):
        outs = super().get_input(i_path, j_instr, t_cur, return_ob=return_ob, return_hist_img_probs=return_hist_img_probs,
                                 return_ob_action=return_ob_action, return_ob_progress=return_ob_progress, ob_cand_pano_view=False)
        for k in ("hist_img_fts", "hist_pano_img_fts", "ob_img_fts"):
            outs.pop(k, None)
        td = self.traj_data[i_path]
        scan, path, viewidx = td["scan"], td["path"][:self.max_act_len - 1], td["path_viewindex"]
        blocks, pano = [], np.zeros((t_cur, N_VIEWS), VIEW_DTYPE)
        for t in range(t_cur):
            views, pano[t] = self.get_image(scan, path[t], t)
            blocks.append(views)
        outs["hist_pano_images"] = pano
        outs["hist_images"] = pano[np.arange(t_cur), np.asarray(viewidx[:t_cur], dtype=np.int64)] if t_cur > 0 else np.zeros((0,), VIEW_DTYPE)
        if return_ob:
            views, outs["ob_images"] = self.get_image(scan, path[t_cur], t_cur)
            blocks.append(views)
        outs["image_views"] = blocks
        return outs
