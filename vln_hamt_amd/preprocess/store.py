"""The stored panorama views (reference: preprocess/build_image_lmdb.py): raw 480 x 640 uint8 renders, 36 per viewpoint -> the
248 x 330 views `PanoImageStore` reads and BASELINE config 4 trains on.

The reference renders each view in the simulator and resizes it on the host with `Image.resize((330, 248), Image.ANTIALIAS)`
(:43-44, 78; ANTIALIAS was Pillow's alias of LANCZOS).  Here the renders come from any object with `get(key) -> uint8
(36, 480, 640, 3)` -- there is no simulator -- and the resize runs on the device, a batch of views per launch, bit for bit PIL's
(`hamt_image_resample`, Lanczos).  Rendering itself and the decoding of stored JPEG / PNG renders are not part of this project.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from .. import streams
from ..data.image_data import N_VIEWS
from ..data.image_resample import image_resample
from .extract import MAX_READERS

RENDER_H, RENDER_W = 480, 640                                  # build_image_lmdb.py:39-41
NEWHEIGHT = 248
NEWWIDTH = int(RENDER_W / RENDER_H * NEWHEIGHT)                # 330 (:43-44)


class PanoImageWriter:
    """Writes what `PanoImageStore` reads: uint8 (36, H, W, 3) per key, as a directory of `<key>.npy`, or -- with `env`, an opened
    LMDB-like environment (`begin(write=True) -> txn`, `txn.put(bytes, bytes)`, `txn.commit()`) -- as the reference's records (key =
    the ascii key, value = the raw bytes, one transaction per key: build_image_lmdb.py:63, 83-84).  The `lmdb` module is not part of
    this project's environment: that back end has been exercised with a stand-in environment only, never with the real module."""

    def __init__(self, path=None, env=None):
        self.path, self.env = path, env
        if env is None:
            if not isinstance(path, (str, os.PathLike)):
                raise ValueError("PanoImageWriter: a directory path or an opened environment (env=) is needed")
            os.makedirs(path, exist_ok=True)

    def put(self, key: str, block: np.ndarray):
        assert block.dtype == np.uint8 and block.ndim == 4 and block.shape[0] == N_VIEWS and block.shape[3] == 3, (block.dtype, block.shape)
        if self.env is not None:
            txn = self.env.begin(write=True)
            txn.put(key.encode("ascii"), np.ascontiguousarray(block).tobytes())
            txn.commit()
        else:
            np.save(os.path.join(self.path, key + ".npy"), block)


def build_image_store(renders, scanvp_list: Sequence[Tuple[str, str]], out_path=None, batch_size: int = 2 * N_VIEWS, num_workers: int = 8,
                      env=None, size=(NEWHEIGHT, NEWWIDTH), device="cuda") -> int:
    """build_image_lmdb.py:55-84 without the simulator.  `renders`: any store with `get(key) -> uint8 (36, H, W, 3)`, key =
    `"{scan}_{viewpoint}"`.  Every panorama is resampled on the device with Lanczos to (36, 248, 330, 3) and written through
    `PanoImageWriter(out_path, env)`.  `batch_size`: views per launch, rounded up to whole panoramas.  `num_workers` host threads (at
    most 16) read panoramas ahead; each batch is gathered into one of two pinned buffers and copied on the copy stream while the
    device resamples the other, and the results come back through two pinned buffers the same way.  -> the number of keys."""
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise L.HamtError("build_image_store: the resample runs on the GPU (the CPU path is data.image_transform.resample_u8)")
    dev = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
    scanvp_list = [(str(s), str(v)) for s, v in scanvp_list]
    keys = ["%s_%s" % sv for sv in scanvp_list]
    n_vp = len(keys)
    writer = PanoImageWriter(out_path, env)
    if n_vp == 0:
        return 0
    OH, OW = int(size[0]), int(size[1])
    P = (batch_size + N_VIEWS - 1) // N_VIEWS                  # panoramas per batch
    n_batches = (n_vp + P - 1) // P
    readers = max(1, min(int(num_workers), MAX_READERS, n_vp))
    main, copy = torch.cuda.current_stream(dev), streams.role_stream(dev, "h2d")

    with ThreadPoolExecutor(max_workers=readers) as pool:
        ahead = readers + 2 * P
        panos: dict = {}
        submitted = 0

        def pano(i):
            nonlocal submitted
            while submitted < min(n_vp, i + ahead):
                panos[submitted] = pool.submit(lambda k=keys[submitted]: np.asarray(renders.get(k)))
                submitted += 1
            return panos.pop(i).result()

        first = pano(0)
        if first.dtype != np.uint8 or first.ndim != 4 or first.shape[0] != N_VIEWS or first.shape[3] != 3:
            raise ValueError(f"build_image_store: a panorama is {first.dtype} {first.shape}, expected uint8 (36, H, W, 3)")
        H, W = first.shape[1], first.shape[2]
        pin = [torch.empty((P * N_VIEWS, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        dbuf = [torch.empty((P * N_VIEWS, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
        obuf = [torch.empty((P * N_VIEWS, OH, OW, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
        out_pin = [torch.empty((P * N_VIEWS, OH, OW, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
        h2d_done, compute_done, out_done = [None, None], [None, None], [None, None]

        def span(i):
            return i * P, min(P, n_vp - i * P)

        def stage(i):
            """gather batch i into its pinned buffer and start its copy"""
            s = i % 2
            p0, m = span(i)
            if h2d_done[s] is not None:
                h2d_done[s].synchronize()                    # the copy out of this pinned buffer (batch i - 2) has finished
            dst = pin[s].numpy()
            for j in range(m):
                blk = first if p0 + j == 0 else pano(p0 + j)
                if blk.shape != (N_VIEWS, H, W, 3) or blk.dtype != np.uint8:
                    raise ValueError(f"build_image_store: '{keys[p0 + j]}' is {blk.dtype} {blk.shape}, expected uint8 {(N_VIEWS, H, W, 3)}")
                dst[j * N_VIEWS:(j + 1) * N_VIEWS] = blk
            with torch.cuda.stream(copy):
                if compute_done[s] is not None:
                    copy.wait_event(compute_done[s])         # the launch that read this device buffer (batch i - 2) has finished
                dbuf[s][:m * N_VIEWS].copy_(pin[s][:m * N_VIEWS], non_blocking=True)
                h2d_done[s] = torch.cuda.Event()
                h2d_done[s].record(copy)

        def run(i):
            s = i % 2
            _, m = span(i)
            main.wait_event(h2d_done[s])
            image_resample(dbuf[s][:m * N_VIEWS], (OH, OW), "lanczos", out=obuf[s][:m * N_VIEWS])
            compute_done[s] = torch.cuda.Event()
            compute_done[s].record(main)
            out_pin[s][:m * N_VIEWS].copy_(obuf[s][:m * N_VIEWS], non_blocking=True)
            out_done[s] = torch.cuda.Event()
            out_done[s].record(main)

        def drain(i):
            s = i % 2
            p0, m = span(i)
            out_done[s].synchronize()
            res = out_pin[s].numpy()
            for j in range(m):
                writer.put(keys[p0 + j], res[j * N_VIEWS:(j + 1) * N_VIEWS])

        with torch.cuda.device(dev):
            stage(0)
            for i in range(n_batches):
                if i + 1 < n_batches:
                    stage(i + 1)
                run(i)
                if i >= 1:
                    drain(i - 1)
            drain(n_batches - 1)
    return n_vp
