"""Thin wrapper over `hamt_image_resample` (csrc/image_resample.hip): uint8 views on the device -> PIL's `Image.resize` of each,
bicubic or Lanczos, of which only a window is computed.  The tap tables come from the library's host function
`hamt_image_resample_taps` (PIL's coefficients with the host's libm) and are cached per geometry and device."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _lib as L
from .image_transform import RESAMPLE_FILTERS

_TABLES: dict = {}


def library_taps(in_size: int, out_size: int, filter, first: int = 0, count: Optional[int] = None):
    """`hamt_image_resample_taps` -> (xmin [count], xcnt [count], k [count, ksize]) int32, the layout of
    `data.image_transform.filter_taps`.  A host function: no GPU is needed."""
    fid = RESAMPLE_FILTERS[filter] if isinstance(filter, str) else int(filter)
    count = out_size - first if count is None else count
    lib = L.load()
    ksize = lib.hamt_image_resample_taps(in_size, out_size, fid, first, count, None, None, None, 0)
    L.check(min(ksize, 0), "hamt_image_resample_taps")
    xmin, xcnt, k = np.zeros(count, np.int32), np.zeros(count, np.int32), np.zeros((count, ksize), np.int32)
    rc = lib.hamt_image_resample_taps(in_size, out_size, fid, first, count, C.c_void_p(xmin.ctypes.data), C.c_void_p(xcnt.ctypes.data),
                                      C.c_void_p(k.ctypes.data), ksize)
    L.check(min(rc, 0), "hamt_image_resample_taps")
    return xmin, xcnt, k


def _axis_table(in_size, out_size, fid, first, count, dev):
    """(host int32 [xmin | xcnt | k], the same on the device, ksize); (None, None, 0) for an axis that is not resampled"""
    if in_size == out_size:
        return None, None, 0
    xmin, xcnt, k = library_taps(in_size, out_size, fid, first, count)
    host = np.ascontiguousarray(np.concatenate([xmin, xcnt, k.reshape(-1)]))
    return host, torch.from_numpy(host).to(dev), k.shape[1]


def _tables(H, W, OH, OW, window, fid, dev):
    key = (H, W, OH, OW, window, fid, str(dev))
    t = _TABLES.get(key)
    if t is None:
        if len(_TABLES) > 256:
            _TABLES.clear()
        x0, y0, w, h = window
        t = _TABLES[key] = (_axis_table(W, OW, fid, x0, w, dev), _axis_table(H, OH, fid, y0, h, dev))
        torch.cuda.current_stream(dev).synchronize()           # (once per geometry: any stream may use the device copies next)
    return t


def image_resample(src: torch.Tensor, size, filter="bicubic", window=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src: uint8 (n, H, W, 3) on the GPU; size = (OH, OW); filter: 'bicubic' or 'lanczos' (or a HAMT_RESAMPLE_* id);
    window = (x0, y0, w, h) of the resized view (default: all of it).  -> uint8 (n, h, w, 3) ==
    `Image.fromarray(view).resize((OW, OH), filter)` cut to the window, bit for bit.  `out`: tensor to fill."""
    if not src.is_cuda:
        raise L.HamtError("image_resample: the views must live on the GPU (the CPU path is data.image_transform.resample_u8)")
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[-1] == 3 and src.is_contiguous(), "src: uint8 (n, H, W, 3)"
    if isinstance(filter, str) and filter not in RESAMPLE_FILTERS:
        raise ValueError(f"resample filter {filter!r}: one of {sorted(RESAMPLE_FILTERS)}")
    fid = RESAMPLE_FILTERS[filter] if isinstance(filter, str) else int(filter)
    n, H, W = src.shape[0], src.shape[1], src.shape[2]
    OH, OW = int(size[0]), int(size[1])
    x0, y0, w, h = (0, 0, OW, OH) if window is None else (int(v) for v in window)
    dev = src.device
    d = L.ImageResampleDesc(n, H, W, OH, OW, x0, y0, w, h, fid, 0, 0)
    ok = fid in RESAMPLE_FILTERS.values() and OH >= 1 and OW >= 1 and w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= OW and y0 + h <= OH
    null = C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if not ok:                                                  # no table can be made: the library names what is wrong
        L.check(L.load().hamt_image_resample(C.byref(d), null, null, null, null, C.c_void_p(src.data_ptr()), null, st), "hamt_image_resample")
        raise L.HamtError("hamt_image_resample accepted a geometry without tables")
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    assert out.dtype == torch.uint8 and out.device == dev and out.numel() == n * h * w * 3 and out.is_contiguous(), "out: uint8 (n, h, w, 3)"
    (xh, xd, kx), (yh, yd, ky) = _tables(H, W, OH, OW, (x0, y0, w, h), fid, dev)
    d.kx, d.ky = kx, ky
    p = lambda a, dev_side: null if a is None else C.c_void_p(a.data_ptr() if dev_side else a.ctypes.data)
    L.check(L.load().hamt_image_resample(C.byref(d), p(xh, False), p(yh, False), p(xd, True), p(yd, True), C.c_void_p(src.data_ptr()),
                                         C.c_void_p(out.data_ptr()), st), "hamt_image_resample")
    return out
