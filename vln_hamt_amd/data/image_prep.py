"""Thin wrapper over `hamt_image_prep` (csrc/image_prep.hip): uint8 views + parameter records on the device -> the prepared float
images (`nchw`) or directly the patch rows of the ViT's patch-embedding GEMM (`patches`, held by `PatchRows`)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _lib as L
from .image_transform import IMGSIZE, VIEW_DTYPE, norm_table

PATCH = 16
PATCHES_PER_VIEW = (IMGSIZE // PATCH) ** 2          # 196
PATCH_K = 3 * PATCH * PATCH                         # 768

_LUTS: dict = {}


def norm_table_on(device) -> torch.Tensor:
    device = torch.device(device)
    t = _LUTS.get(device)
    if t is None:
        t = _LUTS[device] = torch.from_numpy(norm_table().copy()).to(device)
    return t


class PatchRows:
    """Prepared views in the form `hamt_patchify` gives a (n, 3, 224, 224) tensor: `rows` (Rpad, ldy) fp32 or bf16, row
    v * 196 + py * 14 + px, column c * 256 + ky * 16 + kx.  `lead`: the leading shape the n views stand for ((B, T), (B, T, 36),
    (B, V)), so that the model can treat the holder like the image tensor it replaces."""

    def __init__(self, rows: torch.Tensor, n: int, lead=None):
        self.rows, self.n, self.lead = rows, n, tuple(lead) if lead is not None else (n,)
        assert int(np.prod(self.lead, dtype=np.int64)) == n

    @property
    def shape(self):
        return self.lead + (3, IMGSIZE, IMGSIZE)

    @property
    def device(self):
        return self.rows.device

    @property
    def is_cuda(self):
        return self.rows.is_cuda

    def dim(self):
        return len(self.lead) + 3

    def record_stream(self, stream):
        self.rows.record_stream(stream)


def image_prep(src: torch.Tensor, recs: np.ndarray, recs_dev: Optional[torch.Tensor] = None, layout: str = "nchw",
               dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None, ldy: int = PATCH_K, Rpad: Optional[int] = None,
               ws: Optional[torch.Tensor] = None, lead=None):
    """src: uint8 (n_src, H, W, 3) on the GPU; recs: VIEW_DTYPE [n] on the host; recs_dev: the same bytes on the device (copied
    when not given).  -> float32 (n, 3, 224, 224) for `nchw`, a `PatchRows` for `patches`.  `out`: tensor to fill (its shape,
    dtype and 16-byte alignment are checked by the library); `ws`: scratch of HAMT_WS_IMAGE_PREP {n} bytes."""
    if not src.is_cuda:
        raise L.HamtError("image_prep: the views must live on the GPU (the CPU path is data.image_transform.transform_views)")
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[-1] == 3 and src.is_contiguous(), "src: uint8 (n_src, H, W, 3)"
    recs = np.ascontiguousarray(np.atleast_1d(recs), dtype=VIEW_DTYPE)
    n, dev = len(recs), src.device
    if recs_dev is None:
        recs_dev = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
    need = L.workspace_bytes(L.WS_IMAGE_PREP, n)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if layout == "nchw":
        if out is None:
            out = torch.empty((n, 3, IMGSIZE, IMGSIZE), dtype=torch.float32, device=dev)
        assert out.dtype == torch.float32 and out.numel() == n * 3 * IMGSIZE * IMGSIZE and out.is_contiguous()
        d = L.ImagePrepDesc(n, src.shape[0], src.shape[1], src.shape[2], L.IMAGE_NCHW, 0, L.HAMT_F32, 0)
    elif layout == "patches":
        Rpad = n * PATCHES_PER_VIEW if Rpad is None else Rpad
        if out is None:
            out = torch.empty((Rpad, ldy), dtype=dtype, device=dev)
        assert out.dtype in (torch.float32, torch.bfloat16) and out.is_contiguous()
        d = L.ImagePrepDesc(n, src.shape[0], src.shape[1], src.shape[2], L.IMAGE_PATCHES, ldy,
                            L.HAMT_BF16 if out.dtype == torch.bfloat16 else L.HAMT_F32, Rpad)
    else:
        raise ValueError(f"image_layout {layout!r}: 'nchw' or 'patches'")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.load().hamt_image_prep(C.byref(d), C.c_void_p(recs.ctypes.data), C.c_void_p(recs_dev.data_ptr()), C.c_void_p(src.data_ptr()),
                                     C.c_void_p(norm_table_on(dev).data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                     ws.numel(), st), "hamt_image_prep")
    if layout == "patches":
        return PatchRows(out, n, lead)
    return out
