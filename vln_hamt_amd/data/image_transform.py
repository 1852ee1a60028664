"""The per-view image transform of the image-input pipeline on the host, in numpy, and its random parameter draws.

The reference runs timm's `create_transform((3, 224, 224), mean = std = 0.5, interpolation="bicubic", crop_pct=0.9, is_training=...)`
on every uint8 view (pretrain_src/data/image_data.py:70-80, 225-237).  With timm's defaults (no auto-augment, re_prob 0) that is

    train:  RandomResizedCrop(scale (0.08, 1), ratio (3/4, 4/3), bicubic) -> RandomHorizontalFlip(0.5) -> ColorJitter(0.4, 0.4, 0.4)
            (brightness, contrast, saturation factors U(0.6, 1.4) in a random order; hue off) -> ToTensor -> Normalize(0.5, 0.5)
    eval:   Resize(248) (a no-op on a view whose short side is 248) -> CenterCrop(224) -> ToTensor -> Normalize(0.5, 0.5)

Here a draw is a small RECORD (`VIEW_DTYPE`, the numpy mirror of `hamt_image_view` in include/hamt.h) and the transform a pure function
of (uint8 view, record): `apply_view` is the CPU path of the pipeline, `hamt_image_prep` (csrc/image_prep.hip) the GPU path, and both
reproduce PIL bit for bit (tests/test_image_pipeline.py chains PIL == numpy == fixture, tests/test_gpu_image_pipeline.py numpy ==
kernel).  The arithmetic is therefore PIL's, integer where PIL's is:

* resize = `Image.crop(box).resize((224, 224), Image.BICUBIC)`: two passes of 8-bit resampling over the cropped image (Resample.c:
  tap weights in double, normalised, 22-bit fixed point, `clip8((2^21 + sum k p) >> 22)`, horizontal first);
* jitter = `ImageEnhance.{Brightness, Contrast, Color}` = `Image.blend(degenerate, image, factor)` in float32, truncated -- clipped
  when the factor is outside [0, 1] -- and rounded to uint8 after every op; contrast's degenerate is `int(mean(grey) + 0.5)` of the
  image as it is when the op runs, grey = `(19595 R + 38470 G + 7471 B + 0x8000) >> 16`;
* normalisation = `torch.from_numpy(u8).float().div(255).sub(0.5).div(0.5)` through a 256-entry table made with exactly that.

The random STREAM of the draws is this module's own: timm / torchvision draw from python's and torch's global generators in an order
that cannot be replayed without them, so only the distributions (supports, probabilities) are restated, not the sequence.
"""
from __future__ import annotations

import functools
import math
import random
from typing import Sequence

import numpy as np

IMGSIZE = 224
HEIGHT, WIDTH = 248, 330                        # the reference's stored view size (image_data.py:20-22)
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_SKIP = 0, 1, 2, 3        # HAMT_JIT_*
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
NO_JITTER = OP_SKIP | OP_SKIP << 2 | OP_SKIP << 4

VIEW_DTYPE = np.dtype([("src", "<i4"), ("left", "<i4"), ("top", "<i4"), ("width", "<i4"), ("height", "<i4"), ("flip", "<i4"),
                       ("zero", "<i4"), ("order", "<i4"), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                       ("reserved", "<i4")])
assert VIEW_DTYPE.itemsize == 48


def pack_order(ops: Sequence[int]) -> int:
    return int(ops[0]) | int(ops[1]) << 2 | int(ops[2]) << 4


def unpack_order(order: int):
    return (order & 3, (order >> 2) & 3, (order >> 4) & 3)


def make_record(box=(0, 0, IMGSIZE, IMGSIZE), flip=False, order=NO_JITTER, factors=(1.0, 1.0, 1.0), src=0, zero=False):
    """one VIEW_DTYPE record; `box` = (left, top, width, height), `factors` = (brightness, contrast, saturation)"""
    r = np.zeros((), VIEW_DTYPE)
    r["src"], r["left"], r["top"], r["width"], r["height"] = src, box[0], box[1], box[2], box[3]
    r["flip"], r["zero"], r["order"] = int(bool(flip)), int(bool(zero)), order if isinstance(order, (int, np.integer)) else pack_order(order)
    r["brightness"], r["contrast"], r["saturation"] = factors
    return r


def zero_record():
    """a slot that is written as all 0.0 (padded history steps, the killed observation)"""
    return make_record(src=-1, zero=True)


# ------------------------------------------------------------------------------------------------ parameter draws
def _uniform(rng, a, b):
    return float(rng.uniform(a, b))


def _randint(rng, lo, hi):
    """integer in [lo, hi], both ends included"""
    if isinstance(rng, random.Random):
        return rng.randint(lo, hi)
    return int(rng.integers(lo, hi + 1))


def draw_eval_params(H=HEIGHT, W=WIDTH):
    """timm's eval transform at crop_pct 0.9: Resize(int(224 / 0.9) = 248) + CenterCrop(224).  The resize is the identity on a view
    whose short side is 248 -- the only case a (crop, 1:1 resize) record can express, so anything else is an error."""
    if min(H, W) != int(math.floor(IMGSIZE / 0.9)):
        raise ValueError(f"eval transform: the short side of a {H} x {W} view is not {int(math.floor(IMGSIZE / 0.9))}; Resize(248) "
                         "would resample the whole view, which a crop record cannot express")
    return make_record(box=(int(round((W - IMGSIZE) / 2.0)), int(round((H - IMGSIZE) / 2.0)), IMGSIZE, IMGSIZE))


def draw_box(rng, H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop.get_params -> ((left, top, width, height), fell_back)"""
    area = H * W
    for _ in range(10):
        target = _uniform(rng, *scale) * area
        aspect = math.exp(_uniform(rng, math.log(ratio[0]), math.log(ratio[1])))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            top = _randint(rng, 0, H - h)
            left = _randint(rng, 0, W - w)
            return (left, top, w, h), False
    in_ratio = W / H                                       # fallback: centre crop, ratio clamped
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return ((W - w) // 2, (H - h) // 2, w, h), True


def draw_train_params(rng, H=HEIGHT, W=WIDTH, jitter=0.4, hflip=0.5):
    """one independent training draw (`rng`: random.Random or numpy Generator): box, flip, three factors, their order"""
    box, _ = draw_box(rng, H, W)
    flip = _uniform(rng, 0.0, 1.0) < hflip
    factors = tuple(_uniform(rng, 1.0 - jitter, 1.0 + jitter) for _ in range(3))
    order = ORDERS[_randint(rng, 0, 5)]
    return make_record(box=box, flip=flip, order=order, factors=factors)


# ------------------------------------------------------------------------------------------------ resample
# PIL's 8-bit two-pass resample (Resample.c), once: `filter_taps` + `resample_pass_u8`.  Two callers:
# * `resize_bicubic_u8`: a crop box -> 224 x 224, bicubic (`hamt_image_prep`, csrc/image_prep.hip, is the GPU path);
# * `resample_u8`: Image.resize((OW, OH), BICUBIC | LANCZOS) of a whole view at a real scale factor, what the reference's preprocessing
#   runs on every 480 x 640 render (build_image_lmdb.py:78 with ANTIALIAS = LANCZOS for the stored views; timm's Resize(248), bicubic,
#   in precompute_img_features_vit.py:51-52); `hamt_image_resample` (csrc/image_resample.hip) is the GPU path.
RESAMPLE_FILTERS = {"bicubic": 0, "lanczos": 1}                # HAMT_RESAMPLE_*
_SUPPORT = {"bicubic": 2.0, "lanczos": 3.0}


def _cubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, ((1.5 * x - 2.5) * x) * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5, 0.0))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x                                     # libm's sin, as PIL's: numpy's vectorised sin may differ in the last bit


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def filter_taps(in_size: int, out_size: int, filter: str = "bicubic", first: int = 0, count=None):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for output coordinates [first, first + count) of an axis resized
    in_size -> out_size -> (xmin [count], xcnt [count], k [count, ksize] int32, zero beyond xcnt)"""
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"resample filter {filter!r}: one of {sorted(RESAMPLE_FILTERS)}")
    count = out_size - first if count is None else count
    scale = np.float64(in_size) / np.float64(out_size)
    fs = max(scale, np.float64(1.0))
    support, ss = _SUPPORT[filter] * fs, 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    cnt = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((count, ksize), np.float64)
    ww = np.zeros(count, np.float64)
    for x in range(ksize):                                  # sequential sum, as the C loop
        arg = (x + xmin - center + 0.5) * ss
        wx = _cubic(arg) if filter == "bicubic" else np.array([_lanczos(float(a)) for a in arg], np.float64).reshape(arg.shape)
        wx = np.where(x < cnt, wx, 0.0)
        w[:, x] = wx
        ww = ww + wx
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0.0, np.trunc(-0.5 + w * 4194304.0), np.trunc(0.5 + w * 4194304.0)).astype(np.int32)
    k[np.arange(ksize)[None, :] >= cnt[:, None]] = 0
    return xmin.astype(np.int32), cnt.astype(np.int32), k


def resample_pass_u8(img: np.ndarray, axis: int, taps) -> np.ndarray:
    """one 8-bit pass of PIL's resample along `axis` of a uint8 array: clip8((2^21 + sum k p) >> 22) in int32, wrapping as C's does.
    Tap by tap -- one gather of every output coordinate's t-th input per tap -- over blocks that stay in the cache, each turned so
    that the resampled axis comes first and a gather moves whole rows."""
    xmin, cnt, k = taps
    shape, n_out, axis = img.shape, len(xmin), axis % img.ndim
    src = np.ascontiguousarray(img).reshape(-1, shape[axis], int(np.prod(shape[axis + 1:])))          # (lead, in, trail)
    out = np.empty((src.shape[0], n_out, src.shape[2]), np.uint8)
    idx = np.minimum(xmin[:, None] + np.arange(k.shape[1]), shape[axis] - 1)
    kk = np.where(np.arange(k.shape[1]) < cnt[:, None], k, 0).astype(np.int32)          # taps beyond xcnt weigh nothing
    step = max(1, 4096 // max(src.shape[2], 1))
    for l in range(0, src.shape[0], step):
        s = np.ascontiguousarray(src[l:l + step].transpose(1, 0, 2))
        acc = np.full((n_out,) + s.shape[1:], 1 << 21, np.int32)
        for t in range(k.shape[1]):
            acc += s[idx[:, t]] * kk[:, t, None, None]
        out[l:l + step] = np.clip(acc >> 22, 0, 255).transpose(1, 0, 2)
    return out.reshape(shape[:axis] + (n_out,) + shape[axis + 1:])


@functools.lru_cache(maxsize=4096)
def _crop_taps(in_size: int):
    """the crop path draws a new box size for almost every view: the taps of a side are made once"""
    return filter_taps(in_size, IMGSIZE)


def resize_bicubic_u8(crop: np.ndarray) -> np.ndarray:
    """uint8 (h, w, 3) -> uint8 (224, 224, 3) == Image.fromarray(crop).resize((224, 224), Image.BICUBIC)"""
    h, w = crop.shape[:2]
    return resample_pass_u8(resample_pass_u8(crop, 1, _crop_taps(w)), 0, _crop_taps(h))


def resample_u8(img: np.ndarray, size, filter: str = "bicubic", window=None) -> np.ndarray:
    """uint8 (..., H, W, 3) -> the window (x0, y0, w, h) (default: all) of `Image.fromarray(view).resize((OW, OH), filter)` for
    size = (OH, OW), uint8 (..., h, w, 3): horizontal pass first, over the input rows the window's vertical taps need; an axis
    whose size does not change is not resampled, as in PIL."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim < 3 or img.shape[-1] != 3:
        raise ValueError(f"resample_u8: expected uint8 (..., H, W, 3), got {img.dtype} {img.shape}")
    H, W = img.shape[-3], img.shape[-2]
    OH, OW = int(size[0]), int(size[1])
    x0, y0, w, h = (0, 0, OW, OH) if window is None else (int(v) for v in window)
    if OH < 1 or OW < 1 or w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > OW or y0 + h > OH:
        raise ValueError(f"resample_u8: window ({x0}, {y0}, {w}, {h}) empty or outside the {OH} x {OW} result")
    ax_y, ax_x = img.ndim - 3, img.ndim - 2
    if OH == H:
        img = np.take(img, np.arange(y0, y0 + h), axis=ax_y)
    else:
        ty = filter_taps(H, OH, filter, y0, h)
        lo, hi = int(ty[0][0]), int(ty[0][-1] + ty[1][-1])
        img = np.take(img, np.arange(lo, hi), axis=ax_y)                               # the rows PIL's horizontal pass covers
        ty = (ty[0] - lo, ty[1], ty[2])
    img = np.take(img, np.arange(x0, x0 + w), axis=ax_x) if OW == W else resample_pass_u8(img, ax_x, filter_taps(W, OW, filter, x0, w))
    if OH != H:
        img = resample_pass_u8(img, ax_y, ty)
    return np.ascontiguousarray(img)


def eval_resize_geometry(H: int, W: int):
    """timm's eval transform at crop_pct 0.9 on an H x W view -> (OH, OW, window): Resize(248) puts the short side at 248 and the
    long side at int(248 * long / short), CenterCrop(224) cuts at int(round((side - 224) / 2.0)) -- `draw_eval_params`' rounding.
    window = (x0, y0, 224, 224) in the resized view."""
    short = int(math.floor(IMGSIZE / 0.9))
    if H <= W:
        OH, OW = short, int(short * W / H)
    else:
        OH, OW = int(short * H / W), short
    return OH, OW, (int(round((OW - IMGSIZE) / 2.0)), int(round((OH - IMGSIZE) / 2.0)), IMGSIZE, IMGSIZE)


# ------------------------------------------------------------------------------------------------ colour jitter
def grey(img: np.ndarray) -> np.ndarray:
    v = img.astype(np.int32)
    return (19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16


def blend(deg, img: np.ndarray, factor) -> np.ndarray:
    """Image.blend(degenerate, image, factor) on uint8 data"""
    f = np.float32(factor)
    d = np.asarray(deg).astype(np.float32)
    t = d + f * (img.astype(np.float32) - d)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0.0, 0, np.where(t >= 255.0, 255, t.astype(np.int32))).astype(np.uint8)


def jitter_op(img: np.ndarray, op: int, factor) -> np.ndarray:
    if op == OP_BRIGHTNESS:
        return blend(0, img, factor)
    if op == OP_CONTRAST:
        g = grey(img)
        return blend((2 * int(g.sum()) + g.size) // (2 * g.size), img, factor)           # int(mean + 0.5)
    if op == OP_SATURATION:
        return blend(grey(img)[..., None], img, factor)
    return img


# ------------------------------------------------------------------------------------------------ the transform
def apply_view(view: np.ndarray, rec) -> np.ndarray:
    """uint8 (H, W, 3) view + record -> the transformed uint8 (224, 224, 3) image BEFORE normalisation"""
    left, top, w, h = int(rec["left"]), int(rec["top"]), int(rec["width"]), int(rec["height"])
    H, W = view.shape[:2]
    if w < 1 or h < 1 or left < 0 or top < 0 or left + w > W or top + h > H:
        raise ValueError(f"crop box ({left}, {top}, {w}, {h}) outside the {H} x {W} view")
    img = resize_bicubic_u8(np.asarray(view[top:top + h, left:left + w]))
    if int(rec["flip"]):
        img = img[:, ::-1]
    factors = (rec["brightness"], rec["contrast"], rec["saturation"])
    for op in unpack_order(int(rec["order"])):
        if op != OP_SKIP:
            img = jitter_op(img, op, factors[op])
    return np.ascontiguousarray(img)


_LUT = None


def norm_table():
    """float32 [256]: byte -> normalised value, with torch's own arithmetic"""
    global _LUT
    if _LUT is None:
        import torch
        _LUT = torch.arange(256, dtype=torch.uint8).float().div(255).sub(0.5).div(0.5).numpy()
    return _LUT


def normalize(img_u8: np.ndarray) -> np.ndarray:
    """uint8 (..., 224, 224, 3) -> float32 (..., 3, 224, 224)"""
    return np.ascontiguousarray(np.moveaxis(norm_table()[img_u8], -1, -3))


def transform_views(views: np.ndarray, recs: np.ndarray) -> np.ndarray:
    """views uint8 (n_src, H, W, 3), recs VIEW_DTYPE [n] -> float32 (n, 3, 224, 224): the tensor the reference's batch keys hold
    (slots with `zero` or src < 0 are 0.0)"""
    recs = np.atleast_1d(recs)
    out = np.zeros((len(recs), 3, IMGSIZE, IMGSIZE), np.float32)
    for i, r in enumerate(recs):
        if not int(r["zero"]) and int(r["src"]) >= 0:
            out[i] = normalize(apply_view(views[int(r["src"])], r))
    return out
