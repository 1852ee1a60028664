"""Recipe shared by tools/gen_image_resample_golden.py and the resample tests: the cases, their inputs (regenerated from the seed,
never stored), and three deliberately WRONG restatements of PIL's resample that a test of the right one must tell apart.
tests/golden/image_resample.npz holds PIL's own `Image.resize` outputs only."""
import functools

import numpy as np

SEED = 20240611
FILTERS = ("bicubic", "lanczos")
OTHER = {"bicubic": "lanczos", "lanczos": "bicubic"}
# name -> (H, W, OH, OW, window (x0, y0, w, h) or None, filters)
CASES = {
    "a_ratio": (48, 64, 25, 33, None, FILTERS),                          # the real ratio, a partial last row tile, odd row strides
    "b_window": (31, 45, 17, 23, (3, 2, 16, 12), FILTERS),               # a non-zero window origin
    "c_upscale": (20, 20, 40, 37, None, FILTERS),                        # upscaling: filter scale 1, short tap lists at the borders
    "d_one_axis": (32, 48, 32, 25, None, FILTERS),                       # rows unchanged: the skipped pass
    "e_real_lanczos": (480, 640, 248, 330, None, ("lanczos",)),          # the real LDS footprint, 13 taps
    "f_real_bicubic_crop": (480, 640, 248, 330, (53, 12, 224, 224), ("bicubic",)),   # the real shape, centre-224 window
}
TWO_PASS_DOWN = ("a_ratio", "b_window", "e_real_lanczos", "f_real_bicubic_crop")     # both axes shrink
DOWN = TWO_PASS_DOWN + ("d_one_axis",)                                               # at least one does


def keys():
    return [(name, f) for name, c in CASES.items() for f in c[5]]


@functools.lru_cache(None)
def _input(name):
    H, W = CASES[name][:2]
    rng = np.random.Generator(np.random.PCG64(SEED + sorted(CASES).index(name)))
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    bh, bw = max(H // 3, 4), max(W // 3, 4)
    a[:bh, :bw // 2] = 0                                   # top left: a hard vertical edge, 0 | 255
    a[:bh, bw // 2:bw] = 255
    a[H - bh:H - bh // 2, W - bw:] = 255                   # bottom right: a hard horizontal edge, 255 over 0
    a[H - bh // 2:, W - bw:] = 0
    yy, xx = np.mgrid[0:bh, 0:bw]
    a[:bh, W - bw:] = np.where(((yy // 4 + xx // 4) % 2 == 0)[..., None], 0, 255)        # top right: a 4 x 4 checker
    a.setflags(write=False)
    return a


def case_input(name):
    """uint8 (H, W, 3), read only"""
    return _input(name)


def batch_input(name, n=3, at=1):
    """uint8 (n, H, W, 3): the case's input at index `at`, the others random bytes from the same seed"""
    a = _input(name)
    rng = np.random.Generator(np.random.PCG64(SEED + 100 + sorted(CASES).index(name)))
    v = rng.integers(0, 256, (n,) + a.shape, dtype=np.uint8)
    v[at] = a
    return v


# ------------------------------------------------------------------------------------------------ raw passes (for the clip8 census)
def raw_pass(img, axis, taps):
    """(2^21 + sum k p) >> 22 BEFORE clip8, int32"""
    xmin, cnt, k = taps
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    acc = np.full((len(xmin),) + src.shape[1:], 1 << 21, np.int32)
    for t in range(k.shape[1]):
        acc += src[np.minimum(xmin.astype(np.int64) + t, src.shape[0] - 1)] * k[:, t].reshape((-1,) + (1,) * (src.ndim - 1))
    return np.moveaxis(acc >> 22, 0, axis)


def clip_census(name, filt):
    """(values below 0, above 255) BEFORE clip8 in the horizontal pass over the whole input, and in the vertical pass"""
    from vln_hamt_amd.data.image_transform import filter_taps
    H, W, OH, OW = CASES[name][:4]
    a = _input(name)
    h = raw_pass(a, 1, filter_taps(W, OW, filt)) if W != OW else a.astype(np.int32)
    v = raw_pass(np.clip(h, 0, 255).astype(np.uint8), 0, filter_taps(H, OH, filt)) if H != OH else h
    return (int((h < 0).sum()), int((h > 255).sum())), (int((v < 0).sum()), int((v > 255).sum()))


# ------------------------------------------------------------------------------------------------ the wrong variants
def _cut(img, window):
    if window is None:
        return img
    x0, y0, w, h = window
    return img[y0:y0 + h, x0:x0 + w]


def wrong_other_filter(name, filt):
    from vln_hamt_amd.data.image_transform import resample_u8
    H, W, OH, OW, win, _ = CASES[name]
    return resample_u8(_input(name), (OH, OW), OTHER[filt], win)


def _taps_unscaled(in_size, out_size, filt):
    """the taps of an interpolating resize: support 2 (3) whatever the reduction -- no antialiasing"""
    from vln_hamt_amd.data.image_transform import _cubic, _lanczos
    scale = in_size / out_size
    support = 2.0 if filt == "bicubic" else 3.0
    ksize = int(np.ceil(support)) * 2 + 1
    xmin, cnt, k = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32), np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        x0, x1 = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in_size)
        w = np.array([float(_cubic(np.float64(x + x0 - center + 0.5))) if filt == "bicubic" else _lanczos(x + x0 - center + 0.5) for x in range(x1 - x0)])
        w = w / w.sum()
        k[xx, :x1 - x0] = np.where(w < 0, np.trunc(-0.5 + w * 4194304.0), np.trunc(0.5 + w * 4194304.0))
        xmin[xx], cnt[xx] = x0, x1 - x0
    return xmin, cnt, k


def wrong_unscaled_support(name, filt):
    from vln_hamt_amd.data.image_transform import resample_pass_u8
    H, W, OH, OW, win, _ = CASES[name]
    img = _input(name)
    if W != OW:
        img = resample_pass_u8(img, 1, _taps_unscaled(W, OW, filt))
    if H != OH:
        img = resample_pass_u8(img, 0, _taps_unscaled(H, OH, filt))
    return _cut(img, win)


def wrong_single_float_pass(name, filt):
    """PIL's own taps, both passes in float64 with one rounding at the end: no uint8 (rounded, clipped) intermediate"""
    from vln_hamt_amd.data.image_transform import filter_taps
    H, W, OH, OW, win, _ = CASES[name]
    img = _input(name).astype(np.float64)
    for axis, (i, o) in ((1, (W, OW)), (0, (H, OH))):
        if i == o:
            continue
        xmin, cnt, k = filter_taps(i, o, filt)
        src = np.moveaxis(img, axis, 0)
        acc = np.zeros((o,) + src.shape[1:], np.float64)
        for t in range(k.shape[1]):
            acc += src[np.minimum(xmin.astype(np.int64) + t, i - 1)] * (k[:, t] / 4194304.0).reshape(-1, 1, 1)
        img = np.moveaxis(acc, 0, axis)
    return _cut(np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8), win)


WRONG = {"other filter": wrong_other_filter, "support not scaled": wrong_unscaled_support, "single float pass": wrong_single_float_pass}


def wrong_cases(variant):
    """the cases a variant must differ on: every downscaling case; the single float pass only where there ARE two passes (with one
    pass there is no intermediate to leave out, and float taps against 22-bit taps alone need not move a byte)"""
    return TWO_PASS_DOWN if variant == "single float pass" else DOWN
