"""Not gpu: the host side of the whole-view resample.  `resample_u8` (numpy) against PIL's own outputs in
tests/golden/image_resample.npz (tools/gen_image_resample_golden.py), the library's host tap function against the numpy taps, the
eval geometry, the proof that the fixture tells three wrong restatements apart, and the compiled kernel's resources."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _image_resample_ref as R
from _util import load_npz


@functools.lru_cache(None)
def _golden():
    return load_npz("image_resample.npz")


def test_fixture_holds_every_case_and_the_filters_differ():
    g = _golden()
    assert int(g["seed"]) == R.SEED
    assert sorted(k for k in g if k != "seed") == sorted(f"{n}/{f}" for n, f in R.keys())
    for name, c in R.CASES.items():
        H, W, OH, OW, win, filters = c
        shape = (win[3], win[2], 3) if win else (OH, OW, 3)
        for f in filters:
            assert g[f"{name}/{f}"].shape == shape and g[f"{name}/{f}"].dtype == np.uint8
        if len(filters) == 2:
            assert (g[f"{name}/bicubic"] != g[f"{name}/lanczos"]).any()


@pytest.mark.parametrize("name,filt", R.keys(), ids=lambda v: str(v))
def test_resample_u8_equals_pil(name, filt):
    from vln_hamt_amd.data.image_transform import resample_u8
    H, W, OH, OW, win, _ = R.CASES[name]
    got = resample_u8(R.case_input(name), (OH, OW), filt, win)
    want = _golden()[f"{name}/{filt}"]
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), int((got != want).sum())


def test_resample_u8_batches_and_refuses_bad_windows():
    from vln_hamt_amd.data.image_transform import resample_u8
    v = R.batch_input("b_window", n=3, at=1)
    H, W, OH, OW, win, _ = R.CASES["b_window"]
    out = resample_u8(v, (OH, OW), "lanczos", win)
    assert out.shape == (3, win[3], win[2], 3) and np.array_equal(out[1], _golden()["b_window/lanczos"])
    for i in (0, 2):
        assert np.array_equal(out[i], resample_u8(v[i], (OH, OW), "lanczos", win))
    with pytest.raises(ValueError, match="window"):
        resample_u8(v, (OH, OW), "lanczos", (10, 0, 16, 12))
    with pytest.raises(ValueError, match="filter"):
        resample_u8(v, (OH, OW), "nearest")


CROP_SIDES = (1, 45, 223, 224, 225, 500, 784)          # box sides of the crop path, side -> 224: upsampling, 1:1, the 15-tap maximum


@pytest.mark.parametrize("name,filt", R.keys() + [(side, "bicubic") for side in CROP_SIDES], ids=lambda v: str(v))
def test_library_taps_equal_numpy_taps(name, filt):
    """`hamt_image_resample_taps` is a host function: PIL's coefficients integer for integer, for both axes of every case, over the
    whole axis and over the window's coordinates.  The crop sides run the tap function `image_prep_resize_kernel` runs on the device:
    one source (csrc/pil_resample.h), instantiated for the bicubic filter on both sides."""
    from vln_hamt_amd.data.image_resample import library_taps
    from vln_hamt_amd.data.image_transform import filter_taps
    if name in CROP_SIDES:
        axes = ((name, 224, 0, 224), (name, 224, 208, 16))
    else:
        H, W, OH, OW, win, _ = R.CASES[name]
        x0, y0, w, h = win if win else (0, 0, OW, OH)
        axes = ((W, OW, 0, OW), (H, OH, 0, OH), (W, OW, x0, w), (H, OH, y0, h))
    for i, o, first, count in axes:
        a, b = library_taps(i, o, filt, first, count), filter_taps(i, o, filt, first, count)
        for u, v in zip(a, b):
            assert u.dtype == v.dtype == np.int32 and u.shape == v.shape and np.array_equal(u, v), (name, filt, i, o)
        assert (a[1] >= 1).all() and (a[0] >= 0).all() and (a[0] + a[1] <= i).all() and a[2].shape[1] >= a[1].max()


def test_library_taps_tap_counts_and_errors():
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd.data.image_resample import library_taps
    lib = L.load()
    assert lib.hamt_image_resample_taps(640, 330, L.RESAMPLE_BICUBIC, 0, 0, None, None, None, 0) == 9
    assert lib.hamt_image_resample_taps(640, 330, L.RESAMPLE_LANCZOS, 0, 0, None, None, None, 0) == 13
    assert lib.hamt_image_resample_taps(20, 40, L.RESAMPLE_LANCZOS, 0, 0, None, None, None, 0) == 7
    assert library_taps(480, 248, "lanczos")[2].shape == (248, 13) and library_taps(480, 248, "bicubic")[2].shape == (248, 9)
    assert lib.hamt_image_resample_taps(640, 330, 9, 0, 0, None, None, None, 0) == -1
    with pytest.raises(L.HamtError, match="hamt_image_resample_taps"):
        library_taps(640, 330, "bicubic", 300, 31)                      # coordinates past the axis
    with pytest.raises(L.HamtError, match="hamt_image_resample_taps"):
        library_taps(0, 330, "bicubic")


def test_eval_resize_geometry():
    from vln_hamt_amd.data.image_transform import draw_eval_params, eval_resize_geometry
    assert eval_resize_geometry(480, 640) == (248, 330, (53, 12, 224, 224))
    assert eval_resize_geometry(640, 480) == (330, 248, (12, 53, 224, 224))
    OH, OW, win = eval_resize_geometry(248, 330)                        # a stored view: no resize, the crop `draw_eval_params` makes
    r = draw_eval_params(248, 330)
    assert (OH, OW) == (248, 330) and win == (int(r["left"]), int(r["top"]), 224, 224)
    with pytest.raises(ValueError, match="short side"):                 # unchanged: a crop record cannot express the resize
        draw_eval_params(480, 640)


@pytest.mark.parametrize("variant", sorted(R.WRONG))
def test_wrong_variants_differ_from_the_golden(variant):
    """the sensitivity proof: a kernel with one of these mistakes cannot pass the bit-for-bit tests"""
    for name, filt in R.keys():
        if name in R.wrong_cases(variant):
            want = _golden()[f"{name}/{filt}"]
            got = R.WRONG[variant](name, filt)
            assert got.shape == want.shape and (got != want).any(), (variant, name, filt)


def test_inputs_reach_clip8_on_both_sides_in_both_passes():
    for name, filt in R.keys():
        if name in ("a_ratio", "b_window"):
            (h_lo, h_hi), (v_lo, v_hi) = R.clip_census(name, filt)
            assert min(h_lo, h_hi, v_lo, v_hi) > 0, (name, filt)


def test_resample_kernel_has_no_scratch_and_no_spills(tmp_path):
    import test_kernel_resources as K
    if not (os.path.exists(K.READELF) and os.path.exists(K.OBJCOPY)):
        pytest.skip("ROCm LLVM tools not installed")
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = []
    for co in K._code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([K.READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and "image_resample_kernel" in name.group(1):
                seen.append((int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)), int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                             int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))))
    assert seen == [(0, 0, 0)], seen
