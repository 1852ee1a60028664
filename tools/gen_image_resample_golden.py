#!/usr/bin/env python3
"""Writes tests/golden/image_resample.npz: PIL's own `Image.fromarray(view).resize((OW, OH), Image.BICUBIC | Image.LANCZOS)`, cut
to the case's window, for the cases of tests/_image_resample_ref.py (`Image.ANTIALIAS`, what build_image_lmdb.py:78 names, was an
alias of LANCZOS and is gone from current Pillow).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_image_resample_golden.py [--check]

Needs Pillow, which the machine that runs the GPU tests may not have: hence the fixture.  Outputs only (`<case>/<filter>`), plus the
seed; the inputs are regenerated from the seed by whoever reads the fixture.  They are random bytes with three blocks of hard 0 / 255
edges (a vertical edge, a horizontal edge, a 4 x 4 checker), so that the filters' overshoot reaches clip8 on both sides, in the
uint8 intermediate and in the result: --check counts the values below 0 and above 255 in front of both clips for every case with
two passes and asserts that none of the four counts is zero.

--check also compares the fixture with what PIL gives now, and asserts sensitivity on the CPU.  The three wrong variants tried
(tests/_image_resample_ref.py: the other filter; support not scaled by the reduction factor; both passes in float with a single
rounding, no uint8 intermediate) each differ from PIL in at least one byte of every downscaling case, for both filters; the single
float pass is held to the cases with two passes, the only ones that have an intermediate.  At 48 x 64 -> 25 x 33 they differ in
1928 (other filter), 1976 / 2209 (unscaled support, bicubic / Lanczos) and 386 / 447 (single float pass) of 2475 bytes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import _image_resample_ref as R                # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "image_resample.npz")


def build():
    from PIL import Image
    pil = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
    store = {"seed": np.int64(R.SEED)}
    for name, filt in R.keys():
        H, W, OH, OW, win, _ = R.CASES[name]
        out = np.asarray(Image.fromarray(np.array(R.case_input(name))).resize((OW, OH), pil[filt]))
        store[f"{name}/{filt}"] = np.ascontiguousarray(R._cut(out, win))
    return store


def check(data):
    from vln_hamt_amd.data.image_transform import resample_u8
    old = np.load(OUT)
    assert sorted(old.files) == sorted(data), (sorted(old.files), sorted(data))
    for k, v in data.items():
        assert np.array_equal(old[k], v), k
    print("fixture matches PIL")
    for name, filt in R.keys():
        H, W, OH, OW, win, _ = R.CASES[name]
        got = resample_u8(R.case_input(name), (OH, OW), filt, win)
        assert np.array_equal(got, data[f"{name}/{filt}"]), (name, filt)
        if name in R.TWO_PASS_DOWN:
            census = R.clip_census(name, filt)
            print(f"  [{name} {filt}] in front of clip8 (below 0, above 255): horizontal {census[0]}, vertical {census[1]}")
            assert min(census[0]) > 0 and min(census[1]) > 0, (name, filt, census)
    print("numpy restatement matches PIL")
    for variant, fn in R.WRONG.items():
        for name, filt in R.keys():
            if name not in R.wrong_cases(variant):
                continue
            n = int((fn(name, filt) != data[f"{name}/{filt}"]).sum())
            print(f"  [{variant}] {name} {filt}: {n} of {data[f'{name}/{filt}'].size} bytes differ")
            assert n > 0, (variant, name, filt)
    print("every wrong variant is told apart")


if __name__ == "__main__":
    data = build()
    if "--check" in sys.argv:
        check(data)
    else:
        np.savez_compressed(OUT, **data)
        print(OUT, os.path.getsize(OUT), "bytes")
