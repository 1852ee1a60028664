"""-m gpu: what the split-K GEMM path computes -- gemm_fast_kernel with K slices over the grid (csrc/gemm_fast.hip) and
hamt_reduce_partials (csrc/gemm.hip) -- on the problems tests/_gemm_cases.py pins to it (SPLITK_GEMMS; test_gemm_plan.py asserts the
same slices and kernels without a GPU), against tests/_splitk_ref.py.  Per launch (tests/_splitk_gpu.py: check_launch):
  (a) hamt_gemm_plan, given the same workspace, names the row's slices and kernel, and hamt_last_kernel names that kernel afterwards;
  (b) every element of C is finite and within splitk_bound (derived: EPS32 (k_valid + S + 2) (|alpha| |A| @ |B| + |C0|)) of float64;
  (c) the first S M N floats of the NaN-prefilled workspace are all written, nothing behind them is, nor behind C;
  (d) C is reduce32 of the partial tiles read back from the workspace, bit for bit: "deterministic, summed in slice order";
  (e) a second call gives the same bits in C and in the workspace;
  (f) all of it with alpha = 1, 0.5 and -2 (the partial tiles hold alpha x the slice's sum).
tests/test_splitk_ref.py shows on the CPU that bound and cases tell a wrong kernel from a right one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _splitk_gpu as G
import _splitk_ref as R
from _gemm_cases import ROOT, SPLITK_GEMMS, SPLITK_SWITCHES

pytestmark = pytest.mark.gpu
DEFAULT_ROWS = [r for r in SPLITK_GEMMS if r[0] is None]
WGRAD = {(r[2], r[3], r[4]): r for r in DEFAULT_ROWS if (r[1], r[2], r[3], r[4]) in R.WGRAD_ROWS}


@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("row", DEFAULT_ROWS, ids=[R.case_id(r) for r in DEFAULT_ROWS])
def test_splitk_rows_vs_float64(row, alpha):
    G.check_row(row, alpha)


@pytest.mark.parametrize("k_valid", R.WGRAD_K_VALID)
@pytest.mark.parametrize("shape", sorted(WGRAD), ids=lambda s: "x".join(map(str, s)))
def test_wgrad_form_never_reads_the_padding_rows(shape, k_valid):
    """The weight-gradient form (blocks._proj_bwd / _wgrad: TN, k_valid = the rows that count, the rest torch.empty): the rows >= k_valid
    of BOTH operands hold bf16 NaN, then +-3e38, and the result is the float64 product of the valid rows either way -- the same bits
    both times, and the same bits again through ops.gemm(k_valid=), which asks for the slices and allocates the workspace itself."""
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd import ops
    assert len(WGRAD) == 2
    _, layout, M, N, K, epi, _, slices, kernel = WGRAD[shape]
    acc = epi == "acc"
    Ab, Bb, C0 = R.operands(M, N, K)
    outs = []
    for fill in ("nan", "huge"):
        a, b = G.stored(layout, *R.pad_fill(Ab, Bb, k_valid, fill))
        tag = f"wgrad {M}x{N}x{K} k_valid {k_valid} {fill}"
        outs.append(G.check_launch(tag, layout, M, N, K, acc, 1.0, a, b, slices * M * N, slices * M * N * 4, slices, kernel, k_valid, k_valid, k_valid)[1])
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    out = torch.from_numpy(C0.copy()).to(G.DEV) if acc else torch.full((M, N), float("nan"), device=G.DEV)
    ops.gemm(a[:, :M], b[:, :N], out, a_kmajor=True, b_kmajor=True, epilogue=L.EPI_ACCUM if acc else 0, k_valid=k_valid)
    torch.cuda.synchronize()
    assert L.last_kernel() == kernel
    assert np.array_equal(out.cpu().numpy().view(np.uint32), outs[0].view(np.uint32))


def test_wgrad_of_an_ineligible_weight_splits():
    """blocks._wgrad on a weight the grouped launch does not take (not a leaf that needs a gradient): one split-K hamt_gemm, padding rows NaN"""
    from vln_hamt_amd import _lib as L
    from vln_hamt_amd import blocks
    _, layout, M, N, K, _, _, slices, kernel = WGRAD[(136, 200, 1600)]
    rows = 1541
    Ab, Bb, _ = R.operands(M, N, K)
    dy16, x16 = G.stored(layout, *R.pad_fill(Ab, Bb, rows, "nan"))
    w = torch.zeros(M, N, device=G.DEV)
    assert not w.requires_grad
    dw, db = blocks._wgrad(w, None, dy16, x16, rows)
    torch.cuda.synchronize()
    assert db is None and dw.shape == (M, N) and dw.dtype == torch.float32
    plain = kernel.replace("<64, 8,", "<64, 0,")      # (the row accumulates; _wgrad stores)
    assert L.last_kernel() == plain
    assert L.gemm_plan(G.descriptor(layout, M, N, K, False, 1.0, rows, rows)) == (slices, plain) and slices == 3
    want, bound = R.want_and_bound(M, N, K, 1.0, False, slices, rows)
    got = dw.cpu().numpy()
    assert np.isfinite(got).all()
    ratio = float(np.max(np.abs(got - want) / bound))
    print(f"[splitk blocks._wgrad {M}x{N}x{K} rows {rows}] worst error / bound: {ratio:.4f}")
    assert ratio <= 1.0


def test_nn_ragged_reduction():
    """NN with a reduction rounded up for A: B stores K - 5 rows (kb_rows; the 5 behind them hold NaN here and are never read), A holds
    zeros in its last 5 columns"""
    layout, M, N, K, kb = R.NN_RAGGED
    row = next(r for r in DEFAULT_ROWS if r[1:5] == (layout, M, N, K))
    Ab, Bb, _ = R.operands(M, N, K)
    Ab, Bb = Ab.copy(), R.pad_fill(Ab, Bb, kb, "nan")[1]
    Ab[:, kb:] = 0
    a, b = G.stored(layout, Ab, Bb)
    for alpha in R.ALPHAS:
        G.check_launch(f"nn ragged {M}x{N}x{K} kb_rows {kb}", layout, M, N, K, True, alpha, a, b, row[7] * M * N, row[7] * M * N * 4, row[7], row[8], kb, 0, kb)


def test_splitk_rows_under_the_switches(tmp_path):
    """The rows under a dispatch switch (read once per process): one fresh python per switch, one after another, each running its rows
    with checks (a) - (f) inside; the first child that does not exit 0 ends the test."""
    for setting in SPLITK_SWITCHES:
        k, v = setting.split("=")
        out = tmp_path / f"{k}.txt"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_splitk_gpu.py"), setting, str(out)], env={**os.environ, k: v},
                           capture_output=True, text=True, timeout=300)
        print(f"[splitk {setting}] worst error / bound per case:\n{out.read_text() if out.exists() else ''}")
        assert r.returncode == 0, f"{setting}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
