"""The launches and checks of test_gpu_splitk.py, importable (the test) and runnable (its one child per dispatch switch):

    python tests/_splitk_gpu.py HAMT_KS=4 ratios.txt      # with HAMT_KS=4 in the environment: that switch's rows of SPLITK_GEMMS

hamt_gemm_ws is called directly with a workspace and a C the caller owns: both are prefilled (NaN of a known bit pattern; the seeded C0
under HAMT_EPI_ACCUM), both are followed by a guard band of the same pattern, and both are read back whole."""
import ctypes as C
import os
import sys

import numpy as np
import torch

import _splitk_ref as R
from _gemm_cases import EPI_OF, ROOT, SPLITK_GEMMS, plan_desc, splitk_ws_bytes

DEV = "cuda"
GUARD = 4096                       # floats behind the workspace and behind C
NAN_BITS = 0x7FC5A5A5              # a quiet NaN no kernel produces
PAD_BITS = 0x7FC0                  # bf16 NaN in the columns that pad a K-strided operand's rows to 16 bytes


def _L():
    from vln_hamt_amd import _lib as L
    return L


def nan_buffer(n):
    return torch.full((n,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def bits_of(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def dev_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(torch.bfloat16)


def stored(layout, Ab, Bb):
    """the operands as the layout stores them: (A, B) bf16 device tensors, K-strided rows padded to 8 columns of bf16 NaN"""
    def kstrided(X):            # X [K, cols] -> [K, round up to 8]
        K, c = X.shape
        out = np.full((K, (c + 7) // 8 * 8), PAD_BITS, dtype=np.uint16)
        out[:, :c] = X
        return out
    a = kstrided(Ab.T) if layout == "tn" else Ab
    b = Bb.T if layout == "nt" else kstrided(Bb)
    return dev_bf16(a), dev_bf16(b)


def descriptor(layout, M, N, K, acc, alpha, ka_rows=0, kb_rows=0):
    L = _L()
    d = plan_desc(L.GemmDesc, layout, M, N, K, EPI_OF["acc" if acc else "none"], L.HAMT_F32)
    d.alpha, d.ka_rows, d.kb_rows = alpha, ka_rows, kb_rows
    return d


def launch(d, a, b, C0, ws_floats, ws_bytes):
    """one hamt_gemm_ws call on fresh buffers -> (C [M, N] fp32, C's guard bits, the whole workspace's bits, kernel name)"""
    L = _L()
    M, N = d.M, d.N
    cbuf = nan_buffer(M * N + GUARD)
    if d.epilogue & L.EPI_ACCUM:
        cbuf[:M * N] = torch.from_numpy(C0.copy()).to(DEV).reshape(-1)
    ws = nan_buffer(ws_floats + GUARD)
    assert cbuf.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0 and ws_bytes <= ws_floats * 4
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.load().hamt_gemm_ws(C.byref(d), a.data_ptr(), b.data_ptr(), cbuf.data_ptr(), None, None, ws.data_ptr(), ws_bytes, st), "hamt_gemm_ws")
    torch.cuda.synchronize()
    name = L.last_kernel()
    return cbuf[:M * N].cpu().numpy().reshape(M, N), bits_of(cbuf[M * N:]), bits_of(ws), name


def check_launch(tag, layout, M, N, K, acc, alpha, a, b, ws_floats, ws_bytes, slices, kernel, k_valid=None, ka_rows=0, kb_rows=0):
    """checks (a) - (e) of one problem; returns (worst error / bound, C) and prints the ratio"""
    L = _L()
    d = descriptor(layout, M, N, K, acc, alpha, ka_rows, kb_rows)
    C0 = R.operands(M, N, K)[2]
    assert L.gemm_plan(d, ws_bytes) == (slices, kernel), (tag, L.gemm_plan(d, ws_bytes))                      # (a)
    got, cguard, wsbits, name = launch(d, a, b, C0, ws_floats, ws_bytes)
    assert name == kernel, (tag, name)
    assert (cguard == NAN_BITS).all(), f"{tag}: the guard band behind C was written"
    used = slices * M * N if slices > 1 else 0
    assert (wsbits[used:] == NAN_BITS).all(), f"{tag}: the workspace was written beyond {slices} partial tiles"      # (c)
    want, bound = R.want_and_bound(M, N, K, alpha, acc, slices, k_valid)
    assert np.isfinite(got).all(), f"{tag}: {np.count_nonzero(~np.isfinite(got))} non-finite elements of C"        # (b)
    ratio = float(np.max(np.abs(got.astype(np.float64) - want) / bound))
    print(f"[splitk {tag} alpha {alpha:g}] S = {slices}, worst error / bound: {ratio:.4f}")
    assert ratio <= 1.0, (tag, alpha, ratio)
    if slices > 1:
        P = wsbits[:used].view(np.float32).reshape(slices, M * N)
        assert not np.isnan(P).any(), f"{tag}: {np.count_nonzero(np.isnan(P))} floats of the partial tiles were never written"   # (c)
        summed = R.reduce32(P, C0, acc)                                                                            # (d)
        assert np.array_equal(summed.view(np.uint32), got.reshape(-1).view(np.uint32)), f"{tag}: C is not the partial tiles summed in slice order"
    again, _, wsbits2, _ = launch(d, a, b, C0, ws_floats, ws_bytes)                                                # (e)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(wsbits2, wsbits), f"{tag}: a second call gave other bits"
    return ratio, got


def check_row(row, alpha):
    """a SPLITK_GEMMS row with every reduction row valid"""
    L = _L()
    _, layout, M, N, K, epi, ws_ks, slices, kernel = row
    Ab, Bb, _ = R.operands(M, N, K)
    a, b = stored(layout, Ab, Bb)
    asked = L.load().hamt_gemm_ksplit(descriptor(layout, M, N, K, epi == "acc", alpha))
    ws_bytes = splitk_ws_bytes(row, asked)
    return check_launch(R.case_id(row), layout, M, N, K, epi == "acc", alpha, a, b, ws_bytes // 4, ws_bytes, slices, kernel)[0]


if __name__ == "__main__":      # child of test_gpu_splitk.py: the rows of ONE switch (already in os.environ), every alpha, ratios to argv[2]
    sys.path.insert(0, ROOT)
    setting = sys.argv[1]
    k, v = setting.split("=")
    assert os.environ.get(k) == v
    rows = [r for r in SPLITK_GEMMS if r[0] == setting]
    assert rows
    with open(sys.argv[2], "w") as f:
        for row in rows:
            for alpha in R.ALPHAS:
                f.write(f"{R.case_id(row)} alpha {alpha:g}: {check_row(row, alpha):.4f}\n")
                f.flush()
