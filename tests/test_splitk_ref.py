"""CPU: tests/_splitk_ref.py tells a wrong split-K GEMM from a right one.  On every case test_gpu_splitk.py launches, each seeded mistake
moves at least one element by >= 10 x splitk_bound while a right fp32 computation (every slice's partial rounded once, summed by
reduce32) stays inside it; and reduce32's two forms differ in bits, so that the order test_gpu_splitk.py holds the device to is one."""
import numpy as np
import pytest

import _splitk_ref as R
from _gemm_cases import EPI_OF, SPLITK_GEMMS

# (id, M, N, K, accumulate, slices, tile rows, k_valid): the table's rows that split, the weight-gradient sweeps, the ragged NN reduction
CASES = [(R.case_id(r), r[2], r[3], r[4], r[5] == "acc", r[7], R.tile_rows(r[8]), None) for r in SPLITK_GEMMS if r[7] > 1]
CASES += [(f"wgrad-{M}x{N}x{K}-kv{kv}", M, N, K, kv % 2 == 1, 3, 64, kv) for _, M, N, K in R.WGRAD_ROWS for kv in R.WGRAD_K_VALID]
CASES += [("nn-ragged-70x1032x1600-kv1595", 70, 1032, 1600, True, 3, 64, 1595)]
CASES = list({c[1:]: c for c in CASES}.values())      # (the same problem under two switches or two layouts is one case here)


def _values(M, N, K):
    Ab, Bb, C0 = R.operands(M, N, K)
    return R.bf16_value(Ab).astype(np.float64), R.bf16_value(Bb).astype(np.float64), C0


def test_case_table_is_the_plan_table():
    assert len(SPLITK_GEMMS) == 26 and len(CASES) >= 40
    assert all(r[5] in ("none", "acc") and EPI_OF[r[5]] in (0, 8) for r in SPLITK_GEMMS)
    assert {r[7] for r in SPLITK_GEMMS} == {1, 2, 3, 4, 5, 16}
    assert {R.tile_rows(r[8]) for r in SPLITK_GEMMS} == {32, 64, 128}
    assert any(r[2] * r[3] % 4 for r in SPLITK_GEMMS) and any(r[3] % 4 and not r[2] * r[3] % 4 for r in SPLITK_GEMMS)
    assert R.slice_tiles(1600, 3) == [(0, 8), (8, 16), (16, 25)] and R.slice_tiles(448, 4) == [(0, 1), (1, 3), (3, 5), (5, 7)]
    assert R.slice_tiles(320, 4) == [(0, 1), (1, 2), (2, 3), (3, 5)] and R.slice_tiles(128, 2) == [(0, 1), (1, 2)]


def test_operands_are_bf16_and_every_k_tile_is_heavy_somewhere():
    for M, N, K in [(33, 1, 12288), (130, 131, 1600), (200, 136, 128)]:
        Ab, Bb, C0 = R.operands(M, N, K)
        assert Ab.dtype == np.uint16 and Ab.shape == (M, K) and Bb.shape == (K, N) and C0.dtype == np.float32
        A, B = _values(M, N, K)[:2]
        assert np.isfinite(A).all() and np.isfinite(B).all() and (A[:, :, None] * B[None, :, :1] > 0).all()
        heavy = (np.abs(A).reshape(M, K // 64, 64).min(axis=2) >= 0.5)
        assert heavy.any(axis=0).all() and (heavy.sum(axis=1) == -(-(K // 64) // M)).all()


def test_cached_products_are_the_reference():
    M, N, K = 130, 131, 1600
    A, B, C0 = _values(M, N, K)
    for alpha, acc, kv in [(1.0, False, None), (-2.0, True, 1089), (0.5, True, 1)]:
        want, bound = R.want_and_bound(M, N, K, alpha, acc, 3, kv)
        assert np.array_equal(want, R.splitk_f64(A, B, alpha, C0, acc, kv))
        assert np.allclose(bound, R.splitk_bound(A, B, alpha, C0, acc, kv, 3), rtol=1e-14, atol=0)
    assert np.array_equal(R.splitk_f64(A, B, 1.0, None, False, 65), A[:, :65] @ B[:65])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mistakes_leave_the_bound_and_the_right_sum_does_not(case):
    _, M, N, K, acc, S, bm, kv = case
    Ab, Bb, C0 = R.operands(M, N, K)
    kvs = [kv] if kv is not None else [None, K - 37]      # (a case whose rows all count shows "padding rows counted" with 37 of them declared padding)
    for k_valid in kvs:
        Af, Bf = (Ab, Bb) if k_valid is None else R.pad_fill(Ab, Bb, k_valid, "finite")
        A, B = R.bf16_value(Af).astype(np.float64), R.bf16_value(Bf).astype(np.float64)
        seen = set()
        for alpha in R.ALPHAS:
            want, bound = R.want_and_bound(M, N, K, alpha, acc, S, k_valid)
            assert (bound > 0).all()
            P32 = R.partials_f64(A, B, S, k_valid, alpha).astype(np.float32)
            right = R.reduce32(P32, C0, acc).astype(np.float64).reshape(M, N)
            assert (np.abs(right - want) <= bound).all(), (alpha, float(np.max(np.abs(right - want) / bound)))
            for name in R.MISTAKES:
                if kv is None and k_valid is not None and name != "padding rows counted":
                    continue
                got = R.mistaken(name, A, B, alpha, C0, acc, k_valid, S, bm)
                if got is None:
                    continue
                seen.add(name)
                moved = ~(np.abs(got - want) < 10 * bound)      # (a NaN has left the bound)
                assert moved.any(), (name, alpha, k_valid, float(np.nanmax(np.abs(got - want) / bound)))
        # every mistake the case can show was shown: all of them, but for the padding where every row counts, the accumulate without one,
        # and a stale ZERO where the second slice holds less than one whole valid k-tile (its loss is then a term or two of the sum)
        need = set(R.MISTAKES)
        if k_valid is None:
            need -= {"padding rows counted"}
        elif kv is None:
            need = {"padding rows counted"}
        if not acc:
            need -= {"accumulate ignores C0", "accumulate once per slice"}
        if (K if k_valid is None else k_valid) < (R.slice_tiles(K, S)[1][0] + 1) * R.BK:
            need -= {R.MISTAKES[-2]}
        assert seen == need, (k_valid, need - seen, seen - need)


def test_reduce32_forms_differ_from_four_slices_on():
    """(P0 + P1 + P2) + P3 against (P0 + P1) + (P2 + P3): the same bits up to three slices, not from four on"""
    for M, N, K, S, differ in [(33, 1, 12288, 16, True), (200, 300, 8192, 5, True), (64, 128, 2048, 4, True), (130, 131, 1600, 3, False), (136, 200, 1024, 2, False)]:
        A, B, C0 = _values(M, N, K)
        P32 = R.partials_f64(A, B, S).astype(np.float32)
        for acc in (False, True):
            f4, sc = R.reduce32(P32, C0, acc, form="float4"), R.reduce32(P32, C0, acc, form="scalar")
            assert f4.dtype == sc.dtype == np.float32
            assert np.array_equal(f4.view(np.uint32), sc.view(np.uint32)) == (not differ), (M, N, K, S, acc)
    assert np.array_equal(R.reduce32(P32, None, False), R.reduce32(P32, None, False, form="float4"))      # 136 x 200: M N % 4 == 0
    P3 = np.ones((3, 33), dtype=np.float32)
    assert np.array_equal(R.reduce32(P3, None, False), R.reduce32(P3, None, False, form="scalar"))
