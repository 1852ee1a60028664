"""numpy reference of the split-K GEMM path -- gemm_fast_kernel launched with K slices over the grid (csrc/gemm_fast.hip: raw fp32
partial tiles into a workspace) followed by hamt_reduce_partials (csrc/gemm.hip) -- for test_gpu_splitk.py; no torch, no GPU, nothing
of the package.  tests/test_splitk_ref.py shows on the CPU that the cases and the bound tell a wrong kernel from a right one.

  * splitk_f64: alpha A[:, :k_valid] @ B[:k_valid] (+ C0) in float64 of the exact bf16 operand values;
  * splitk_bound: the derived per-element bound of the fp32 chain;
  * reduce32: the reduce pass in fp32, bit for bit, in both forms hamt_reduce_partials chooses between;
  * the cases (tests/_gemm_cases.py: SPLITK_GEMMS) with their seeded operands, and the seeded mistakes."""
import functools

import numpy as np

from _gemm_cases import SPLITK_GEMMS
from _smallops_ref import EPS32, F32, bf16_bits, bf16_value

BK = 64                                     # k-tile (gemm_frag.h)
ALPHAS = (1.0, 0.5, -2.0)
# valid reduction rows of the weight-gradient form (TN, K = 1600: three slices of 8, 8, 9 k-tiles, so slice boundaries at 512 and 1024):
# inside the last slice (K - 1, 1541, 1030), on a k-tile boundary and one past it (1088, 1089), on a slice boundary and one past it
# (1024, 1025: the last slice holds nothing / one row; 512, 513), in the first slice only (65: one row of its second k-tile; 1)
WGRAD_ROWS = [("tn", 136, 200, 1600), ("tn", 130, 131, 1600)]
WGRAD_K_VALID = [1599, 1541, 1089, 1088, 1030, 65, 1, 1025, 1024, 513, 512]
NN_RAGGED = ("nn", 70, 1032, 1600, 1595)    # B stores K - 5 rows, A holds zeros in its last 5 columns


# ---------------------------------------------------------------------------------------------- the three statements
def splitk_f64(A, B, alpha=1.0, C0=None, accumulate=False, k_valid=None):
    """alpha A[:, :k_valid] @ B[:k_valid] (+ C0), float64.  A [M, K] and B [K, N] hold the exact values of the bf16 operands (however the
    kernel's layout stores them); k_valid None = all K rows count."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    kv = A.shape[1] if k_valid is None else k_valid
    out = float(alpha) * (A[:, :kv] @ B[:kv])
    return out + np.asarray(C0, dtype=np.float64) if accumulate else out


def splitk_bound(A, B, alpha=1.0, C0=None, accumulate=False, k_valid=None, slices=1):
    """|C - splitk_f64| <= EPS32 (k_valid + S + 2) (|alpha| |A| @ |B| + |C0|) per element.  Derived, not measured: a product of two bf16
    values (8 significant bits each) is exact in fp32, so only additions round.  Whatever order the MFMA and the k loop add a slice's
    products in, a product passes through at most k_valid - 1 additions before its partial tile is stored (each at most EPS32 / 2
    relative, so k_valid EPS32 is generous); S more for the sum over the S slices, one for alpha, one for the accumulate into C0."""
    A, B = np.abs(np.asarray(A, dtype=np.float64)), np.abs(np.asarray(B, dtype=np.float64))
    kv = A.shape[1] if k_valid is None else k_valid
    mag = abs(float(alpha)) * (A[:, :kv] @ B[:kv])
    if accumulate:
        mag = mag + np.abs(np.asarray(C0, dtype=np.float64))
    return EPS32 * (kv + slices + 2) * mag


def reduce32(P, C0=None, accumulate=False, form=None):
    """hamt_reduce_partials in fp32, bit for bit.  P [S, M N] fp32 = the partial tiles as the workspace holds them.
    M N % 4 == 0 (and 16-byte aligned pointers: the tests' are) -> reduce_partials4_kernel ("float4"): slices added in order 0, 1, 2, ...
    into a zero, then + C0.  Otherwise reduce_partials_kernel ("scalar"): four phases r = ph, ph + 4, ... each summed in order into a
    zero, t = (r0 + r1) + (r2 + r3), then C0 + t.  `form` forces one of them (the CPU test compares the two)."""
    P = np.asarray(P, dtype=F32)
    P = P.reshape(P.shape[0], -1)
    S, n = P.shape
    form = form or ("float4" if n % 4 == 0 else "scalar")
    if form == "float4":
        s = np.zeros(n, dtype=F32)
        for r in range(S):
            s = s + P[r]
        if accumulate:
            s = s + np.asarray(C0, dtype=F32).reshape(-1)
        return s
    assert form == "scalar"
    ph = []
    for p in range(4):
        s = np.zeros(n, dtype=F32)
        for r in range(p, S, 4):
            s = s + P[r]
        ph.append(s)
    t = (ph[0] + ph[1]) + (ph[2] + ph[3])
    return np.asarray(C0, dtype=F32).reshape(-1) + t if accumulate else t


# ---------------------------------------------------------------------------------------------- how the kernel cuts the reduction
def slice_tiles(K, S):
    """[(first k-tile, one past the last)] of the S slices (gemm_fast_kernel: kt0 = nk s / S)"""
    nk = K // BK
    return [(nk * s // S, nk * (s + 1) // S) for s in range(S)]


def tile_rows(kernel):
    return int(kernel.split("<")[1].split(",")[0])


def partials_f64(A, B, S, k_valid=None, alpha=1.0):
    """[S, M, N] float64: alpha x each slice's own sum (what the workspace holds, unrounded)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    K = A.shape[1]
    kv = K if k_valid is None else k_valid
    return np.stack([float(alpha) * (A[:, min(kv, t0 * BK):min(kv, t1 * BK)] @ B[min(kv, t0 * BK):min(kv, t1 * BK)]) for t0, t1 in slice_tiles(K, S)])


# ---------------------------------------------------------------------------------------------- cases
def case_id(row):
    sw, layout, M, N, K, epi, ws, ks, _ = row
    return f"{sw + '-' if sw else ''}{layout}-{M}x{N}x{K}-{epi}" + (f"-ws{ws}" if ws else "")


@functools.lru_cache(maxsize=None)
def operands(M, N, K, seed=0):
    """(A bits [M, K], B bits [K, N], C0 fp32 [M, N]) as read-only arrays; logical orientation, the tests lay them out.
    Every product A[m, k] B[k, n] is positive (A's and B's signs follow one random sign per k), so no part of the reduction can vanish
    from the result by cancellation; magnitudes are uniform in [0.5, 1.5), A's scaled by 1/32 outside the row's own run of `heavy`
    consecutive k-tiles, which start at (m * heavy) % nk: every k-tile is heavy for some row (heavy = ceil(nk / M)), and there it is a
    share of the row's sum that a bound of EPS32 K cannot hide even at K = 12288, where one k-tile in 192 of equal weight would be
    0.5 % of the sum against 10 x bound = 1.5 %."""
    rng = np.random.default_rng([M, N, K, seed])
    nk = K // BK
    heavy = -(-nk // M)
    sgn = rng.choice([-1.0, 1.0], size=K)
    tile = np.arange(K) // BK
    first = (np.arange(M) * heavy) % nk
    is_heavy = ((tile[None, :] - first[:, None]) % nk) < heavy
    A = rng.uniform(0.5, 1.5, size=(M, K)) * sgn[None, :] * np.where(is_heavy, 1.0, 1.0 / 32)
    B = rng.uniform(0.5, 1.5, size=(K, N)) * sgn[:, None]
    C0 = (rng.standard_normal((M, N)) * 32).astype(F32)
    out = bf16_bits(A.astype(F32)), bf16_bits(B.astype(F32)), C0
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def products(M, N, K, k_valid=None, seed=0):
    """(A @ B, |A| @ |B|) over the first k_valid rows, float64, computed once per problem"""
    Ab, Bb, _ = operands(M, N, K, seed)
    A, B = bf16_value(Ab).astype(np.float64), bf16_value(Bb).astype(np.float64)
    kv = K if k_valid is None else k_valid
    p = A[:, :kv] @ B[:kv]
    q = np.abs(A[:, :kv]) @ np.abs(B[:kv])
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


def want_and_bound(M, N, K, alpha, accumulate, slices, k_valid=None, seed=0):
    """splitk_f64 and splitk_bound of the seeded problem, from the cached products (the same numbers: test_splitk_ref.py checks that)"""
    p, q = products(M, N, K, k_valid, seed)
    C0 = operands(M, N, K, seed)[2].astype(np.float64)
    kv = K if k_valid is None else k_valid
    want = alpha * p + (C0 if accumulate else 0.0)
    bound = EPS32 * (kv + slices + 2) * (abs(alpha) * q + (np.abs(C0) if accumulate else 0.0))
    return want, bound


def pad_fill(Ab, Bb, k_valid, kind):
    """copies of the operand bits with the reduction rows >= k_valid of BOTH filled: "nan" (bf16 NaN), "huge" (+-3e38, alternating),
    "finite" (+-2 with the signs of row k_valid - 1: each padding row adds about +4 to every output element if it is counted)"""
    Ab, Bb = Ab.copy(), Bb.copy()
    n = Ab.shape[1] - k_valid
    if kind == "nan":
        Ab[:, k_valid:], Bb[k_valid:] = 0x7FC0, 0xFFC1
    elif kind == "huge":
        big = bf16_bits(np.array([3e38, -3e38], dtype=F32))
        Ab[:, k_valid:] = big[(np.arange(n) % 2)][None, :]
        Bb[k_valid:] = big[((np.arange(n) // 2) % 2)][:, None]
    else:
        assert kind == "finite"
        Ab[:, k_valid:] = ((Ab[:, k_valid - 1] & 0x8000) | 0x4000)[:, None]
        Bb[k_valid:] = ((Bb[k_valid - 1] & 0x8000) | 0x4000)[None, :]
    return Ab, Bb


# ---------------------------------------------------------------------------------------------- seeded mistakes
MISTAKES = ["alpha dropped", "one slice left out", "last k-tile of a slice dropped", "one k-tile counted in two slices", "accumulate ignores C0",
            "accumulate once per slice", "padding rows counted", "slice s stored at slice s + 1 (last row tile), stale zero",
            "slice s stored at slice s + 1 (last row tile), stale NaN"]


def mistaken(name, A, B, alpha, C0, accumulate, k_valid, S, bm):
    """float64 result of a kernel that makes the mistake `name` (None where the case cannot show it: alpha == 1, no accumulate, ...).
    A [M, K], B [K, N] float64 with finite padding rows (pad_fill "finite").  The slice the mistake sits in is the one that holds the last
    valid row, and "its last k-tile" the one that holds that row -- slices and k-tiles wholly behind k_valid add nothing either way."""
    K = A.shape[1]
    kv = K if k_valid is None else k_valid
    tiles = slice_tiles(K, S)
    last_tile = (kv - 1) // BK
    s_star = next(s for s, (t0, t1) in enumerate(tiles) if t0 <= last_tile < t1)
    P = partials_f64(A, B, S, kv, alpha)
    add = C0.astype(np.float64) if accumulate else 0.0
    k0, k1 = last_tile * BK, min(kv, (last_tile + 1) * BK)
    one_tile = alpha * (A[:, k0:k1] @ B[k0:k1])
    if name == "alpha dropped":
        return None if alpha == 1.0 else P.sum(0) / alpha + add
    if name == "one slice left out":
        return P.sum(0) - P[s_star] + add
    if name == "last k-tile of a slice dropped":
        return P.sum(0) - one_tile + add
    if name == "one k-tile counted in two slices":
        return P.sum(0) + one_tile + add
    if name == "accumulate ignores C0":
        return P.sum(0) if accumulate else None
    if name == "accumulate once per slice":
        return P.sum(0) + S * add if accumulate else None
    if name == "padding rows counted":
        return None if kv == K else alpha * (A @ B) + add
    stale = {"slice s stored at slice s + 1 (last row tile), stale zero": 0.0, "slice s stored at slice s + 1 (last row tile), stale NaN": np.nan}[name]
    # slice 0's rows of the last row tile land in slot 1 and slot 0 keeps what it held: with a zero there the sum loses slice 1, which
    # shows when slice 1 holds at least one whole valid k-tile; with the NaN the GPU test prefills the workspace with, it always shows
    if stale == 0.0 and kv < (tiles[1][0] + 1) * BK:
        return None
    m0 = (A.shape[0] - 1) // bm * bm
    Q = P.copy()
    Q[1, m0:] = P[0, m0:]
    Q[0, m0:] = stale
    return Q.sum(0) + add
