"""numpy reference of the grouped weight-gradient launch -- hamt_wgrad_grouped / hamt_wgrad_grouped_ex (csrc/gemm_fast.hip:
wgrad_grouped_kernel on the 64 x 128, 128 x 128 and one-phase 256 x 256 tiles of gemm_tile, wgrad_grouped_p8_kernel on the two-phase
256 x 256 tile of p8_tile; contract in include/hamt.h: hamt_wgrad_desc) -- for test_gpu_wgrad.py; no torch, no GPU, nothing of the
package.  tests/test_wgrad_ref.py shows on the CPU that the cases and the bounds tell a wrong kernel from a right one.

  * wgrad_f64 / wgrad_db_f64: dy[:kv].T @ x[:kv] (+ dy2[:kv2].T @ x2[:kv2]) (+ dw0) and the column sums, float64 of the exact bf16 values;
  * wgrad_bound / wgrad_db_bound / wire_bound / SS_CHAIN: the derived bounds;
  * ss_layout / ss_f64: which slots of the tile sums of squares a tile size owns, and what they hold;
  * units: how the launcher cuts a problem with many tiles into XCD-pinned rectangles (restated; the seeded mistakes need it);
  * the cases per tile setting with their seeded operands, and the seeded mistakes.

The bounds (derived, not measured; the argument of _splitk_ref.splitk_bound).  A product of two bf16 values (8 significant bits each) is
exact in fp32, so only additions round.  Whatever order the MFMA and the k loop add the products in, a product passes through at most
kv + kv2 - 1 additions before the tile leaves the accumulators (each at most EPS32 / 2 relative, so (kv + kv2) EPS32 is generous), one
more for the accumulate into dW0 / db0, one rounding for the wire scale:
    |dW - want| <= EPS32 (kv + kv2 + 3) (|dy|^T |x| + |dy2|^T |x2| + |dw0|)     per element,
    |db - want| <= EPS32 (kv + kv2 + 3) (sum |dy| + sum |dy2| + |db0|)          per row.
The wire value bf16(wire_scale dW) gets the same bound times |wire_scale| plus the half-ulp of round-to-nearest bf16.  bf16 has 8
significant bits, so in the binade [2^e, 2^(e+1)) the spacing is 2^(e-7) and the half-ulp 2^(e-8): between 2^-9 |v| (top of the
binade) and 2^-8 |v| (bottom).  2^-9 |wire_scale want| alone is therefore NOT a bound -- 32.57 rounds to 32.5, 0.0725 away, 2^-9 of
it is 0.0636; test_wgrad_ref.py asserts that its correctly rounded restatement leaves it -- and wire_bound takes the exact half-ulp of the binade,
the binade being that of the largest value the first term admits around `want` (a statement about the reference, not about what the
GPU returned).

The tile sums of squares are checked per slot against the float64 sum of squares of the fp32 dW the kernel itself stored, read back,
so dW's own error does not enter: every term v * v is positive, rounds once as a product and then passes through at most c additions,
    |ss[slot] - sum v^2| <= EPS32 (c + 2) sum v^2,        c = SS_CHAIN[tile rows]:
  * 64 x 128, 256 threads (gemm_tile's staged epilogue): a thread owns 8 columns of the rows (t >> 4) + 16 p, p < 4: 32 terms added one
    after the other into tile_ssq (epi_store); wave_sum: 6 shuffle additions; tile_sumsq_store's loop over the 4 waves: 4.  c = 42;
  * 128 x 128, 256 threads: the same with p < 8: 64 terms + 6 + 4.  c = 74;
  * 256 x 256, 512 threads, two-phase (p8_tile: two halves of 8 row pieces of 8 columns = 128 terms per thread through epi_fast8 or
    epi_store) and one-phase (gemm_tile stores from the MFMA layout: 8 x 4 fragments of 4 values = 128 terms): 128 + 6 + 8.  c = 142."""
import collections
import functools

import numpy as np

import _splitk_ref as S
from _smallops_ref import EPS32, F32, bf16_bits, bf16_value

BK = 64
SS_CHAIN = {64: 42, 128: 74, 256: 142}
UNIT_TILES = 12                                  # tiles per XCD-pinned unit (the launcher's default)
WG_MAX = 192                                     # table entries one table-write launch carries
FILLS = ("nan", "huge", "finite")
SETTINGS = {                                     # name -> (environment read per call, the tile rows the setting's cases are meant for)
    "64": ({"HAMT_WGRAD_TILE": "64"}, 64),
    "128": ({"HAMT_WGRAD_TILE": "128"}, 128),
    "256": ({"HAMT_WGRAD_TILE": "256"}, 256),
    "auto256": ({"HAMT_WGRAD_MIN256": "1"}, 256),   # the launcher's own choice, a handful of tiles still taking the 256 class
    "auto128": ({"HAMT_WGRAD_MIN128": "1"}, 128),   # ... the 128-row tile
    "auto": ({}, 64),                               # what ships: this few tiles fold into the 64-row tiles
}
ENV_NAMES = ("HAMT_WGRAD_TILE", "HAMT_WGRAD_MIN256", "HAMT_WGRAD_MIN128", "HAMT_WGRAD_UNIT_TILES", "HAMT_WGRAD_UNIT_2D")

# One problem of a call.  kv / kv2: K_valid / K2_valid (0: every row counts); db: 0 none, 1 store (into a NaN-prefilled buffer),
# 2 accumulate (onto db0); wire: wire_scale (0: fp32 dW); fill: what the padding rows hold; rows: the tile rows the case NAMES for this
# problem (asserted from hamt_debug_wgrad_times and from the ss slots); wide: operand rows >= 256 elements (the 256 class's condition);
# ldw_pad: ldw - N for an fp32 dW (a wire dW has the next multiple of 8 above N + 8).
Prob = collections.namedtuple("Prob", "M N K kv K2 kv2 acc db ss wire fill rows wide ldw_pad seed")


def prob(M, N, K, rows, kv=0, K2=0, kv2=0, acc=0, db=1, ss=True, wire=0.0, fill="nan", wide=None, ldw_pad=5, seed=0):
    return Prob(M, N, K, kv, K2, kv2, acc, db, bool(ss) and wire == 0.0, wire, fill, rows, rows == 256 if wide is None else wide, ldw_pad, seed)


def bn_of(bm):
    return 256 if bm == 256 else 128


def kv_of(p):
    return p.kv if 0 < p.kv < p.K else p.K


def kv2_of(p):
    return 0 if not p.K2 else (p.kv2 if 0 < p.kv2 < p.K2 else p.K2)


def keff(kv):
    return -(-kv // BK) * BK


def takes_256(p):
    """the launcher's condition for the 256 class (before the tile setting folds the classes)"""
    return p.wide and keff(kv_of(p)) >= 128 and (not p.K2 or keff(kv2_of(p)) >= 128)


def leading_dims(p):
    """(column offset of the operand slices in their buffers, ldy, ldx, ldy2, ldx2, ldw): slices at an even 8-column offset (16 bytes),
    at least 8 columns of bf16 NaN behind the last one, the minima 64 / 128 (or 256) where the slice fits them"""
    off = 8
    lo_y, lo_x = (256, 256) if p.wide else (64, 128)
    ldy, ldx = max(lo_y, (off + p.M + 8 + 7) // 8 * 8), max(lo_x, (off + p.N + 8 + 7) // 8 * 8)
    ldw = (p.N + 8 + 8) // 8 * 8 if p.wire else p.N + p.ldw_pad
    return off, ldy, ldx, ldy + 16, ldx + 24, ldw


# ---------------------------------------------------------------------------------------------- the statements
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def wgrad_f64(dy, x, dw0=None, accumulate=False, k_valid=None, dy2=None, x2=None, k2_valid=None):
    """dy[:kv].T @ x[:kv] (+ dy2[:kv2].T @ x2[:kv2]) (+ dw0), float64.  dy [K, M], x [K, N] hold the exact values of the bf16 operands"""
    dy, x = _f64(dy), _f64(x)
    kv = dy.shape[0] if k_valid is None else k_valid
    out = dy[:kv].T @ x[:kv]
    if dy2 is not None:
        dy2, x2 = _f64(dy2), _f64(x2)
        kv2 = dy2.shape[0] if k2_valid is None else k2_valid
        out = out + dy2[:kv2].T @ x2[:kv2]
    return out + _f64(dw0) if accumulate else out


def wgrad_db_f64(dy, db0=None, accumulate=False, k_valid=None, dy2=None, k2_valid=None):
    """the column sums of dy[:kv] (+ of dy2[:kv2]) (+ db0), float64"""
    dy = _f64(dy)
    kv = dy.shape[0] if k_valid is None else k_valid
    out = dy[:kv].sum(0)
    if dy2 is not None:
        dy2 = _f64(dy2)
        out = out + dy2[:(dy2.shape[0] if k2_valid is None else k2_valid)].sum(0)
    return out + _f64(db0) if accumulate else out


def wgrad_bound(dy, x, dw0=None, accumulate=False, k_valid=None, dy2=None, x2=None, k2_valid=None):
    kv = np.shape(dy)[0] if k_valid is None else k_valid
    kv2 = 0 if dy2 is None else (np.shape(dy2)[0] if k2_valid is None else k2_valid)
    mag = wgrad_f64(np.abs(_f64(dy)), np.abs(_f64(x)), None if dw0 is None else np.abs(_f64(dw0)), accumulate, k_valid,
                    None if dy2 is None else np.abs(_f64(dy2)), None if x2 is None else np.abs(_f64(x2)), k2_valid)
    return EPS32 * (kv + kv2 + 3) * mag


def wgrad_db_bound(dy, db0=None, accumulate=False, k_valid=None, dy2=None, k2_valid=None):
    kv = np.shape(dy)[0] if k_valid is None else k_valid
    kv2 = 0 if dy2 is None else (np.shape(dy2)[0] if k2_valid is None else k2_valid)
    mag = wgrad_db_f64(np.abs(_f64(dy)), None if db0 is None else np.abs(_f64(db0)), accumulate, k_valid, None if dy2 is None else np.abs(_f64(dy2)), k2_valid)
    return EPS32 * (kv + kv2 + 3) * mag


def wire_bound(want_dw, bound_dw, scale):
    """bound of bf16(scale dW) around scale want_dw: |scale| bound_dw + half an ulp of bf16 in the binade of the largest value the first
    term admits, 2^(floor(log2 v) - 8) for the 8 significant bits of bf16"""
    first = abs(scale) * bound_dw
    return first + np.exp2(np.floor(np.log2(np.abs(scale * want_dw) + first)) - 8)


def ss_layout(M, N, bm, bn):
    """boolean [ceil(M / 64), ceil(N / 128)]: the slots that must be non-zero -- the origins of the bm x bn tiles in units of 64 rows x 128
    columns; every other slot must be +0.0 exactly"""
    m = np.zeros((-(-M // 64), -(-N // 128)), dtype=bool)
    m[::bm // 64, ::bn // 128] = True
    return m


def ss_f64(dw, bm, bn):
    """float64 [ceil(M / 64), ceil(N / 128)]: each tile's sum of squares of dw (the fp32 values a kernel stored) in its origin slot, 0 elsewhere"""
    dw = _f64(dw)
    M, N = dw.shape
    out = np.zeros((-(-M // 64), -(-N // 128)))
    for m0 in range(0, M, bm):
        for n0 in range(0, N, bn):
            out[m0 // 64, n0 // 128] = np.sum(dw[m0:m0 + bm, n0:n0 + bn] ** 2)
    return out


def ss_bound(ss_want, bm):
    return EPS32 * (SS_CHAIN[bm] + 2) * ss_want


def units(M, N, bm, unit_tiles=UNIT_TILES):
    """[(m_lo, m_rows, n_lo, n_cols)]: the launcher's units of one problem (wgrad_grouped_impl, restated): rectangles of r x c tiles with
    r c <= unit_tiles (a single tile row always allowed), at most ceil(M / 64) of them, fewest operand panel reads, then most tiles"""
    bn = bn_of(bm)
    tm, tn = -(-M // bm), -(-N // bn)
    best, ur, uc = -1, 1, 1
    for r in range(1, tm + 1):
        for c in range(1, tn + 1):
            if r * c > unit_tiles and not (r == 1 and c == tn):
                continue
            if -(-tm // r) * -(-tn // c) > -(-M // 64):
                continue
            panels = sum(min(r, tm - r0) + min(c, tn - c0) for r0 in range(0, tm, r) for c0 in range(0, tn, c))
            if best < 0 or panels < best or (panels == best and r * c > ur * uc):
                best, ur, uc = panels, r, c
    return [(r0 * bm, min(ur * bm, M - r0 * bm), c0 * bn, min(uc * bn, N - c0 * bn)) for r0 in range(0, tm, ur) for c0 in range(0, tn, uc)]


def table_entries(probs, bm_of):
    """entries the launch table of a call needs: its units (bm_of(p) = the tile rows p runs on)"""
    return sum(len(units(p.M, p.N, bm_of(p))) for p in probs if p.K > 0)


# ---------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def operands(M, N, K, K2=0, seed=0):
    """(dy bits [K, M], x bits [K, N], dy2 bits [K2, M] or None, x2 bits [K2, N] or None, dw0 fp32 [M, N], db0 fp32 [M]), read-only.
    _splitk_ref.operands' construction per pair, stored [K][M] / [K][N]: every product dy[k, m] x[k, n] is positive (one random sign per
    k), so no part of a reduction can vanish by cancellation, and each output row m has its own heavy k-tile (the others are 1/32 of
    it), so a lost k-tile is most of some row's sum"""
    A, B, C0 = S.operands(M, N, K, seed)
    dy2 = x2 = None
    if K2:
        A2, B2, _ = S.operands(M, N, K2, seed + 101)
        dy2, x2 = np.ascontiguousarray(A2.T), B2
    db0 = (np.random.default_rng([M, N, K, K2, seed, 7]).standard_normal(M) * 8).astype(F32)
    out = (np.ascontiguousarray(A.T), B, dy2, x2, C0, db0)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def padded(p, fill=None):
    """(dy, x, dy2, x2) bits of p with the rows >= K_valid (K2_valid) of BOTH operands of a pair filled (_splitk_ref.pad_fill)"""
    dy, x, dy2, x2, _, _ = operands(p.M, p.N, p.K, p.K2, p.seed)
    fill = fill or p.fill
    if kv_of(p) < p.K:
        a, b = S.pad_fill(np.ascontiguousarray(dy.T), x, kv_of(p), fill)
        dy, x = np.ascontiguousarray(a.T), b
    if p.K2 and kv2_of(p) < p.K2:
        a, b = S.pad_fill(np.ascontiguousarray(dy2.T), x2, kv2_of(p), fill)
        dy2, x2 = np.ascontiguousarray(a.T), b
    return dy, x, dy2, x2


def values(p, fill="finite"):
    """float64 (dy, x, dy2, x2) with the padding rows filled"""
    return tuple(None if b is None else bf16_value(b).astype(np.float64) for b in padded(p, fill))


@functools.lru_cache(maxsize=None)
def want_and_bounds(p):
    """{"dw", "dw_bound", "db", "db_bound"} (+ "wire", "wire_bound") of the seeded problem, float64, read-only"""
    dy, x, dy2, x2 = values(p)
    _, _, _, _, dw0, db0 = operands(p.M, p.N, p.K, p.K2, p.seed)
    a = (kv_of(p), dy2, x2, kv2_of(p) if p.K2 else None)
    out = {"dw": wgrad_f64(dy, x, dw0, bool(p.acc), *a), "dw_bound": wgrad_bound(dy, x, dw0, bool(p.acc), *a),
           "db": wgrad_db_f64(dy, db0, p.db == 2, a[0], dy2, a[3]), "db_bound": wgrad_db_bound(dy, db0, p.db == 2, a[0], dy2, a[3])}
    if p.wire:
        out["wire"], out["wire_bound"] = p.wire * out["dw"], wire_bound(out["dw"], out["dw_bound"], p.wire)
    for v in out.values():
        v.setflags(write=False)
    return out


def restate32(p):
    """(dW, db) of an fp32 computation that sums in k-tile order: every k-tile's masked product rounded once, added in order (the second
    pair's behind the first's), then + dw0 / db0 -- a right kernel, for test_wgrad_ref.py"""
    dy, x, dy2, x2 = values(p)
    _, _, _, _, dw0, db0 = operands(p.M, p.N, p.K, p.K2, p.seed)
    acc, cs = np.zeros((p.M, p.N), dtype=F32), np.zeros(p.M, dtype=F32)
    for a, b, kv in ((dy, x, kv_of(p)), (dy2, x2, kv2_of(p))):
        for k0 in range(0, kv, BK):
            k1 = min(kv, k0 + BK)
            acc = acc + (a[k0:k1].T @ b[k0:k1]).astype(F32)
            cs = cs + a[k0:k1].sum(0).astype(F32)
    return (acc + dw0 if p.acc else acc), (cs + db0 if p.db == 2 else cs)


# ---------------------------------------------------------------------------------------------- cases
EDGES = [(1, 1), (63, 127), (64, 128), (65, 129), (127, 255), (129, 257), (255, 131), (257, 255), (256 + 58, 384)]
REDUCTIONS = (64, 128, 192, 320)
PAIRS = [(64, 64), (128, 128), (128, 320), (320, 128), (192, 64)]
UNIT_SHAPES = {64: (320, 640), 128: (640, 640), 256: (1024 + 58, 1024 + 100)}      # 25 tiles each


def k_valid_positions(K):
    """K - 1; the 32-row half of the last k-tile (K - 31, K - 32, K - 33); a whole k-tile less (K - 63, K - 64); 65, 64, 1"""
    return sorted({kv for kv in (K - 1, K - 31, K - 32, K - 33, K - 63, K - 64, 65, 64, 1) if 0 < kv < K}, reverse=True)


def _rows(bm, small, wide, K, kv=0, K2=0, kv2=0):
    """tile rows a problem meant for `bm` runs on: a 256-class problem whose keff (keff2) is one k-tile is demoted to the small tiles"""
    if bm != 256:
        return bm
    ok = wide and keff(kv if 0 < kv < K else K) >= 128 and (not K2 or keff(kv2 if 0 < kv2 < K2 else K2) >= 128)
    return 256 if ok else small


@functools.lru_cache(maxsize=None)
def cases(setting):
    """[(case id, [Prob, ...])] of one tile setting: every list is ONE hamt_wgrad_grouped call"""
    bm = SETTINGS[setting][1]
    forced = setting in ("64", "128", "256")
    small = 64                                   # what the 256 settings leave to the other class (HAMT_WGRAD_TILE=256 forces nothing there)
    wide = bm == 256 or setting == "auto"        # ("auto": problems that COULD take the 256 class, folded into the 64-row tiles)
    out = []

    def P(M, N, K, **kw):
        return prob(M, N, K, _rows(bm, small, wide, K, kw.get("kv", 0), kw.get("K2", 0), kw.get("kv2", 0)), wide=wide, **kw)

    # output edges x reductions: store and accumulate, db none / store / accumulate, ss, every third problem a wire output; the
    # second call shifts every choice by one
    for shift in (0, 1):
        ps = []
        for i, (M, N) in enumerate(EDGES):
            j = i + shift
            K = REDUCTIONS[j % 4] if bm != 256 else (128, 192, 320)[j % 3]
            is_wire = j % 3 == 2
            ps.append(P(M, N, K, acc=0 if is_wire else j % 2, db=j % 3 if not is_wire else 1 + (j // 3) % 2, wire=(0.5, -1.0 / 3)[j % 2] if is_wire else 0.0,
                        ldw_pad=(5, 8, 0)[(j // 2) % 3], seed=j))
        out.append((f"edges-{'ab'[shift]}", ps))
        if not forced and setting != "auto256":
            return out                            # "auto" / "auto128": the launcher's decision, once
    # K_valid at every position, padding rows NaN / huge / finite; a 256-class problem whose keff is one k-tile runs on the small tiles
    M, N = bm + 1, bn_of(bm) + 1
    ps = []
    for K in REDUCTIONS:
        for kv in k_valid_positions(K):
            i = len(ps)
            ps.append(P(M, N, K, kv=kv, acc=i % 2, db=1 + i % 2, fill=FILLS[i % 3], seed=K // 64))
    assert bm != 256 or {p.rows for p in ps} == {256, small}
    out.append(("k-valid", ps))
    # the shortest reductions of the 256 tile, alone in their launch: 2 and 3 k-tiles, K_valid across a 32-row half of the last one
    if bm == 256:
        out.append(("p8-nk2-nk3", [P(257, 255, 128, kv=97, fill="huge"), P(255, 257, 192, kv=159, acc=1, db=2, fill="nan", seed=1),
                                   P(256, 256, 128, ldw_pad=0, seed=2), P(256, 256, 192, ldw_pad=0, acc=1, seed=3)]))
    # second operand pair: other leading dimensions, K2_valid at the same positions relative to K2, store / accumulate, with / without db
    ps = []
    for K, K2 in PAIRS:
        for kv2 in [0] + k_valid_positions(K2):
            i = len(ps)
            ps.append(P(M, N, K, K2=K2, kv2=kv2, acc=i % 2, db=(1, 2, 0)[i % 3] if i % 2 else (1, 0)[(i // 2) % 2], fill=FILLS[i % 3], seed=i % 5))
    out.append(("second-pair", ps))
    # units: 25 tiles in one problem, db stored into NaN / accumulated onto db0 exactly once, ss, and the same with a wire output
    UM, UN = UNIT_SHAPES[bm]
    out.append(("units", [P(UM, UN, 128, db=1), P(UM, UN, 128, acc=1, db=2, ldw_pad=8, seed=1), P(UM, UN, 128, db=2, wire=0.5, seed=2),
                          P(UM, UN, 128, db=1, wire=-1.0 / 3, seed=3)]))
    # one problem of one tile alone in a call: seven XCD queues are empty
    out.append(("one-tile", [P(bm, bn_of(bm), 128, ldw_pad=0)]))
    out.append(("one-tile-ragged", [P(bm - 7, bn_of(bm) - 3, 128, acc=1, db=2)]))
    # a call mixing both launch classes: a narrow problem (operand rows of 64 / 128 elements) next to the class's own
    if bm == 256:
        out.append(("both-classes", [P(257, 255, 192), prob(65, 129, 128, small, wide=False, acc=1, db=2, seed=1), P(255, 257, 192, kv=64, seed=2),
                                     prob(64, 128, 64, small, wide=False, seed=3), P(300, 300, 320, K2=128, acc=1, seed=4)]))
    # more than WG_MAX table entries: several table-write launches
    if setting in ("64", "128", "256"):
        out.append(("long-table", [prob(64, 128, 64, small if bm == 256 else bm, wide=wide, acc=i % 2, db=1 + i % 2, ldw_pad=(0, 5)[i % 2], seed=i % 7) for i in range(200)]))
    return out


def class_probs(bm):
    """every problem of every setting's cases that the cases name for tile rows `bm` (the long table once)"""
    seen = {}
    for setting in SETTINGS:
        for cid, ps in cases(setting):
            for p in (ps[:7] if cid == "long-table" else ps):
                if p.rows == bm:
                    seen[p] = None
    return list(seen)


# ---------------------------------------------------------------------------------------------- seeded mistakes
MISTAKES = {      # name -> the quantity it shows in
    "last k-tile dropped": "dw",
    "padding rows counted": "dw",
    "the 32-row half that holds K_valid masked whole": "dw",
    "second pair dropped": "dw",
    "the second pair's tail mask applied at the first pair's index": "dw",
    "accumulate ignores dW0": "dw",
    "db written once per column unit": "db",
    "db misses the rows of the ragged last tile": "db",
    "rows >= M of dY enter the bias sums": "db",
    "ss of the values before accumulation": "ss",
    "ss slot addressed with the unit's own column count instead of the problem's": "ss",
    "ss of the first segment kept instead of the last": "ss",
    "wire value without the scale": "wire",
    "unit's dW offset taken in fp32 elements for a bf16 array": "wire",
}


def mistaken(name, p, bm):
    """float64 result (the quantity MISTAKES[name] names: dW [M, N], db [M], ss [slots], wire [M, N]) of a kernel that makes the mistake
    `name` on problem p with tile rows bm, or None where the case cannot show it.  Padding rows hold pad_fill's "finite" fill.  ss is
    the mistaken kernel's sums over its own (right) dW, so it is compared with ss_f64 of the same dW."""
    dy, x, dy2, x2 = values(p)
    _, _, _, _, dw0, db0 = operands(p.M, p.N, p.K, p.K2, p.seed)
    W = want_and_bounds(p)
    kv, kv2, bn = kv_of(p), kv2_of(p), bn_of(bm)
    la, lb, lkv = (dy2, x2, kv2) if p.K2 else (dy, x, kv)      # the pair that holds the call's last k-tile
    k0 = (lkv - 1) // BK * BK
    last_tile = la[k0:lkv].T @ lb[k0:lkv]
    un = units(p.M, p.N, bm)
    ragged0 = p.M // bm * bm                     # first row of the ragged last row tile (== M: none)
    if name == "last k-tile dropped":
        return W["dw"] - last_tile
    if name == "padding rows counted":
        return None if kv == p.K and kv2 == p.K2 else wgrad_f64(dy, x, dw0, bool(p.acc), None, dy2, x2, None)
    if name == "the 32-row half that holds K_valid masked whole":
        h0 = (lkv - 1) // 32 * 32
        return None if lkv % 32 == 0 else W["dw"] - la[h0:lkv].T @ lb[h0:lkv]
    if name == "second pair dropped":
        return wgrad_f64(dy, x, dw0, bool(p.acc), kv) if p.K2 else None
    if name == "the second pair's tail mask applied at the first pair's index":
        # k-tile kt of the whole reduction in place of kt - nk1: every row of the second pair's last k-tile lies behind K2_valid then
        return W["dw"] - last_tile if p.K2 else None
    if name == "accumulate ignores dW0":
        return W["dw"] - dw0 if p.acc else None
    if name == "db written once per column unit":
        # a store writes the same sums again; an accumulate adds them once per unit of the row band
        ncu = len({u[2] for u in un})
        return W["db"] + (ncu - 1) * wgrad_db_f64(dy, None, False, kv, dy2, kv2 if p.K2 else None) if p.db == 2 and ncu > 1 else None
    if name == "db misses the rows of the ragged last tile":
        if not p.db or ragged0 == p.M:
            return None
        out = W["db"].copy()
        out[ragged0:] = db0[ragged0:] if p.db == 2 else np.nan      # (what the buffer held: db0, or the NaN prefill)
        return out
    if name == "rows >= M of dY enter the bias sums":
        if not p.db or ragged0 == p.M:
            return None
        out = W["db"].copy()
        out[ragged0:] = np.nan                   # bf16 NaN lies behind the operand's last column
        return out
    if name == "wire value without the scale":
        return W["dw"] if p.wire else None
    if name == "unit's dW offset taken in fp32 elements for a bf16 array":
        if not p.wire or len(un) == 1:
            return None
        ldw = leading_dims(p)[5]
        flat = np.full(2 * p.M * ldw + 2 * p.N, np.nan)
        for m_lo, mr, n_lo, nc in un:
            for r in range(mr):
                o = 2 * (m_lo * ldw + n_lo) + r * ldw
                flat[o:o + nc] = W["wire"][m_lo + r, n_lo:n_lo + nc]
        return flat[:p.M * ldw].reshape(p.M, ldw)[:, :p.N]
    if not p.ss:
        return None
    if name == "ss of the values before accumulation":
        return ss_f64(W["dw"] - dw0, bm, bn) if p.acc else None
    if name == "ss of the first segment kept instead of the last":
        return ss_f64(wgrad_f64(dy, x, dw0, bool(p.acc), kv), bm, bn) if p.K2 else None
    assert name == "ss slot addressed with the unit's own column count instead of the problem's"
    right, ld = ss_f64(W["dw"], bm, bn), -(-p.N // 128)
    flat = np.zeros(right.size + ld * right.shape[0])
    for m_lo, mr, n_lo, nc in un:
        uld = -(-nc // 128)
        for m0 in range(0, mr, bm):
            for n0 in range(0, nc, bn):
                flat[(m_lo >> 6) * ld + (n_lo >> 7) + (m0 >> 6) * uld + (n0 >> 7)] = right[(m_lo + m0) >> 6, (n_lo + n0) >> 7]
    out = flat[:right.size].reshape(right.shape)
    return None if np.array_equal(out, right) else out
