"""Plain numpy restatements of the LayerNorm family (csrc/norm.hip on csrc/ln_row.h):  y = dropout_post(LN(dropout_pre(x) + residual)),
its backward, the `add` form of the backward and the column-sum reductions, with the cases and bounds of their op-level tests.
test_ln_ref.py proves on the CPU that the cases tell a wrong kernel from a right one, test_gpu_ln.py runs the kernels on them.
float64 for what a kernel should compute (`ln64`), float32 in the kernel's own order of operations for what fp32 arithmetic can reach
(`ln32`, with a switch for every mistake test_ln_ref.py lists), the integer mask stream of _smallops_ref for the dropout factors.
Nothing here touches torch, the GPU or the package under test.

Constant non-zero rows are left out of the compared cases: their variance is 0, rstd = eps^-1/2 (1e6 at eps = 1e-12) multiplies whatever
rounding the fp32 mean has, and no float64 value is a fair reference for that.  `const_case` holds such rows for a finiteness check only."""
import functools

import numpy as np

from _smallops_ref import CALL_ID, EPS32, F32, SEED, bf16_bits, bf16_value, drop_keep4, drop_scale4, inv_keep32, keep_rate4, rng_key  # noqa: F401

POST_SALT = 0x5BD1E995                   # the post mask's key is call_id ^ POST_SALT, the pre mask's call_id
LNRED_CHUNK = 64                         # entries per kernarg chunk of hamt_ln_bwd_reduce_grouped
KINDS = ("randn", "off30", "off100", "big", "small", "zero", "onehot")
KINDS_PRE = ("randn", "big", "small", "zero", "onehot")      # rows of the p_pre cases: a masked offset row is no offset row any more
DY_SCALES = (1.0, 0.0, 1e3, 1e-3, -1.5)                    # G_CYCLE's idea: a zero row, 1e3 next to 1e-3
ROW_OUTPUTS = ("z", "mean", "rstd", "y", "dz", "dx")
COL_OUTPUTS = ("dgamma", "dbeta", "dxsum")


def nv_of(H):
    """float4 vectors per lane: LN_ROW_DISPATCH"""
    return (H + 255) // 256


def geometry(M):
    """ln_bwd_geometry: waves per block and blocks (= partials) of the backward kernel"""
    nwv = 16 if M >= 2048 else (8 if M >= 1024 else 4)
    return nwv, min(256, -(-M // nwv))


def mpad(M):
    return -(-M // 64) * 64


# ---------------------------------------------------------------------------------------------- cases
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _make_case(name, M, H, seed, eps, has_res, p_pre=0.0, p_post=0.0, kinds=KINDS):
    rng = _rng(1000 + seed)
    kind = [kinds[r % len(kinds)] for r in range(M)]
    x = rng.standard_normal((M, H))
    res = 0.5 * rng.standard_normal((M, H)) if has_res else None
    for r, k in enumerate(kind):
        if k == "off30":
            x[r] += 30.0
        elif k == "off100":
            x[r] = 100.0 + 0.1 * x[r]
        elif k == "big":
            x[r] *= 1e3
        elif k == "small":
            x[r] *= 1e-3
            if has_res:
                res[r] *= 1e-3
        elif k in ("zero", "onehot"):
            x[r] = 0.0
            if has_res:
                res[r] = 0.0
            if k == "onehot":
                x[r, rng.integers(H)] = 3.0 * (1 if rng.integers(2) else -1)
    dy = rng.standard_normal((M, H)) * np.array([DY_SCALES[(3 * r + seed) % len(DY_SCALES)] for r in range(M)])[:, None]
    c = dict(name=name, M=M, H=H, eps=eps, p_pre=p_pre, p_post=p_post, kind=kind, x=x.astype(F32), res=None if res is None else res.astype(F32),
             gamma=(1 + 0.1 * rng.standard_normal(H)).astype(F32), beta=(0.1 * rng.standard_normal(H)).astype(F32), dy=dy.astype(F32),
             add=rng.standard_normal((M, H)).astype(F32))
    c["fpre"], c["fpost"] = mask_factors(c)
    return c


M_NARROW = ((1, 64), (3, 132), (5, 64), (1023, 132), (1024, 64), (1025, 132), (2047, 64), (2048, 132), (4095, 64), (4097, 132), (4100, 64))
H_AT_37 = (4, 12, 64, 132, 256, 260, 516, 768, 1020, 1024)
EXTRA = ((1025, 768), (2049, 1024))
DROPOUT = (("post", 37, 132, 0.0, 0.1), ("post", 130, 256, 0.0, 0.5), ("pre", 37, 132, 0.1, 0.0), ("pre", 1030, 64, 0.5, 0.0),
           ("both", 70, 260, 0.1, 0.5), ("both", 1030, 768, 0.5, 0.1))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  Every M with a narrow H, every H with M = 37, 768 x 1025 and 1024 x 2049; eps alternates between BERT's 1e-12 and
    ViT's 1e-6, every second pair has a residual.  Rows cycle through KINDS (so the row index tests row addressing), dy rows through
    DY_SCALES, gamma / beta differ per column.  The arrays are shared: do not write to them."""
    out = {}
    for i, (M, H) in enumerate(M_NARROW + tuple((37, H) for H in H_AT_37) + EXTRA):
        out[f"{M}x{H}"] = _make_case(f"{M}x{H}", M, H, i, (1e-12, 1e-6)[i % 2], (i // 2) % 2 == 1)
    for j, (what, M, H, pp, pq) in enumerate(DROPOUT):
        name = f"{what} {M}x{H} p {max(pp, pq):g}" if what != "both" else f"both {M}x{H} p {pp:g}/{pq:g}"
        out[name] = _make_case(name, M, H, 100 + j, (1e-12, 1e-6)[j % 2], what != "post", pp, pq, KINDS_PRE if pp > 0 else KINDS)
    return out


def plain_cases():
    return [c for c in cases().values() if c["p_pre"] == 0 and c["p_post"] == 0]


def dropout_cases():
    return [c for c in cases().values() if c["p_pre"] > 0 or c["p_post"] > 0]


GROUPED = ((37, 64), (1023, 128), (1024, 64), (2047, 768), (2048, 128), (1025, 768))
GROUPED_N = LNRED_CHUNK + 1


@functools.lru_cache(maxsize=None)
def grouped_cases():
    """the problems behind the entries of the grouped-reduction test: H of 64, 128 and 768, M on both sides of 1024 and of 2048"""
    return [_make_case(f"grouped {M}x{H}", M, H, 300 + i, 1e-12, False) for i, (M, H) in enumerate(GROUPED)]


@functools.lru_cache(maxsize=None)
def const_case():
    """constant non-zero rows (and one ordinary row): finiteness only, see the module's docstring"""
    c = _make_case("const 9x132", 9, 132, 200, 1e-12, False)
    x = c["x"].copy()
    for r, v in enumerate((3.0, -0.1, 100.0, 1e-3, 1e3, 1.0 / 3.0, -7.7, 65504.0)):
        x[r] = v
    c["x"] = x
    return c


# ---------------------------------------------------------------------------------------------- masks
def mask_factors(c, seed=SEED, epoch=0, call_id=CALL_ID, swap_keys=False, one_key=False, per_column=False):
    """(pre, post) factor arrays [M, H] of fp32 1 / (1 - p) or 0, None where p = 0: drop_scale4 with the key of `call_id` for the pre mask
    and of `call_id ^ POST_SALT` for the post mask.  The mistakes: the two keys swapped, both masks from the pre key, the group index taken
    as the column (one draw per column: the first uniform of every group of a four times wider stream)"""
    kpre, kpost = rng_key(seed, epoch, call_id), rng_key(seed, epoch, call_id ^ POST_SALT)
    if swap_keys:
        kpre, kpost = kpost, kpre
    if one_key:
        kpost = kpre
    M, H = c["M"], c["H"]

    def f(key, p):
        if not p > 0:
            return None
        return np.ascontiguousarray(drop_scale4(key, M, 4 * H, p)[:, ::4]) if per_column else drop_scale4(key, M, H, p)
    return f(kpre, c["p_pre"]), f(kpost, c["p_post"])


# ---------------------------------------------------------------------------------------------- float64 statement
def ln64(c, add=None, x=None):
    """z = x fpre + res; mean, rstd (biased variance, eps inside the root); y = ((z - mean) rstd gamma + beta) fpost;
    a = dy fpost; dgamma = sum_r a xhat; dbeta = sum_r a; dz = rstd (u - mean_c(u) - xhat mean_c(u xhat)) [+ add], u = a gamma;
    dx = (dz without add) fpre; dxsum = sum_r dx.  All from the fp32 input values, in float64."""
    f8 = np.float64
    x = c["x"] if x is None else x
    one = f8(1)
    fpre = one if c["fpre"] is None else c["fpre"].astype(f8)
    fpost = one if c["fpost"] is None else c["fpost"].astype(f8)
    z = x.astype(f8) * fpre + (0 if c["res"] is None else c["res"].astype(f8))
    mean = z.mean(axis=1)
    var = ((z - mean[:, None]) ** 2).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + f8(F32(c["eps"])))
    xh = (z - mean[:, None]) * rstd[:, None]
    g = c["gamma"].astype(f8)
    y = (xh * g + c["beta"].astype(f8)) * fpost
    a = c["dy"].astype(f8) * fpost
    u = a * g
    r = rstd[:, None] * (u - u.mean(axis=1, keepdims=True) - xh * (u * xh).mean(axis=1, keepdims=True))
    dx = r * fpre
    cond = np.maximum(1.0, np.abs(mean) / np.where(var > 0, np.sqrt(np.where(var > 0, var, 1.0)), np.inf))
    return dict(z=z, mean=mean, rstd=rstd, sigma=np.sqrt(var), cond=cond, xh=xh, a=a, y=y, dz=r if add is None else r + add.astype(f8), dx=dx,
                dgamma=(a * xh).sum(axis=0), dbeta=a.sum(axis=0), dxsum=dx.sum(axis=0))


# ---------------------------------------------------------------------------------------------- fp32, the kernels' order of operations
def col_sums32(term, M, mut=None):
    """Column sums as ln_bwd_kernel and the reduce kernels take them: wave w of block b adds its rows b nwv + w + k nb nwv in order, the
    upper waves fold into the lower (half = nwv / 2 ... 4), the block's partial is ((w0 + w1) + w2) + w3, and the nb partials are summed
    as 16 phases (b, b + 16, ...) whose sums are added in order.
    The mistakes: drop_wave = w (that wave's partial left out), drop_last_block, drop_trip2 (rows >= 256 nwv left out)."""
    mut = mut or {}
    nwv, nb = geometry(M)
    H = term.shape[1]
    span = nb * nwv
    trips = -(-M // span)
    pad = np.zeros((trips * span, H), dtype=F32)
    pad[:M] = term
    if mut.get("drop_trip2"):
        pad[256 * nwv:] = 0
    P = np.zeros((nb, nwv, H), dtype=F32)
    for t in range(trips):
        P = P + pad[t * span:(t + 1) * span].reshape(nb, nwv, H)
    if mut.get("drop_wave") is not None:
        P[:, mut["drop_wave"]] = 0
    half = nwv // 2
    while half >= 4:
        P[:, :half] = P[:, :half] + P[:, half:2 * half]
        half //= 2
    B = ((P[:, 0] + P[:, 1]) + P[:, 2]) + P[:, 3]
    if mut.get("drop_last_block"):
        B[nb - 1] = 0
    return sum_partials32(B)


def sum_partials32(B):
    """ln_bwd_reduce_kernel / reduce_partials: [nb, H] -> [H]"""
    ph = np.zeros((16, B.shape[1]), dtype=F32)
    for b in range(B.shape[0]):
        ph[b % 16] = ph[b % 16] + B[b]
    t = ph[0].copy()
    for i in range(1, 16):
        t = t + ph[i]
    assert t.dtype == F32
    return t


def _image(v, M):
    """bf16 image [Mpad16, H] of v [M, H]: rounded rows, zero padding rows"""
    img = np.zeros((mpad(M), v.shape[1]), dtype=np.uint16)
    img[:M] = bf16_bits(v)
    return img


PAD_FILL = 0x7FC0                        # what a never-written padding row of a bf16 image holds in the restated mistake (a NaN)


def ln32(c, mut=None, add=None, x=None):
    """ln_fwd_kernel / ln_bwd_kernel in fp32: two-pass variance, / (float)H, rsqrt(var + eps), (v - m) r g + b, r (u - c1 - n c2); row
    sums in numpy's (pairwise) order, column sums as col_sums32.  `mut` switches the mistakes on:
      statistics    one_pass, eps_outside, div_hm1, div_padded (256 NV), count_dead (the dead columns of the last vector enter the variance)
      row terms     no_c1, no_c2, no_rstd, dgamma_dyg, dg_before_post, neighbour_stats
      column sums   drop_wave = w, drop_last_block, drop_trip2, dxsum_dz, add_leaks
      masks         swap_keys, one_key, per_column, pre_not_on_dx, dropped_not_zero
      images        pad_unzeroed"""
    mut = mut or {}
    x = c["x"] if x is None else x
    M, H = c["M"], c["H"]
    fpre, fpost = c["fpre"], c["fpost"]
    if any(mut.get(k) for k in ("swap_keys", "one_key", "per_column")):
        fpre, fpost = mask_factors(c, swap_keys=mut.get("swap_keys", False), one_key=mut.get("one_key", False), per_column=mut.get("per_column", False))
    if mut.get("dropped_not_zero") and fpost is not None:
        fpost = np.where(fpost == 0, F32(2.0 ** -20), fpost)
    v = x.astype(F32)
    if fpre is not None:
        v = v * fpre
    if c["res"] is not None:
        v = v + c["res"]
    Hf = F32(H - 1 if mut.get("div_hm1") else (256 * nv_of(H) if mut.get("div_padded") else H))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mean = v.sum(axis=1, dtype=F32) / Hf
        if mut.get("one_pass"):
            var = (v * v).sum(axis=1, dtype=F32) / Hf - mean * mean
        else:
            e = v - mean[:, None]
            sq = (e * e).sum(axis=1, dtype=F32)
            if mut.get("count_dead"):
                sq = sq + F32(256 * nv_of(H) - H) * (mean * mean)
            var = sq / Hf
        eps = F32(c["eps"])
        rstd = (F32(1) / (np.sqrt(var) + eps)) if mut.get("eps_outside") else (F32(1) / np.sqrt(var + eps))
        y = ((v - mean[:, None]) * rstd[:, None]) * c["gamma"] + c["beta"]
        if fpost is not None:
            y = y * fpost
        # backward
        bm, br = (np.roll(mean, -1), np.roll(rstd, -1)) if mut.get("neighbour_stats") else (mean, rstd)
        a = c["dy"] if fpost is None else c["dy"] * fpost
        h = (v - bm[:, None]) * br[:, None]
        a_par = c["dy"] if mut.get("dg_before_post") else a
        if mut.get("add_leaks") and add is not None:
            a_par = a_par + add
        dgt = ((a_par * c["gamma"]) * h) if mut.get("dgamma_dyg") else a_par * h
        u = a * c["gamma"]
        c1 = F32(0) if mut.get("no_c1") else (u.sum(axis=1, dtype=F32) / F32(H))[:, None]
        c2 = F32(0) if mut.get("no_c2") else ((u * h).sum(axis=1, dtype=F32) / F32(H))[:, None]
        r = u - c1 - h * c2
        if not mut.get("no_rstd"):
            r = br[:, None] * r
        dz = r if add is None else r + add
        dx = r if (fpre is None or mut.get("pre_not_on_dx")) else r * fpre
        dxt = dz if mut.get("dxsum_dz") else dx
        if mut.get("add_leaks") and add is not None:
            dxt = dx + add
        out = dict(z=v, mean=mean, rstd=rstd, y=y, dz=dz, dx=dx, dgamma=col_sums32(dgt, M, mut), dbeta=col_sums32(a_par, M, mut),
                   dxsum=col_sums32(dxt, M, mut), y16=_image(y, M), dx16=_image(dx, M))
    if mut.get("pad_unzeroed"):
        out["y16"][M:] = PAD_FILL
        out["dx16"][M:] = PAD_FILL
    assert all(out[k].dtype == F32 for k in ROW_OUTPUTS + COL_OUTPUTS)
    return out


def grouped32(entries, start, mut=None):
    """hamt_ln_bwd_reduce_grouped: entries of dict(ws = partials [nb, 3, H], out = (name | None) x 3, atomic), `start`: name -> what the
    output buffer holds before.  Output i of an entry is stored, or added where bit i of `atomic` is set -> name -> values after.
    The mistake: invert_atomic (the bit read inverted)."""
    mut = mut or {}
    bufs = {k: np.asarray(v, dtype=F32).copy() for k, v in start.items()}
    for e in entries:
        for i, name in enumerate(e["out"]):
            if name is None:
                continue
            t = sum_partials32(e["ws"][:, i])
            bit = (e["atomic"] >> i) & 1
            if mut.get("invert_atomic"):
                bit ^= 1
            bufs[name] = bufs[name] + t if bit else t
    return bufs


# ---------------------------------------------------------------------------------------------- errors in the units of the bounds
def _worst(d):
    d = np.asarray(d, dtype=np.float64)
    return 0.0 if d.size == 0 else float(np.where(np.isnan(d), np.inf, d).max())


def _exact_or_inf(got, want):
    return 0.0 if np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)) else np.inf


def errors(c, out, add=None, x=None, ref=None):
    """{(output, kind): worst error} for the outputs present in `out`.
    Row outputs, per row and then worst per row kind: z, y, dz, dx as max_c |err| / max_c |float64 row| (the output's own scale per row);
    rstd relative; mean relative to max(|mean|, sigma).  A float64 row of exact zeros has to be met exactly (a zero dy row, the zero
    input row), and so have the dropped positions of y, dx and z (= the residual there): anything else counts as an infinite error.
    Column outputs, kind None: worst |err_c| / (eps32 U_c) where U_c sums over the rows what one rounding of that row's term can move:
    dbeta |a|, dgamma cond |a| (1 + |xhat|), dxsum cond max_c |dx row|, cond = max(1, |mean| / sigma) being the row's amplification of the
    fp32 mean's rounding -- so the offset rows widen a column's unit by what they themselves can add and no more."""
    ref = ln64(c, add=add, x=x) if ref is None else ref
    kinds = np.array(c["kind"])
    res = {}

    def by_kind(name, e):
        for k in sorted(set(c["kind"])):
            res[name, k] = _worst(e[kinds == k])

    def rows(name, got, want, exact_mask=None):
        got = np.asarray(got, dtype=np.float64)
        scale = np.abs(want).max(axis=1)
        e = np.abs(got - want).max(axis=1) / np.where(scale > 0, scale, 1.0)
        e = np.where(np.isnan(e), np.inf, e)
        e[(scale == 0) & (np.abs(got).max(axis=1) != 0)] = np.inf
        if exact_mask is not None:
            e[((got != want) & exact_mask).any(axis=1)] = np.inf
        by_kind(name, e)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dropped_pre = None if c["fpre"] is None else c["fpre"] == 0
        dropped_post = None if c["fpost"] is None else c["fpost"] == 0
        if "z" in out:
            rows("z", out["z"], ref["z"], dropped_pre)
        if "y" in out:
            rows("y", out["y"], ref["y"], dropped_post)
        if "dz" in out:
            rows("dz", out["dz"], ref["dz"])
        if "dx" in out:
            rows("dx", out["dx"], ref["dx"], dropped_pre)
        if "rstd" in out:
            by_kind("rstd", np.abs(np.asarray(out["rstd"], dtype=np.float64) - ref["rstd"]) / ref["rstd"])
        if "mean" in out:
            got = np.asarray(out["mean"], dtype=np.float64)
            den = np.maximum(np.abs(ref["mean"]), ref["sigma"])
            e = np.abs(got - ref["mean"]) / np.where(den > 0, den, 1.0)
            e[(den == 0) & (got != 0)] = np.inf
            by_kind("mean", e)
        units = col_units(ref)
        for name in COL_OUTPUTS:
            if name in out:
                got, U = np.asarray(out[name], dtype=np.float64), units[name]
                e = np.abs(got - ref[name]) / (EPS32 * np.where(U > 0, U, 1.0))
                e = np.where(np.isnan(e), np.inf, e)
                e[(U == 0) & (got != 0)] = np.inf
                res[name, None] = _worst(e)
    return res


def col_units(ref):
    """U_c of the column outputs (see `errors`) from an ln64 result"""
    cond = ref["cond"][:, None]
    return dict(dbeta=np.abs(ref["a"]).sum(axis=0), dgamma=(cond * np.abs(ref["a"]) * (1 + np.abs(ref["xh"]))).sum(axis=0),
                dxsum=(cond[:, 0] * np.abs(ref["dx"]).max(axis=1)).sum() * np.ones(ref["a"].shape[1]))


def image_errors(bits, value, M):
    """a bf16 image [Mpad16, H] against the fp32 tensor it images: (elements that are not the rounding of `value`, non-zero padding elements)"""
    bits = np.asarray(bits, dtype=np.uint16)
    return int((bits[:M] != bf16_bits(value)).sum()), int(np.count_nonzero(bits[M:mpad(M)]))


# Worst values of the fp32 restatement `ln32` against `ln64` over cases(), as printed by
# test_ln_ref.py::test_fp32_restatement_is_inside_the_measured_caps (which also asserts that none is exceeded), rounded up to two digits.
# Row outputs: relative errors per row kind (see `errors`); the offset rows carry the fp32 mean's rounding, eps32 |mean| / sigma (4e-6 for
# 30 + randn, 1e-4 for 100 + 0.1 randn), into everything that goes through xhat, in caps of their own.  Column outputs: units of eps32 U_c.
# The GPU bound is 8 x the measured cap: the wave-shuffle and LDS sums run in another order than numpy's pairwise row sums.
ROW_MEASURED = {
    "z": {"randn": 6.8e-08, "off30": 6e-08, "off100": 3.8e-08, "big": 8.6e-08, "small": 6.8e-08, "zero": 0, "onehot": 0},
    "mean": {"randn": 6.6e-08, "off30": 1.4e-07, "off100": 1.4e-07, "big": 5.9e-08, "small": 7.4e-08, "zero": 0, "onehot": 2.7e-09},
    "rstd": {"randn": 1.7e-07, "off30": 7.3e-07, "off100": 3.8e-06, "big": 1.5e-07, "small": 1.4e-07, "zero": 6.3e-08, "onehot": 3.5e-07},
    "y": {"randn": 2.7e-07, "off30": 2.2e-06, "off100": 6.8e-05, "big": 2.8e-07, "small": 2.6e-07, "zero": 5e-08, "onehot": 4.2e-07},
    "dz": {"randn": 3.9e-07, "off30": 1.6e-06, "off100": 3.4e-05, "big": 2.6e-07, "small": 2.6e-07, "zero": 2.4e-07, "onehot": 5.6e-07},
    "dx": {"randn": 3.9e-07, "off30": 1.6e-06, "off100": 3.4e-05, "big": 2.6e-07, "small": 2.3e-07, "zero": 2.1e-07, "onehot": 5.6e-07},
}
COL_MEASURED = {"dgamma": 1.0, "dbeta": 1.5, "dxsum": 1.9}
GPU_MARGIN, CAUGHT_FACTOR = 8.0, 10.0
ONE_ROUNDING = 2.0 ** -24


def cap(name, kind=None):
    """The measured value; for a row output that is not exact (measured > 0) at least one fp32 rounding, 2^-24: where the restatement's
    few roundings happened to fall well (the mean of a one-hot row is a single division) the measured value says nothing about another
    order of the same sums.  An exact 0 stays 0: such an output has to be met bit for bit."""
    if kind is None:
        return COL_MEASURED[name]
    m = ROW_MEASURED[name][kind]
    return max(m, ONE_ROUNDING) if m > 0 else 0.0


def measured(name, kind=None):
    return COL_MEASURED[name] if kind is None else ROW_MEASURED[name][kind]


def bound(name, kind=None):
    return GPU_MARGIN * cap(name, kind)


def worst_ratio(errs, cap_fn=bound):
    """{output: worst error / bound over the row kinds} of an `errors` result (0 / 0 counts as 0: an exact output with a zero cap)"""
    out = {}
    for (name, kind), e in errs.items():
        b = cap_fn(name, kind)
        r = (0.0 if e == 0 else np.inf) if b == 0 else e / b
        out[name] = max(out.get(name, 0.0), r)
    return out
