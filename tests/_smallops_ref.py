"""Plain numpy restatements of the loss, dropout and small-reduction kernels (csrc/loss.hip, the elementwise half of csrc/elementwise.hip,
hamt_colsum / hamt_smallk_wgrad of csrc/gemm.hip, the counter-based RNG of csrc/common.h) and the cases of their op-level tests:
test_smallops_ref.py proves on the CPU that the cases can tell a wrong kernel from a right one, test_gpu_losses.py and
test_gpu_smallops.py run the kernels on them.  float64 for what a kernel should compute, float32 in the kernel's own order of
operations for what fp32 arithmetic can reach, 32-bit integers for the RNG.  Nothing here touches torch, the GPU or the package under test."""
import functools
import math

import numpy as np

F32 = np.float32
EPS32 = 2.0 ** -23

# Worst values of the fp32 restatement on the cases below, in the units of `row_unit` (CE, KL) / of eps32 |g| (GELU'), as printed by
# test_smallops_ref.py::test_fp32_restatement_is_inside_the_bounds (which also asserts that they are not exceeded).  Each GPU bound is
# 8 x the measured value: the device's expf / logf / erff are a few ulp where numpy's float64 ones, rounded once, are correctly rounded.
CE_LOSS_MEASURED, CE_TERM_MEASURED = 0.80, 0.33
KL_LOSS_MEASURED, KL_TERM_MEASURED = 0.76, 0.34
DGELU_MEASURED = 1.03
CE_LOSS_BOUND, CE_TERM_BOUND = 8 * CE_LOSS_MEASURED, 8 * CE_TERM_MEASURED
KL_LOSS_BOUND, KL_TERM_BOUND = 8 * KL_LOSS_MEASURED, 8 * KL_TERM_MEASURED
DGELU_BOUND = 8 * DGELU_MEASURED
assert CE_LOSS_BOUND <= 8.0                      # (the CE bound may be rounded up to 8 units and no further)


# ---------------------------------------------------------------------------------------------- float64 restatements
def lse_f64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def ce_f64(x, label):
    """F.cross_entropy(x, label, reduction='none'), negative labels ignored -> (loss [R], lse [R], d loss_r / d x_r [R, C])"""
    x = np.asarray(x, dtype=np.float64)
    R, C = x.shape
    lse = lse_f64(x)
    lab = np.clip(label, 0, C - 1)
    rows = np.arange(R)
    with np.errstate(invalid="ignore"):
        loss = np.where(label < 0, 0.0, lse - x[rows, lab])
    term = np.exp(x - lse[:, None])
    term[rows, lab] -= 1.0
    term[label < 0] = 0.0
    return loss, lse, term


def kl_f64(x, t):
    """F.kl_div(log_softmax(x), t, reduction='none').sum(1) with 0 log 0 = 0 -> (loss, lse, softmax(x) sum(t) - t)"""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    lse = lse_f64(x)
    tl = np.where(t > 0, t * np.log(np.where(t > 0, t, 1.0)), 0.0)
    loss = (tl - t * (x - lse[:, None])).sum(axis=1)
    return loss, lse, np.exp(x - lse[:, None]) * t.sum(axis=1, keepdims=True) - t


def row_unit(x, lse):
    """the unit of the CE / KL bounds, per row: eps32 max(1, |lse|, max finite |x|)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    a = np.where(np.isfinite(a), a, 0.0)
    amax = a.max(axis=1) if a.shape[1] else np.zeros(a.shape[0])
    l = np.where(np.isfinite(lse), np.abs(lse), 0.0)
    return EPS32 * np.maximum(1.0, np.maximum(l, amax))


def mse_f64(x, t):
    d = np.asarray(x, dtype=np.float64) - np.asarray(t, dtype=np.float64)
    return d * d


def erf_f64(a):
    a = np.asarray(a, dtype=np.float64)
    u, inv = np.unique(a, return_inverse=True)
    return np.array([math.erf(v) for v in u], dtype=np.float64)[inv].reshape(a.shape)


def dgelu_f64(x):
    """d/dx [x Phi(x)] = Phi(x) + x phi(x)"""
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * (1.0 + erf_f64(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def dgelu_tanh_f64(x):
    """the derivative of the tanh approximation (the mistake: not what the reference's erf-GELU has)"""
    x = np.asarray(x, dtype=np.float64)
    k = math.sqrt(2.0 / math.pi)
    u = k * (x + 0.044715 * x ** 3)
    th = np.tanh(u)
    return 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * k * (1.0 + 3 * 0.044715 * x * x)


def drelu(h, g):
    """g where h > 0, else +0 (h = +-0.0 included)"""
    return np.where(np.asarray(h) > 0, g, np.zeros_like(g))


def colsum_f64(x, out0=None, accumulate=False):
    s = np.asarray(x, dtype=np.float64).sum(axis=0)
    return s + np.asarray(out0, dtype=np.float64) if (accumulate and out0 is not None) else s


def smallk_wgrad_f64(dy, x, dw0=None, accumulate=False):
    """dW[n][k] = sum_m dy[m][n] x[m][k]"""
    w = np.asarray(dy, dtype=np.float64).T @ np.asarray(x, dtype=np.float64)
    return w + np.asarray(dw0, dtype=np.float64) if (accumulate and dw0 is not None) else w


def chunk_chain(M):
    """the longest chain of additions behind one output of hamt_colsum / hamt_smallk_wgrad: ceil(rows per chunk / 4) + 2 in the partial
    kernel (four row phases, then their sum), ceil(chunks / 4) + 2 in the reduction of the chunks"""
    chunks = 64 if M >= 64 * 64 else max(1, (M + 63) // 64)
    rpc = max(1, -(-M // chunks))
    return -(-rpc // 4) + 2 + -(-chunks // 4) + 2


def colsum_bound(x, out0=None):
    """per column: eps32 (longest chain) sum|x| (+ |out| when the sum is added to it)"""
    a = np.abs(np.asarray(x, dtype=np.float64)).sum(axis=0)
    if out0 is not None:
        a = a + np.abs(np.asarray(out0, dtype=np.float64))
    return EPS32 * chunk_chain(np.shape(x)[0]) * a


def smallk_bound(dy, x, dw0=None):
    a = np.abs(np.asarray(dy, dtype=np.float64)).T @ np.abs(np.asarray(x, dtype=np.float64))
    if dw0 is not None:
        a = a + np.abs(np.asarray(dw0, dtype=np.float64))
    return EPS32 * chunk_chain(np.shape(dy)[0]) * a


# ---------------------------------------------------------------------------------------------- bf16
def bf16_bits(x):
    """fp32 -> bf16 bits (uint16), round to nearest even; a NaN stays a (quiet) NaN"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = np.isnan(np.asarray(x, dtype=F32))
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


# ---------------------------------------------------------------------------------------------- fp32, the kernels' order of operations
def exp32(a):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(a, dtype=F32).astype(np.float64)).astype(F32)


def log32(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(a, dtype=F32).astype(np.float64)).astype(F32)


def block_sum32(v, drop_tail=False, drop_wave=None):
    """loss.hip's row sum of v [R, C]: thread t of 256 adds columns t, t + 256, ... in order, every wave of 64 lanes runs the xor
    butterfly (offsets 32 ... 1), lane 0 of the four waves gives r0 ... r3, the sum is (r0 + r1) + (r2 + r3).
    The mistakes: drop_tail = the columns c >= 256 floor(C / 256) are left out, drop_wave = one wave's partial sum is."""
    v = np.asarray(v, dtype=F32)
    R, C = v.shape
    if drop_tail:
        C = 256 * (C // 256)
    n = -(-C // 256)
    pad = np.zeros((R, max(n, 1) * 256), dtype=F32)
    pad[:, :C] = v[:, :C]
    pad = pad.reshape(R, max(n, 1), 256)
    s = np.zeros((R, 256), dtype=F32)
    for j in range(n):
        s = s + pad[:, j]
    lane = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    r = s[:, ::64].copy()
    if drop_wave is not None:
        r[:, drop_wave] = 0
    assert s.dtype == F32
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def row_lse32(x, sub_max=True, **mut):
    """row_lse: m + logf(sum expf(x - m)).  The mistake sub_max=False: no maximum subtracted"""
    x = np.asarray(x, dtype=F32)
    m = x.max(axis=1) if sub_max else np.zeros(x.shape[0], dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return m + log32(block_sum32(exp32(x - m[:, None]), **mut))


def ce32(x, label, g, label_shift=0, ignore=True, **mut):
    """ce_fwd_kernel / ce_bwd_kernel -> (loss, dx); label_shift / ignore=False are the mistakes 'label off by one' and 'an ignored row
    given the ordinary gradient'"""
    x, g = np.asarray(x, dtype=F32), np.asarray(g, dtype=F32)
    R, C = x.shape
    rows = np.arange(R)
    l = row_lse32(x, **mut)
    lab = np.clip(label + label_shift, 0, C - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        loss = np.where(label < 0, F32(0), l - x[rows, lab])
        onehot = np.zeros((R, C), dtype=F32)
        onehot[rows, lab] = 1
        dx = g[:, None] * (exp32(x - l[:, None]) - onehot)
    if ignore:
        dx[label < 0] = 0
    assert loss.dtype == F32 and dx.dtype == F32
    return loss, dx


def kl32(x, t, g, with_tsum=True, nan_at_zero=False):
    """kl_fwd_kernel / kl_bwd_kernel -> (loss, dx).  The mistakes: with_tsum=False = the gradient without the sum(t) factor,
    nan_at_zero = t log t at t = 0 taken as it comes (0 * -inf)"""
    x, t, g = np.asarray(x, dtype=F32), np.asarray(t, dtype=F32), np.asarray(g, dtype=F32)
    l = row_lse32(x)
    with np.errstate(invalid="ignore"):
        tl = t * log32(t)
        if not nan_at_zero:
            tl = np.where(t > 0, tl, F32(0))
        loss = block_sum32(tl - t * (x - l[:, None]))
        ts = block_sum32(t) if with_tsum else np.ones(x.shape[0], dtype=F32)
        dx = g[:, None] * (exp32(x - l[:, None]) * ts[:, None] - t)
    assert loss.dtype == F32 and dx.dtype == F32
    return loss, dx


def mse32(x, t):
    d = np.asarray(x, dtype=F32) - np.asarray(t, dtype=F32)
    return d * d


def mse_bwd32(x, t, g):
    return (F32(2) * np.asarray(g, dtype=F32)) * (np.asarray(x, dtype=F32) - np.asarray(t, dtype=F32))


def dgelu32(x):
    """common.h's dgelu_erf: 0.5 (1 + erff(x / sqrt 2)) + x (1 / sqrt(2 pi)) expf(-0.5 x x), every operation rounded to fp32"""
    x = np.asarray(x, dtype=F32)
    c1, c2 = F32(0.70710678118654752440), F32(0.39894228040143267794)
    erf = erf_f64((x * c1).astype(np.float64)).astype(F32)
    out = F32(0.5) * (F32(1) + erf) + x * c2 * exp32(F32(-0.5) * x * x)
    assert out.dtype == F32
    return out


def inv_keep32(p):
    """the kernels' 1.0f / (1.0f - p)"""
    return F32(1) / (F32(1) - F32(p))


def mean_mid_bwd32(dy, S):
    return np.asarray(dy, dtype=F32) * (F32(1) / F32(S))


def extend_mask32(m):
    """(1 - (m ? 1 : 0)) * -10000: -10000 where m == 0, and MINUS zero elsewhere"""
    return (F32(1) - (np.asarray(m) != 0).astype(F32)) * F32(-10000)


def add3_32(a, b, c=None):
    s = np.asarray(a, dtype=F32) + np.asarray(b, dtype=F32)
    return s + np.asarray(c, dtype=F32) if c is not None else s


# ---------------------------------------------------------------------------------------------- the counter-based RNG (common.h)
_M = 0xFFFFFFFF
_M64 = np.uint64(_M)


def mix32_int(x):
    x &= _M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M
    x ^= x >> 16
    return x


def mix32(x):
    """hamt_mix32 on an array of 32-bit values (held in uint64 so that the products do not overflow)"""
    x = np.asarray(x, dtype=np.uint64) & _M64
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M64
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M64
    return x ^ (x >> np.uint64(16))


def rng_key(seed, epoch, call_id):
    """(k0, k1) of rng_key: seed / epoch are the two 64-bit words of the device RNG state, call_id the 32-bit call counter"""
    k0 = mix32_int((seed & _M) ^ mix32_int((epoch & _M) + 0x9E3779B9) ^ ((call_id * 0x85EBCA6B) & _M))
    k1 = mix32_int(((seed >> 32) & _M) ^ ((epoch >> 32) & _M) ^ ((call_id + 0xC2B2AE35) & _M))
    return k0, k1


def drop_keep(key, n, p, u_gt_p=False):
    """keep mask of drop_scale for the element indices 0 .. n - 1: u = (x >> 8) 2^-24 >= p, i.e. x >> 8 >= ceil(p 2^24) with the fp32 p.
    (u_gt_p: the mistake 'u > p')"""
    k0, k1 = key
    idx = np.arange(n, dtype=np.uint64)
    x = mix32((idx & _M64) ^ np.uint64(k0))
    x = mix32((x + (idx >> np.uint64(32)) * np.uint64(0x9E3779B9) + np.uint64(k1)) & _M64)
    p24 = float(F32(p)) * 16777216.0                      # exact: a power of two times an fp32 value
    u = (x >> np.uint64(8)).astype(np.int64)
    return u > p24 if u_gt_p else u >= math.ceil(p24)


def drop_scale(key, n, p):
    """the factors hamt_dropout multiplies by: 1 / (1 - p) in fp32 where kept, 0 where dropped"""
    return np.where(drop_keep(key, n, p), inv_keep32(p), F32(0)).astype(F32)


def drop_keep4(key, R, C, p):
    """keep mask [R, C] of drop_scale4 as hamt_cast_pad_bf16_dropout uses it: rowh = mix32(row ^ k0), one two-round hash per group of
    four columns gives four 16-bit uniforms (x low, x high, y low, y high), keep iff u16 >= floor(p 65536)"""
    k0, k1 = key
    rowh = mix32(np.arange(R, dtype=np.uint64) ^ np.uint64(k0))
    grp = np.arange((C + 3) // 4, dtype=np.uint64)
    x = mix32((rowh[:, None] + grp[None, :] * np.uint64(0x9E3779B9) + np.uint64(k1)) & _M64)
    y = mix32(x ^ np.uint64(0x85EBCA6B))
    u = np.stack([x & np.uint64(0xFFFF), x >> np.uint64(16), y & np.uint64(0xFFFF), y >> np.uint64(16)], axis=2).reshape(R, -1)[:, :C]
    return u.astype(np.int64) >= drop_thr16(p)


def drop_thr16(p):
    return int(F32(p) * F32(65536))


def drop_scale4(key, R, C, p):
    return np.where(drop_keep4(key, R, C, p), inv_keep32(p), F32(0)).astype(F32)


def keep_rate(p):
    """exact keep probability of drop_scale for a uniform 24-bit draw"""
    return 1.0 - math.ceil(float(F32(p)) * 16777216.0) / 16777216.0


def keep_rate4(p):
    return 1.0 - drop_thr16(p) / 65536.0


# ---------------------------------------------------------------------------------------------- cases
SEED, CALL_ID = 1234, 186                # ops.manual_seed(SEED); ops._call_counter[0] = CALL_ID - 1 in front of the call under test
TIE_INDEX = 114282                       # with (SEED, epoch 0, CALL_ID) this element draws u = 0.5 exactly: kept by `u >= p` at p = 0.5, dropped by `u > p`
G_CYCLE = (1.0, 0.0, -1.5, 1e-3, 1e3, 0.37, -2.0)      # upstream weights: 0, a negative value, 1e-3 next to 1e3
PAD_VALUE = 7.0                          # what the padding columns of a strided buffer hold (finite: a row read at r C shows)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _ce_case(name, C, ld, layout, rows, seed):
    """rows: (kind, label) per row.  kind: s3 / s12 / s30 = N(0, 1) times the scale, o1e4 = 3 N + 1e4, s60 = 60 N - 300, half = 3 N with
    half of the columns -inf, one = a single finite logit.  label: an int (negative: ignored; -2 stands for C - 1), 'rand', 'fin' = a
    finite column (the finite one of `one`), 'ninf' = a -inf column."""
    rng = _rng(seed)
    R = len(rows)
    buf = np.full((R, ld), PAD_VALUE, dtype=F32)
    label = np.zeros(R, dtype=np.int64)
    for r, (kind, lab) in enumerate(rows):
        z = rng.standard_normal(C)
        x = {"s3": 3 * z, "s12": 12 * z, "s30": 30 * z, "o1e4": 3 * z + 1e4, "s60": 60 * z - 300, "half": 3 * z, "one": 3 * z}[kind]
        if kind == "half":
            x[rng.permutation(C)[:C // 2]] = -np.inf
        if kind == "one":
            keep = int(rng.integers(C))
            x[np.arange(C) != keep] = -np.inf
        fin = np.flatnonzero(np.isfinite(x))
        if lab == "rand":
            lab = int(rng.integers(C))
        elif lab == "fin":
            lab = int(fin[rng.integers(len(fin))])
        elif lab == "ninf":
            lab = int(np.flatnonzero(np.isinf(x))[0])
        elif lab == -2:
            lab = C - 1
        buf[r, :C] = x
        label[r] = lab
    g = np.array([G_CYCLE[(r + seed) % len(G_CYCLE)] for r in range(R)], dtype=F32)
    return dict(name=name, R=R, C=C, ld=ld, layout=layout, buf=buf, x=buf[:, :C], label=label, g=g, kinds=[k for k, _ in rows],
                labs=[l for _, l in rows])


@functools.lru_cache(maxsize=None)
def ce_cases():
    """Every cross-entropy case.  layout: 'view' = [:, :C] of a [R, ld] buffer, 'empty_rows' = allocated by ops.empty_rows (ld = C padded
    to 4 floats), 'colstride' = the transpose of a [C, R] tensor (column stride R: the .contiguous() branch).  The arrays are shared."""
    plain = [("s3", "rand"), ("s30", -2), ("o1e4", 0), ("s60", "rand")]
    every = [("s3", "rand"), ("s30", "rand"), ("o1e4", "rand"), ("s60", "rand"), ("one", "fin"), ("half", "ninf"), ("half", "fin"),
             ("s3", -100), ("s30", -1), ("s3", 0), ("s30", -2), ("o1e4", -100), ("half", "fin"), ("s60", 0), ("one", "fin"), ("s3", "rand"),
             ("half", "ninf"), ("s30", "rand"), ("s60", -2)]
    cases = [
        _ce_case("5x1", 1, 1, "view", [("s3", 0), ("s30", -100), ("o1e4", 0), ("s60", -1), ("s3", -2)], 1),
        _ce_case("7x37 in 40", 37, 40, "view", [("half", "fin"), ("s3", "rand"), ("half", "ninf"), ("one", "fin"), ("half", "fin"), ("s30", -100),
                                               ("half", "fin")], 2),
        _ce_case("4x255", 255, 255, "view", plain, 3),
        _ce_case("4x256", 256, 256, "view", plain, 4),
        _ce_case("4x257", 257, 257, "view", plain, 5),
        _ce_case("19x1003 in 1008", 1003, 1008, "view", every, 6),
        _ce_case("6x30522 empty_rows", 30522, 30524, "empty_rows", [("s3", "rand"), ("s12", "rand"), ("o1e4", -2), ("s30", 0), ("one", "fin"), ("s60", "rand")], 7),
        _ce_case("6x130 column stride", 130, 130, "colstride", [("s3", "rand"), ("s30", "rand"), ("half", "ninf"), ("s3", -100), ("o1e4", "rand"), ("s60", 0)], 8),
    ]
    assert len(every) == 19
    return cases


def _kl_case(name, R, C, scale, seed, t64=False):
    """target rows cycle: a softmax, a softmax with a third of its entries zero, a one-hot, an all-zero row, a row summing to 0.5"""
    rng = _rng(seed)
    x = (scale * rng.standard_normal((R, C))).astype(F32)
    t = np.zeros((R, C), dtype=np.float64)
    kinds = []
    for r in range(R):
        kind = ("softmax", "third_zero", "onehot", "zero", "half_mass")[(r + seed) % 5]
        z = 2 * rng.standard_normal(C)
        sm = np.exp(z - z.max())
        sm /= sm.sum()
        if kind == "third_zero":
            sm[rng.permutation(C)[:C // 3]] = 0.0
        elif kind == "onehot":
            sm[:] = 0.0
            sm[rng.integers(C)] = 1.0
        elif kind == "zero":
            sm[:] = 0.0
        elif kind == "half_mass":
            sm *= 0.5
        t[r] = sm
        kinds.append(kind)
    if not t64:
        t = t.astype(F32)
    g = np.array([G_CYCLE[(r + seed + 2) % len(G_CYCLE)] for r in range(R)], dtype=F32)
    return dict(name=name, R=R, C=C, x=x, t=t, t32=t.astype(F32), g=g, kinds=kinds)


@functools.lru_cache(maxsize=None)
def kl_cases():
    """(R, C) = (3, 1), (11, 40), (4, 257), (5, 1000) at logit scales 2 and 30; the 1000-wide cases take all five target kinds, one of
    them with a float64 target (the Function's .to(float32))"""
    out = []
    for i, (R, C) in enumerate([(3, 1), (11, 40), (4, 257), (5, 1000)]):
        for j, scale in enumerate((2.0, 30.0)):
            out.append(_kl_case(f"{R}x{C} scale {scale:g}", R, C, scale, 10 + 2 * i + j, t64=(C == 1000 and j == 1)))
    return out


MSE_SIZES = (1, 3, 255, 257, 2048 * 256 + 5)


def mse_case(n, seed=20):
    rng = _rng(seed + n % 97)
    x, t, g = (rng.standard_normal(n).astype(F32) for _ in range(3))
    g[::7] = 0
    return x, t, g


COLSUM_M = (1, 63, 64, 65, 4095, 4096, 4097)
COLSUM_N = (1, 40, 130, 768)


def colsum_case(M, N, dtype="f32", seed=30):
    """x [M, ld] with the N columns under test at column offset 3 of a wider buffer (ld = N + 5), the start `out` holds for accumulate;
    dtype 'bf16': the values are bf16-representable and `bits` holds their 16-bit patterns"""
    rng = _rng(seed + 7 * M + N)
    buf = rng.standard_normal((M, N + 5)).astype(F32)
    bits = None
    if dtype == "bf16":
        bits = bf16_bits(buf)
        buf = bf16_value(bits)
    out0 = (np.sign(rng.standard_normal(N)) * (5 + np.abs(rng.standard_normal(N)))).astype(F32)
    return dict(M=M, N=N, off=3, buf=buf, bits=bits, x=buf[:, 3:3 + N], out0=out0)


def fp16_value(bits):
    """the mistake: bf16 bit patterns read as IEEE half"""
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)


SMALLK_K, SMALLK_N, SMALLK_M = (1, 4, 8), (1, 64, 65, 768), (1, 65, 4097)


def smallk_case(M, N, K, seed=40):
    """dy = columns 2 .. 2 + N of a [M, N + 3] buffer, x = columns 1 .. 1 + K of a [M, K + 4] buffer (ldx > K), dw0 for accumulate"""
    rng = _rng(seed + 11 * M + 3 * N + K)
    dyb = rng.standard_normal((M, N + 3)).astype(F32)
    xb = rng.standard_normal((M, K + 4)).astype(F32)
    dw0 = (3 + rng.standard_normal((N, K))).astype(F32)
    return dict(M=M, N=N, K=K, dyb=dyb, xb=xb, dy=dyb[:, 2:2 + N], x=xb[:, 1:1 + K], dw0=dw0)


ACT_SPECIALS = (0.0, -0.0, 1e-20, -1e-20, 0.5, -0.5, 3.0, -3.0, 10.0, -10.0, 40.0, -40.0)
ACT_SIZES = (4, 1024, 4 * (2048 * 256) + 4)


@functools.lru_cache(maxsize=None)
def act_block(seed=50):
    """1024 pre-activations (the specials first, then N(0, 2)) and upstream gradients; larger cases tile it"""
    rng = _rng(seed)
    h = (2 * rng.standard_normal(1024)).astype(F32)
    h[:len(ACT_SPECIALS)] = ACT_SPECIALS
    g = rng.standard_normal(1024).astype(F32)
    g[np.abs(g) < 1e-3] = 1.0
    return h, g


def act_case(n):
    """(h, g) of n elements: n = 4 takes +-0.0 and +-1e-20 ... the first four specials"""
    h, g = act_block()
    reps = -(-n // 1024)
    return np.tile(h, reps)[:n].copy(), np.tile(g, reps)[:n].copy()


def cast_case(n, seed=60):
    """fp32 values whose bf16 rounding is decided by a tie (to even, both ways), +-inf, +-0, subnormals, NaN, then N(0, 1)"""
    rng = _rng(seed + n)
    x = rng.standard_normal(n).astype(F32)
    special = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001,
                        0x807FFFFF, 0x00018000, 0x7FC00000, 0x7F7FFFFF, 0xFFC00001, 0x3F7FFFFF, 0x00008000, 0x00028000], dtype=np.uint32).view(F32)
    k = min(n, len(special))
    x[:k] = special[:k]
    return x


# ---------------------------------------------------------------------------------------------- errors in the units of the bounds
def _worst(d):
    d = np.asarray(d, dtype=np.float64)
    if d.size == 0:
        return 0.0
    return float(np.where(np.isnan(d), np.inf, d).max())


def ce_errors(c, loss, dx):
    """per row: the loss error and the worst error of dx / g against the float64 restatement, in row units.  What has to hold exactly
    (an infinite loss, an ignored row, a single finite logit that is the label, a zero upstream weight, -g at a label on a -inf column)
    counts as an infinite error where it does not."""
    loss, dx = np.asarray(loss, dtype=np.float64), np.asarray(dx, dtype=np.float64)
    want, lse, term = ce_f64(c["x"], c["label"])
    unit = row_unit(c["x"], lse)
    g = c["g"].astype(np.float64)
    el, et = np.zeros(c["R"]), np.zeros(c["R"])
    for r in range(c["R"]):
        lab = int(c["label"][r])
        zero = lab < 0 or (c["kinds"][r] == "one" and c["labs"][r] == "fin")
        if zero:
            el[r] = 0.0 if loss[r] == 0 else np.inf
        elif np.isinf(want[r]):
            el[r] = 0.0 if loss[r] == np.inf else np.inf
        else:
            el[r] = _worst(abs(loss[r] - want[r]) / unit[r])
        if zero or g[r] == 0:
            et[r] = 0.0 if (dx[r] == 0).all() else np.inf
        else:
            et[r] = _worst(np.abs(dx[r] - g[r] * term[r]) / (abs(g[r]) * unit[r]))
            if c["labs"][r] == "ninf" and dx[r, lab] != -g[r]:
                et[r] = np.inf
    return el, et


def kl_errors(c, loss, dx):
    """as ce_errors; an all-zero target row has loss 0 and gradient 0 exactly"""
    loss, dx = np.asarray(loss, dtype=np.float64), np.asarray(dx, dtype=np.float64)
    want, lse, term = kl_f64(c["x"], c["t32"])
    unit = row_unit(c["x"], lse)
    g = c["g"].astype(np.float64)
    el, et = np.zeros(c["R"]), np.zeros(c["R"])
    for r in range(c["R"]):
        zero = c["kinds"][r] == "zero"
        el[r] = (0.0 if loss[r] == 0 else np.inf) if zero else _worst(abs(loss[r] - want[r]) / unit[r])
        if zero or g[r] == 0:
            et[r] = 0.0 if (dx[r] == 0).all() else np.inf
        else:
            et[r] = _worst(np.abs(dx[r] - g[r] * term[r]) / (abs(g[r]) * unit[r]))
    return el, et


def dgelu_errors(h, g, dx, ref=dgelu_f64):
    """|dx - g gelu'(h)| in units of eps32 |g|"""
    g = np.asarray(g, dtype=np.float64)
    return np.abs(np.asarray(dx, dtype=np.float64) - g * ref(h)) / (EPS32 * np.abs(g))
