"""numpy statement of hamt_range_audit's record (include/hamt.h), on RAW bit patterns, and the cases the GPU test runs.

A case is a list of calls on one record.  Every call's operand x [M, N] (row stride ld) sits at element `off` of a larger flat buffer whose
every other element -- in front, behind, and in the ld - N gap columns -- is poison: NaN, +-inf and at-the-limit patterns, so a kernel
that reads one element outside [M, N] gets a different record.  The record is pre-loaded with non-zero values, so adding is told from
overwriting.  `audit_record(..., fault=...)` restates the record WITH one deliberate error; tests/test_range_audit_ref.py shows that
each error changes the expected record of at least one case, i.e. that the cases can see it.
"""
import numpy as np

# format: (numpy type of the raw pattern, magnitude mask, first non-finite magnitude, at-the-limit magnitude or None, elements per 16 bytes)
FMT = {
    "f16": (np.uint16, 0x7FFF, 0x7C00, 0x7BFF, 8),
    "bf16": (np.uint16, 0x7FFF, 0x7F80, None, 8),
    "f32": (np.uint32, 0x7FFFFFFF, 0x7F800000, None, 4),
}
FAULTS = ("ignore_sign", "count_7bfe", "inf_at_limit", "nonfinite_in_max", "read_col_N", "read_row_M", "drop_tail", "replace_max",
          "zero_exp_nonfinite")

F32_ONE_AND_HALF = 0x3FC00000
REC0 = (3, 5, F32_ONE_AND_HALF, 7)                      # what every record holds before its first call


def f32_bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def bits_f32(b):
    return float(np.array([b], dtype=np.uint32).view(np.float32)[0])


def widen(fmt, a):
    """float32 bit pattern of the value a magnitude pattern `a` of `fmt` encodes (exact: every half / bf16 is a float32)"""
    if fmt == "f16":
        return int(np.array([a], dtype=np.uint16).view(np.float16).astype(np.float32).view(np.uint32)[0])
    return int(a) << 16 if fmt == "bf16" else int(a)


def encode(fmt, v):
    """raw patterns of the float32 array v rounded to `fmt` (finite, in range)"""
    v = np.asarray(v, dtype=np.float32)
    if fmt == "f16":
        return v.astype(np.float16).view(np.uint16)
    if fmt == "f32":
        return v.view(np.uint32).copy()
    b = v.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)      # round to nearest even


def specials(fmt):
    """(patterns planted from element 0 on, pattern planted on the LAST element of x): -limit, limit - 1 ulp, +inf, NaN, -0, a subnormal,
    -inf; the last element (the tail of the last row) holds +limit -- the operand's largest finite value and, in half, a count"""
    if fmt == "f16":
        return [0xFBFF, 0x7BFE, 0x7C00, 0x7E01, 0x8000, 0x0001, 0xFC00], 0x7BFF
    if fmt == "bf16":     # (bf16 has no 65504: 0x477F = 65280 and 0x4780 = 65536 straddle it; 0x7BFF is some large finite bf16)
        return [0xFBFF, 0x477F, 0x7F80, 0x7FC1, 0x8000, 0x0001, 0xFF80], 0x7C00
    return [f32_bits(-65504.0), 0x7BFE, 0x7F800000, 0x7FC00001, 0x80000000, 0x00000001, 0xFF800000], f32_bits(70000.0)


def poison(fmt, n, phase=0):
    dt = FMT[fmt][0]
    if fmt == "f16":
        p = [0x7E00, 0x7C00, 0x7BFF, 0xFC00, 0xFBFF]
    elif fmt == "bf16":
        p = [0x7FC0, 0x7F80, 0x7F7F, 0xFF80, 0xFF7F]
    else:
        p = [0x7FC00000, 0x7F800000, 0x7F7FFFFF, 0xFF800000, 0xFF7FFFFF]
    return np.resize(np.roll(np.array(p, dtype=dt), -(phase % 5)), n)


PAD = 64            # poison elements in front of x (x then starts 16-byte aligned in an aligned allocation) and at least as many behind


def make_call(fmt, M, N, ld=None, off=PAD, seed=0, plant=True, scale=100.0):
    """-> dict(fmt, M, N, ld, off, buf): `buf` the flat raw buffer, x[r, c] = buf[off + r * ld + c]"""
    ld = N if ld is None else ld
    dt = FMT[fmt][0]
    total = off + (M + 1) * ld + PAD
    buf = poison(fmt, total, phase=seed)
    rng = np.random.default_rng(1000 + seed)
    vals = encode(fmt, (rng.standard_normal((M, N)) * scale).astype(np.float32))
    if plant and M * N > 0:
        sp, last = specials(fmt)
        flat = vals.reshape(-1)
        for i, s in enumerate(sp[:max(0, flat.size - 1)]):
            flat[i] = s
        flat[-1] = last
    idx = off + np.arange(M)[:, None] * ld + np.arange(N)[None, :]
    buf[idx.reshape(-1)] = vals.reshape(-1).astype(dt)
    return dict(fmt=fmt, M=M, N=N, ld=ld, off=off, buf=buf)


def audit_record(call, rec, fault=None):
    """the record after one hamt_range_audit call on `call`, from the record `rec` before it (lists of 4 ints)"""
    fmt, M, N, ld, off, buf = (call[k] for k in ("fmt", "M", "N", "ld", "off", "buf"))
    _, mask, inf, limit, V = FMT[fmt]
    rows = M + 1 if (fault == "read_row_M" and M > 0) else M
    cols = N + 1 if (fault == "read_col_N" and ld > N) else N
    if fault == "drop_tail":
        cols = N // V * V
    idx = off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
    raw = buf[idx.reshape(-1)].astype(np.uint64)
    a = raw & mask
    finite = a < inf
    if fault == "zero_exp_nonfinite":
        finite &= (a & inf) != 0                # (an exponent field of zeros -- zeros, subnormals -- taken for one of ones)
    at_limit = 0
    if limit is not None:
        hit = (raw if fault == "ignore_sign" else a) == limit
        if fault == "count_7bfe":
            hit |= a == limit - 1
        if fault == "inf_at_limit":
            hit |= a == inf
        at_limit = int(hit.sum())
    in_max = a if fault == "nonfinite_in_max" else a[finite]
    # (a non-finite magnitude has no exact float32 widening in half / bf16 terms that matters here: its pattern, widened like the others)
    new_max = widen(fmt, int(in_max.max())) if in_max.size and int(in_max.max()) > 0 else 0
    return [rec[0] + at_limit, rec[1] + int((~finite).sum()), new_max if fault == "replace_max" else max(rec[2], new_max), rec[3] + 1]


def fold(calls, rec=REC0, fault=None):
    rec = list(rec)
    for c in calls:
        rec = audit_record(c, rec, fault)
    return rec


# The kernel takes units of work grid-stride over at most 1024 workgroups of 256 lanes (csrc/audit.hip: kMaxBlocks, kThreads), one
# 16-byte vector (or one ragged tail) per unit: a single pass covers 262 144 units.  (257, 776, ld 784) is 257 x 97 = 24 929 units in half
# -- one pass --, so the case that makes lanes come round a second time is sized from that cap: 1031 rows of 257 vectors (+ a 3-element
# tail in half / bf16) = 265 998 units; in fp32 the same shape is 1031 x 515 units.
GRID_LANES = 1024 * 256             # units one pass covers (tests/test_range_audit_ref.py checks the large case against it)
SHAPES = [
    # name, M, N, ld, off
    ("1x8", 1, 8, 8, PAD),
    ("3x7_ld9", 3, 7, 9, PAD),
    ("5x136_unaligned", 5, 136, 136, PAD + 1),
    ("64x128", 64, 128, 128, PAD),
    ("257x776_ld784", 257, 776, 784, PAD),
    ("0x8", 0, 8, 8, PAD),
    # beyond the issue's list: the ragged tail behind full vectors with aligned rows, and as the end of one long contiguous row
    ("9x77_ld80", 9, 77, 80, PAD),
    ("7x13", 7, 13, 13, PAD),
    ("1031x2059_ld2064", 1031, 2059, 2064, PAD),
]


def cases():
    """{name: [calls]}: every shape in every format (one call), and two calls on one record whose second operand is the smaller"""
    out = {}
    for fmt in FMT:
        for s, (name, M, N, ld, off) in enumerate(SHAPES):
            out[f"{fmt}/{name}"] = [make_call(fmt, M, N, ld, off, seed=s)]
        out[f"{fmt}/two_calls"] = [make_call(fmt, 5, 24, 32, PAD, seed=20), make_call(fmt, 4, 40, 40, PAD, seed=21, plant=False, scale=3.0)]
    return out
