"""Cases, float64 reference and numpy-fp32 restatement of `hamt_attn_cls_fwd` (csrc/attn_cls.hip) for test_attn_cls_ref.py (CPU) and
test_gpu_extract.py (GPU).

Error unit: |o - o64| / max|v of that image| / 2^-24, per output row (image).  The restatement follows the kernel's order of
operations (8 columns per lane left to right, xor butterflies 1-2-4 for a score, 32..1 for the softmax sum, 8-16-32 for P V) with a
rounded product plus a rounded add where the kernel has one fused multiply-add, so its error is an upper estimate of the kernel's.
`MEASURED` caps the restatement's worst error over `cases()`; the GPU bound is 8 x that (the convention of _smallops_ref.py)."""
import numpy as np

F32 = np.float32
UNIT = 2.0 ** -24
N_IMG, HEADS, DH = 3, 2, 64
H = HEADS * DH
SCALE = DH ** -0.5
SKS = (1, 5, 63, 64, 65, 197, 256)
MEASURED = 1.0           # cap on the worst restatement error in units (test_attn_cls_ref.py prints the figure: 0.975, Sk5 bf16)
BOUND = 8 * MEASURED     # what the GPU kernel must meet
MISTAKES = ("no_scale", "no_max", "drop_last", "swap_heads")


def to_bf16(a):
    """round-to-nearest-even to bf16, returned as the float32 values"""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(F32)


def cases():
    """[{name, Sk, dtype, q [n, H], k / v [n * Sk, H] (float32 holding values of `dtype`), pad_q / pad_kv: extra row stride in elements}]"""
    out = []
    for it, Sk in enumerate(SKS):
        for dt in ("fp32", "bf16"):
            g = np.random.Generator(np.random.PCG64([77, Sk, int(dt == "bf16")]))
            q, k, v = (g.standard_normal(s, dtype=F32) for s in ((N_IMG, H), (N_IMG * Sk, H), (N_IMG * Sk, H)))
            v *= F32(1.0 + it)                                                  # (the scaling by max|v| has to be real)
            out.append(dict(name=f"Sk{Sk} {dt}", Sk=Sk, dtype=dt, q=q, k=k, v=v, pad_q=8 * (it % 3), pad_kv=16 * (it % 2)))
    # one score at +90 and one at -90 in the same row (image 0, head 0): 64 * 3.0 * 3.75 / 8 = 90; every value is exact in bf16
    for dt in ("fp32", "bf16"):
        g = np.random.Generator(np.random.PCG64([78, int(dt == "bf16")]))
        Sk = 65
        q, k, v = (g.standard_normal(s, dtype=F32) for s in ((N_IMG, H), (N_IMG * Sk, H), (N_IMG * Sk, H)))
        q[0, :DH] = 3.0
        k[3, :DH], k[64, :DH] = 3.75, -3.75
        out.append(dict(name=f"Sk65 +-90 {dt}", Sk=Sk, dtype=dt, q=q, k=k, v=v, pad_q=8, pad_kv=0))
    # all keys of an image equal: the softmax is uniform, o = mean(v)
    g = np.random.Generator(np.random.PCG64(79))
    Sk = 63
    q, v = g.standard_normal((N_IMG, H), dtype=F32), g.standard_normal((N_IMG * Sk, H), dtype=F32)
    k = np.repeat(g.standard_normal((N_IMG, H), dtype=F32), Sk, axis=0)
    out.append(dict(name="Sk63 equal keys bf16", Sk=Sk, dtype="bf16", q=q, k=k, v=v, pad_q=0, pad_kv=16))
    for c in out:
        if c["dtype"] == "bf16":
            c["q"], c["k"], c["v"] = to_bf16(c["q"]), to_bf16(c["k"]), to_bf16(c["v"])
    return out


def attn_cls_f64(q, k, v, Sk):
    n = q.shape[0]
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    qh, kh, vh = q.reshape(n, HEADS, DH), k.reshape(n, Sk, HEADS, DH), v.reshape(n, Sk, HEADS, DH)
    s = np.einsum("nhd,njhd->nhj", qh, kh) * SCALE
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("nhj,njhd->nhd", p, vh).reshape(n, H)


def _butterfly(a, axis, offsets):
    idx = np.arange(a.shape[axis])
    for o in offsets:
        a = a + np.take(a, idx ^ o, axis=axis)
    return a


def attn_cls32(q, k, v, Sk, mistake=None):
    """float32 throughout, the kernel's order; `mistake`: one of MISTAKES"""
    n = q.shape[0]
    q, k, v = (np.ascontiguousarray(a, dtype=F32) for a in (q, k, v))
    k5, v5 = k.reshape(n, Sk, HEADS, 8, 8), v.reshape(n, Sk, HEADS, 8, 8)            # (image, key, head, sub, column of the lane)
    if mistake == "drop_last":
        Sk, k5, v5 = Sk - 1, k5[:, :Sk - 1], v5[:, :Sk - 1]
    q4 = q.reshape(n, HEADS, 8, 8)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        acc = np.zeros((n, Sk, HEADS, 8), F32)
        for i in range(8):
            acc = acc + q4[:, None, :, :, i] * k5[..., i]
        s = _butterfly(acc, 3, (1, 2, 4))[..., 0]                                       # (n, Sk, heads)
        if mistake != "no_scale":
            s = s * F32(SCALE)
        m = s.max(axis=1, keepdims=True) if Sk else np.zeros((n, 1, HEADS), F32)
        p = np.exp(s if mistake == "no_max" else s - m)
        assert p.dtype == F32
        lanes = np.zeros((n, 64, HEADS), F32)
        for t in range(0, Sk, 64):
            c = p[:, t:t + 64]
            lanes[:, :c.shape[1]] = lanes[:, :c.shape[1]] + c
        l = _butterfly(lanes, 1, (32, 16, 8, 4, 2, 1))[:, 0]                            # (n, heads)
        o = np.zeros((n, 8, HEADS, 8, 8), F32)                                          # (image, grp, head, sub, column)
        for j0 in range(0, Sk, 8):
            c = min(8, Sk - j0)
            o[:, :c] = o[:, :c] + p[:, j0:j0 + c, :, None, None] * v5[:, j0:j0 + c]
        o = _butterfly(o, 1, (1, 2, 4))[:, 0] / l[:, :, None, None]
    o = o.reshape(n, H)
    if mistake == "swap_heads":
        o = np.concatenate([o[:, DH:], o[:, :DH]], axis=1)
    return o


def errors(c, o):
    """per image, in units; a non-finite output counts as infinite"""
    want = attn_cls_f64(c["q"], c["k"], c["v"], c["Sk"])
    vmax = np.abs(c["v"]).reshape(N_IMG, -1).max(axis=1).astype(np.float64)
    e = np.abs(np.asarray(o, dtype=np.float64) - want).max(axis=1) / vmax / UNIT
    return np.where(np.isfinite(e), e, np.inf)
