"""Plain numpy restatements of the attention kernels (csrc/attn.hip: the fp32 MFMA path, csrc/attn16.hip: the bf16 path with its
single-pass, wide and tiled kernels, and the packed forms that ride on the single-pass kernels), dropout on the probabilities included,
with the cases and bounds of their op-level tests.  test_attn_ref.py proves on the CPU that the cases tell a wrong kernel from a right
one, test_gpu_attn.py runs the kernels on them.

  attn64    float64, from the values the kernel is given:  S = Q K^T scale + mask, lse = logsumexp(S), P = exp(S - lse), P~ = P f,
            O = P~ V, delta = rowsum(dO * O), dV = P~^T dO, dP = dO V^T, dS = P (dP f - delta) scale, dQ = dS K, dK = dS^T Q
  restate   the same at the kernels' precision with the roundings where the kernels place them (`attn32` / `attn16` by the case's
            path), with a switch for every mistake test_attn_ref.py lists
  f         1 / (1 - p) or 0 from the host twins of the device RNG (_smallops_ref): the fp32 path draws drop_scale at the linear index
            ((b heads + h) Sq + q) Sk + k, the bf16 path drop_scale4 with row (b heads + h) Sq + q and key group k >> 2; Sq, Sk are the
            DESCRIPTOR's (the maxima of a packed batch) and b is the query sequence's index

A case is a list of query sequences (rows cuq[b] .. cuq[b + 1] of q / do) each paired with one key side (rows cuk[j] .. cuk[j + 1] of
k / v, row j of the mask) or with none (a filler: zero out, zero dq, lse 0) -- the padded batch is the special case of equal lengths and
pair[b] = b.  Samples cycle through KINDS (`_key_side`, `_query_side`), so the sample index tests batch addressing; the two heads hold
different data.  A sample that is left with one live key is called `lastonly` whatever the cycle says.
On the bf16 path the `peaked` rows hold q and k that are bf16 values already (whatever the buffer's dtype): scores of a few tens times
the 2^-9 of an operand rounding would move P by tens of percent and the caps of those rows would say nothing.
Nothing here touches torch, the GPU or the package under test."""
import functools

import numpy as np

from _smallops_ref import CALL_ID, F32, SEED, bf16_bits, bf16_value, drop_scale, drop_scale4, keep_rate, keep_rate4, rng_key  # noqa: F401

HEADS, DH = 2, 64
H = HEADS * DH
SCALE = 0.125                            # 1 / sqrt(64): a power of two, so `s * scale + mask` and fma(s, scale, mask) round alike
MASKED = -10000.0
KINDS = ("randn", "peaked", "ramp", "headmask", "allmask", "lastonly", "nomask")
NOMASK_KINDS = ("nomask", "peaked")      # what the samples of a case without a mask (null pointer, packed keys) cycle through
OUTPUTS = ("out", "lse", "dq", "dk", "dv")
LOG2E, LN2 = F32(1.4426950408889634), F32(0.6931471805599453)


def _bf(x):
    return bf16_value(bf16_bits(x))


def fexp(x):
    """__expf: the hardware exp2 of the fp32 product x log2(e) (the product's rounding is the argument rounding of the fast exp)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp2((np.asarray(x, dtype=F32) * LOG2E).astype(np.float64)).astype(F32)


def flog(x):
    """__logf: the hardware log2 times ln 2"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log2(np.asarray(x, dtype=F32).astype(np.float64)).astype(F32) * LN2


def exp32(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, dtype=F32).astype(np.float64)).astype(F32)


def log32(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(x, dtype=F32).astype(np.float64)).astype(F32)


# ---------------------------------------------------------------------------------------------- which kernel a case reaches
def fwd_kernel(c):
    """hamt_attn_small_fwd / hamt_attn16_fwd_launch: the fp32 path has one forward; the bf16 path takes the single-pass kernel for every
    packed form and for Sk <= 256, the tiled one beyond"""
    if c["path"] == "fp32":
        return "attn_fwd_kernel"
    return "attn_s128_fwd_kernel" if (c["form"] != "pad" or c["Sk"] <= 256) else "attn16_fwd_kernel"


def fwd_kb(c):
    """launch_s128_fwd's KB: the staged 16-key blocks, even, at least 2"""
    nkb = (c["Sk"] + 15) // 16
    return 2 if nkb <= 2 else (nkb + 1) & ~1


def bwd_kernel(c):
    """hamt_attn16_bwd_launch: packed or both sides <= 128 -> s128, both <= 224 -> wide, else tiled"""
    if c["path"] == "fp32":
        return "attn_bwd_kernel"
    if c["form"] != "pad" or (c["Sq"] <= 128 and c["Sk"] <= 128):
        return "attn_s128_bwd_kernel"
    return "attn_wide_bwd_kernel" if (c["Sq"] <= 224 and c["Sk"] <= 224) else "attn16_bwd_kernel"


def bwd_nb(c):
    """launch_s128_bwd's NB"""
    nb = max((c["Sq"] + 15) // 16, (c["Sk"] + 15) // 16)
    return 2 if nb <= 2 else (4 if nb <= 4 else (6 if nb <= 6 else 8))


def kernel_of(c, output):
    return fwd_kernel(c) if output in ("out", "lse") else bwd_kernel(c)


def path_key(c):
    """the key of the cap tables: the path, and on the bf16 path whether the outputs are rounded to bf16 as well"""
    return c["path"] + ("/bf16" if c["io"] == "bf16" else "")


# ---------------------------------------------------------------------------------------------- cases
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _key_side(kind, nk, rng):
    """k, v [nk, H] and the additive mask row [nk] of a sample of this kind: randn a random -10000 mask that keeps at least one key,
    ramp +8 ... +11.75 on the last 16 keys (scores of sd 0.5: every row's maximum lies there, in the last key tile), headmask the first
    64 keys masked (all but the last where there are no more), allmask every key, lastonly all but the last, nomask / peaked zeros"""
    k, v = rng.standard_normal((nk, H)), rng.standard_normal((nk, H))
    m = np.zeros(nk)
    if kind == "randn":
        m[rng.random(nk) < 0.3] = MASKED
        m[rng.integers(nk)] = 0.0
    elif kind == "ramp":
        n = min(16, nk)
        m[nk - n:] = 8.0 + 0.25 * np.arange(n)
    elif kind == "headmask":
        m[:64 if nk > 64 else nk - 1] = MASKED
    elif kind == "allmask":
        m[:] = MASKED
    elif kind == "lastonly":
        m[:nk - 1] = MASKED
    return k, v, m


def _query_side(kind, nq, k, v, lone, rng, snap):
    """q, do [nq, H] against the key side `k`, `v` (None: a filler's queries).  Where one key carries a row (peaked, lastonly) dO leans
    toward that key's V: delta = dO . O is the scale the cancellation dP f - delta is measured in (see `errors`), and a delta that is
    small by accident would make the unit of dq / dk say nothing about the roundings of dP and delta themselves."""
    q, do = rng.standard_normal((nq, H)), rng.standard_normal((nq, H))
    if kind == "peaked" and k is not None and k.shape[0] > 0:
        for h in range(HEADS):
            hs = slice(h * DH, (h + 1) * DH)
            tgt = rng.integers(k.shape[0], size=nq)
            q[:, hs] = 4.0 * k[tgt, hs]
            do[:, hs] += 0.5 * v[tgt, hs]
        if snap:
            q = _bf(q.astype(F32)).astype(np.float64)
    elif kind == "lastonly":
        do += 0.5 * v[lone]
    elif kind == "ramp":
        q *= 0.5
    return q, do


def make_case(name, path, Sq, Sk, p=0.0, io="f32", layout=None, form="pad", B=7, lens_q=None, lens_k=None, pair=None, n_pairs=None,
              null_mask=False, seed=0, rot=0, call_id=CALL_ID):
    """form: pad (fixed strides), vself (hamt_attn_varlen_*: lens_q, keys = queries), vq (cu_q: lens_q, keys at stride Sk under the
    mask), vk (cu_k: queries at stride Sq, lens_k, no mask).  `pair` [B]: key side of query sequence b, < 0 a filler; None with n_pairs:
    b pairs with b, the sequences behind n_pairs are fillers."""
    rng = _rng(7000 + seed)
    p16 = path == "bf16"
    if form == "pad":
        lens_q, lens_k = [Sq] * B, [Sk] * B
    elif form == "vself":
        B, lens_k = len(lens_q), list(lens_q)
    elif form == "vq":
        B = len(lens_q)
        nks = (max(pair) + 1) if pair is not None else n_pairs
        lens_k = [Sk] * nks
    elif form == "vk":
        B = len(pair) if pair is not None else len(lens_k)
        lens_q = [Sq] * B
    Bk = len(lens_k)
    prs = list(pair) if pair is not None else [b if b < (B if n_pairs is None else n_pairs) else -1 for b in range(B)]
    has_mask = form in ("pad", "vq") and not null_mask
    kinds = KINDS if has_mask else NOMASK_KINDS
    kind_k = [kinds[(j + rot) % len(kinds)] for j in range(Bk)]
    snap = p16                               # peaked q, k on the bf16 grid (see the module's docstring)
    ks, vs, ms, lone = [], [], [], []
    for j in range(Bk):
        k, v, m = _key_side(kind_k[j] if has_mask else "nomask", lens_k[j], rng)
        if kind_k[j] == "peaked" and snap:
            k = _bf(k.astype(F32)).astype(np.float64)
        # one live key is `lastonly` whatever the cycle says: a single key, the head mask of a sample with at most 65 keys, a random
        # mask that left one key
        live = np.flatnonzero(m > MASKED / 2)
        lone.append(0 if lens_k[j] == 1 else (int(live[0]) if len(live) == 1 else -1))
        if lone[j] >= 0:
            kind_k[j] = "lastonly"
        ks.append(k), vs.append(v), ms.append(m)
    qs, dos, kind_q = [], [], []
    for b in range(B):
        j = prs[b]
        kind_q.append("filler" if (j < 0 or lens_k[j] == 0) else kind_k[j])
        q, do = _query_side(kind_q[b], lens_q[b], ks[j] if j >= 0 else None, vs[j] if j >= 0 else None, lone[j] if j >= 0 else -1, rng, snap)
        qs.append(q), dos.append(do)

    def cat(parts):
        a = np.concatenate(parts, axis=0).astype(F32)
        return _bf(a) if io == "bf16" else a
    cu = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)  # noqa: E731
    c = dict(name=name, path=path, io=io, form=form, layout=layout or ("self" if (form in ("pad", "vself") and Sq == Sk) else "cross"),
             B=B, Bk=Bk, Sq=Sq, Sk=Sk, p=float(p), call_id=call_id, q=cat(qs), k=cat(ks), v=cat(vs), do=cat(dos), cuq=cu(lens_q), cuk=cu(lens_k),
             pair=np.array(prs, dtype=np.int32), pair_given=pair is not None, n_pairs=(B if n_pairs is None else n_pairs),
             mask=np.stack(ms).astype(F32) if has_mask else None, kind_q=kind_q, kind_k=kind_k)
    if c["layout"] == "self":
        assert np.array_equal(c["cuq"], c["cuk"]) and c["pair"].tolist() == list(range(B))
    c["F"] = factor_table(c)
    return c


FP32_SHAPES = ((1, 1), (16, 17), (63, 65), (64, 64), (65, 63), (129, 130), (17, 193))
# bf16 path, by the backward kernel; the forward is single-pass but for Sk > 256.  Sk covers one value per KB of the single-pass forward
# (1, 16, 17 -> 2; 33 -> 4; 65 -> 6; 97 -> 8; 129 -> 10; 161 -> 12; 193, 197 -> 14; 225, 256 -> 16), Sq 1, 128 and 129 its query chunks
S128_SHAPES = ((16, 16), (33, 17), (17, 65), (128, 97), (97, 128), (1, 33))                         # NB 2, 4, 6, 8, 8, 4
WIDE_SHAPES = ((129, 1), (1, 129), (129, 129), (197, 197), (224, 224), (224, 17), (128, 161), (128, 193), (129, 130))
TILED_SHAPES = ((225, 225), (1, 225), (257, 64), (65, 257), (1, 257), (64, 320), (129, 256))       # the tiled forward: Sk 257, 320
P_HALF = (("fp32", 129, 130), ("bf16", 97, 128), ("bf16", 197, 197), ("bf16", 65, 257), ("bf16", 225, 225))
BF16_IO = ((33, 17), (129, 129), (65, 257), (225, 225))
VSELF_LENS = (1, 16, 0, 17, 128, 33)


def _name(path, Sq, Sk, p, io="f32", extra=""):
    return f"{path} {Sq}x{Sk}" + (f" p {p:g}" if p else "") + (" bf16io" if io == "bf16" else "") + extra


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  Every shape at p = 0 and 0.1 (the same call id forward and backward), p = 0.5 on one shape per kernel, bf16 in / out on
    one shape per bf16 kernel, one null mask per path, the packed forms with dropout.  The arrays are shared: do not write to them."""
    out = {}
    n = [0]

    def add(name, *a, **kw):
        out[name] = make_case(name, *a, seed=n[0], rot=n[0], **kw)
        n[0] += 1
    for (Sq, Sk) in FP32_SHAPES:
        for p in (0.0, 0.1):
            add(_name("fp32", Sq, Sk, p), "fp32", Sq, Sk, p)
    for (Sq, Sk) in S128_SHAPES + WIDE_SHAPES + TILED_SHAPES:
        for p in (0.0, 0.1):
            add(_name("bf16", Sq, Sk, p), "bf16", Sq, Sk, p)
    for (path, Sq, Sk) in P_HALF:
        add(_name(path, Sq, Sk, 0.5), path, Sq, Sk, 0.5)
    for (Sq, Sk) in BF16_IO:
        for p in (0.0, 0.1):
            add(_name("bf16", Sq, Sk, p, "bf16"), "bf16", Sq, Sk, p, io="bf16")
    add("fp32 64x64 null mask", "fp32", 64, 64, 0.0, null_mask=True)
    add("bf16 97x128 null mask p 0.1", "bf16", 97, 128, 0.1, null_mask=True)
    add("bf16 197x197 null mask", "bf16", 197, 197, 0.0, null_mask=True)
    # packed forms (bf16 path, the single-pass kernels): descriptor Sq / Sk = the maxima
    add("packed self p 0.1 bf16io", "bf16", 128, 128, 0.1, io="bf16", form="vself", lens_q=VSELF_LENS)
    add("packed self", "bf16", 128, 128, 0.0, form="vself", lens_q=VSELF_LENS)
    add("packed q pair p 0.1", "bf16", 80, 37, 0.1, form="vq", lens_q=(5, 0, 33, 80, 17, 1, 16, 9, 64, 3),
        pair=(2, -1, 0, 1, -1, 3, 6, 4, 5, -1))
    add("packed q fillers behind p 0.1 bf16io", "bf16", 20, 65, 0.1, io="bf16", form="vq", lens_q=(7, 20, 16, 3, 5), n_pairs=3)
    add("packed k pair p 0.1", "bf16", 37, 80, 0.1, form="vk", lens_k=(3, 80, 0, 64, 17), pair=(1, -1, 0, 3, 2, 4))
    add("packed k p 0.5 bf16io", "bf16", 17, 33, 0.5, io="bf16", form="vk", lens_k=(33, 1, 16))
    return out


@functools.lru_cache(maxsize=None)
def nan_cases():
    """B = 3, Sk no multiple of 16; the GPU test overwrites the middle sample's q, k, v, dO with NaN and looks at samples 0 and 2 only"""
    specs = (("bf16", 33, 17, 0.0, "f32"), ("bf16", 129, 130, 0.1, "f32"), ("bf16", 65, 257, 0.0, "bf16"), ("fp32", 63, 65, 0.1, "f32"))
    return [make_case("nan neighbour " + _name(pa, Sq, Sk, p, io), pa, Sq, Sk, p, io=io, B=3, layout="cross", seed=500 + i, rot=2 * i)
            for i, (pa, Sq, Sk, p, io) in enumerate(specs)]


def autograd_cases(call_id):
    """what test_gpu_attn.py sends through ops.attention: the packed [q | k | v] buffer and a cross case, p = 0.1, bf16 path"""
    return [make_case("autograd self 80x80 p 0.1", "bf16", 80, 80, 0.1, B=3, seed=600, rot=0, call_id=call_id),
            make_case("autograd cross 37x80 p 0.1", "bf16", 37, 80, 0.1, B=3, seed=601, rot=2, call_id=call_id)]


def pairs(c):
    """(b, key side or -1, query rows, key rows) of every query sequence that has rows"""
    for b in range(c["B"]):
        rq = slice(int(c["cuq"][b]), int(c["cuq"][b + 1]))
        if rq.stop == rq.start:
            continue
        j = int(c["pair"][b])
        rk = slice(int(c["cuk"][j]), int(c["cuk"][j + 1])) if j >= 0 else slice(0, 0)
        yield b, (j if rk.stop > rk.start else -1), rq, rk


def row_kinds(c):
    """the kind of every row of q / out / dq and of k / dk / dv, and of every key row whether a workgroup writes its gradient.  The key
    rows of a single query carry the suffix " q1": their dk / dv are one term, not a sum over queries, and the roundings of that one
    dP and delta meet no averaging -- a cap of their own keeps them from widening the cap of the ordinary rows."""
    kq = np.array([c["kind_q"][b] for b in range(c["B"]) for _ in range(c["cuq"][b + 1] - c["cuq"][b])], dtype=object)
    kk = np.array([c["kind_k"][j] for j in range(c["Bk"]) for _ in range(c["cuk"][j + 1] - c["cuk"][j])], dtype=object)
    written = np.zeros(c["k"].shape[0], dtype=bool)
    for _, j, rq, rk in pairs(c):
        if j >= 0:
            written[rk] = True
            if rq.stop - rq.start == 1:
                kk[rk] = c["kind_k"][j] + " q1"
    return kq, kk, written


# ---------------------------------------------------------------------------------------------- masks
def factor_table(c, call_id=None, per_key=False, row_sk=False, hb_swap=False, stream32=None, no_inv_keep=False):
    """f [B, heads, Sq, Sk] (descriptor sizes) of fp32 1 / (1 - p) or 0, None where p = 0.  The mistakes: one draw per key instead of per
    group of four (the first uniform of every group of a four times wider stream), the row built with Sk in place of Sq, h B + b in
    place of b heads + h, the other path's stream, the factor of a kept element left at 1."""
    p = c["p"]
    if not p > 0:
        return None
    B, Sq, Sk = c["B"], c["Sq"], c["Sk"]
    key = rng_key(SEED, 0, c["call_id"] if call_id is None else call_id)
    b, h, q = np.meshgrid(np.arange(B), np.arange(HEADS), np.arange(Sq), indexing="ij")
    row = (h * B + b if hb_swap else b * HEADS + h) * (Sk if row_sk else Sq) + q
    if (c["path"] == "fp32") if stream32 is None else stream32:
        idx = row[..., None] * Sk + np.arange(Sk)
        f = drop_scale(key, int(idx.max()) + 1, p)[idx]
    else:
        C4, R = -(-Sk // 4) * 4, int(row.max()) + 1
        t = drop_scale4(key, R, 4 * C4, p)[:, ::4] if per_key else drop_scale4(key, R, C4, p)
        f = t[row][..., :Sk]
    if no_inv_keep:
        f = (f > 0).astype(F32)
    return np.ascontiguousarray(f, dtype=F32)


# ---------------------------------------------------------------------------------------------- float64 statement
_REF = {}


def attn64(c):
    """out, dq [Mq, heads, 64]; dk, dv [Mk, heads, 64]; lse [B, heads, Sq] (entries behind a sequence's length: 0, `lse_ok` False);
    U: the unit of every row (see `errors`).  Cached per case: do not write to the result."""
    if id(c) in _REF:
        return _REF[id(c)][1]
    f8 = np.float64
    Mq, Mk, B = c["q"].shape[0], c["k"].shape[0], c["B"]
    out, dq, dk, dv = (np.zeros((M, HEADS, DH)) for M in (Mq, Mq, Mk, Mk))
    lse, ok = np.zeros((B, HEADS, c["Sq"])), np.zeros((B, HEADS, c["Sq"]), dtype=bool)
    U = dict(out=np.zeros((Mq, HEADS)), dq=np.zeros((Mq, HEADS)), dk=np.zeros((Mk, HEADS)), dv=np.zeros((Mk, HEADS)), lse=np.ones((B, HEADS, c["Sq"])))
    for b, j, rq, rk in pairs(c):
        nq, nk = rq.stop - rq.start, rk.stop - rk.start
        ok[b, :, :nq] = True
        if j < 0:
            continue
        for h in range(HEADS):
            hs = slice(h * DH, (h + 1) * DH)
            Q, K, V, dO = c["q"][rq, hs].astype(f8), c["k"][rk, hs].astype(f8), c["v"][rk, hs].astype(f8), c["do"][rq, hs].astype(f8)
            S = Q @ K.T * SCALE + (0.0 if c["mask"] is None else c["mask"][j, :nk].astype(f8))
            m = S.max(axis=1)
            l = m + np.log(np.exp(S - m[:, None]).sum(axis=1))
            P = np.exp(S - l[:, None])
            f = 1.0 if c["F"] is None else c["F"][b, h, :nq, :nk].astype(f8)
            Pt = P * f
            O = Pt @ V
            delta = (dO * O).sum(axis=1)
            dP = dO @ V.T
            dS = P * (dP * f - delta[:, None]) * SCALE
            A = SCALE * P * (np.abs(dP * f) + np.abs(delta)[:, None])
            out[rq, h], dq[rq, h], dk[rk, h], dv[rk, h], lse[b, h, :nq] = O, dS @ K, dS.T @ Q, Pt.T @ dO, l
            U["out"][rq, h], U["dv"][rk, h] = (Pt @ np.abs(V)).max(axis=1), (Pt.T @ np.abs(dO)).max(axis=1)
            U["dq"][rq, h], U["dk"][rk, h] = (A @ np.abs(K)).max(axis=1), (A.T @ np.abs(Q)).max(axis=1)
            U["lse"][b, h, :nq] = 1.0 + SCALE * (P * (np.abs(Q) @ np.abs(K).T)).sum(axis=1)
    ref = dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, U=U, lse_ok=ok)
    _REF[id(c)] = (c, ref)
    return ref


# ---------------------------------------------------------------------------------------------- the kernels' precision
def _forward(S, f, Vo, single, rb, no_alpha=False):
    """-> (acc / l, lse).  single: attn_s128_fwd_kernel (one pass, fast exp / log); else the online softmax per 64-key tile of
    attn_fwd_kernel / attn16_fwd_kernel (alpha by the fast exp, the probabilities and the final log by expf / logf).  The row sum takes
    the unrounded, undropped e; rb(e f) -- bf16 on the bf16 path -- enters the P V product BEFORE the 1 / l normalisation."""
    nq, nk = S.shape
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):   # (a mistake may leave a row without a key: NaN is its finding)
        if single:
            m = S.max(axis=1)
            e = fexp(S - m[:, None])
            l = e.sum(axis=1, dtype=F32)
            acc = rb(e if f is None else e * f) @ Vo
            lse = m + flog(l)
        else:
            m, l, acc = np.full(nq, -np.inf, dtype=F32), np.zeros(nq, dtype=F32), np.zeros((nq, DH), dtype=F32)
            for k0 in range(0, nk, 64):
                t = slice(k0, min(k0 + 64, nk))
                mn = np.maximum(m, S[:, t].max(axis=1))
                alpha = np.ones(nq, dtype=F32) if (no_alpha or k0 == 0) else fexp(m - mn)
                e = exp32(S[:, t] - mn[:, None])
                l = l * alpha + e.sum(axis=1, dtype=F32)
                acc = acc * alpha[:, None] + rb(e if f is None else e * f[:, t]) @ Vo[t]
                m = mn
            lse = m + log32(l)
        return acc * (F32(1) / l)[:, None], lse


def restate(c, mut=None):
    """The kernels the case reaches (fwd_kernel / bwd_kernel) in their own precision -> out, lse, dq, dk, dv shaped as attn64's.
    fp32 path (`attn32`): everything fp32, products by fp32 matmul.  bf16 path (`attn16`): Q, K, V, dO rounded to bf16 as MFMA
    operands, scores and the max / sum statistics fp32, bf16(e f) before the normalisation, backward P~ and dS rounded to bf16, delta
    from the unrounded dO and the stored O, dQ of the tiled backward accumulated through memory in the gradient's dtype once per key
    tile, outputs rounded to bf16 where the case says so.  The single-pass forward and the s128 / wide backward use the fast exp / log.
    `mut` switches the mistakes on:
      dropout   ds_no_f, delta_undropped, per_key, row_sk, hb_swap, no_inv_keep, stream32, dq_other_draw
      keys      lose_last_key, pad_zero, mask_next, mask_scaled
      tiles     no_alpha, dq_last_tile"""
    mut = mut or {}
    p16, io16 = c["path"] == "bf16", c["io"] == "bf16"
    rb = _bf if p16 else (lambda x: x)
    ro = _bf if io16 else (lambda x: x)
    fk, bk = fwd_kernel(c), bwd_kernel(c)
    single, fast_b, tiled_b = fk == "attn_s128_fwd_kernel", bk in ("attn_s128_bwd_kernel", "attn_wide_bwd_kernel"), bk in ("attn_bwd_kernel", "attn16_bwd_kernel")
    F = c["F"]
    fm = {k: True for k in ("per_key", "row_sk", "hb_swap", "no_inv_keep") if mut.get(k)}
    if mut.get("stream32"):
        fm["stream32"] = True
    if fm and F is not None:
        F = factor_table(c, **fm)
    Fq = factor_table(c, call_id=c["call_id"] + 1) if (mut.get("dq_other_draw") and F is not None) else F
    Mq, Mk, B = c["q"].shape[0], c["k"].shape[0], c["B"]
    out, dq, dk, dv = (np.zeros((M, HEADS, DH), dtype=F32) for M in (Mq, Mq, Mk, Mk))
    lse = np.zeros((B, HEADS, c["Sq"]), dtype=F32)
    sc = F32(SCALE)
    for b, j, rq, rk in pairs(c):
        nq, nk = rq.stop - rq.start, rk.stop - rk.start
        if j < 0:
            continue
        for h in range(HEADS):
            hs = slice(h * DH, (h + 1) * DH)
            Qo, Ko, Vo, dOv = rb(c["q"][rq, hs]), rb(c["k"][rk, hs]), rb(c["v"][rk, hs]), c["do"][rq, hs]
            dOo = rb(dOv)
            bias = np.zeros(nk, dtype=F32) if c["mask"] is None else c["mask"][(j + 1) % c["Bk"] if mut.get("mask_next") else j, :nk].copy()
            f, fq = (None, None) if F is None else (F[b, h, :nq, :nk], Fq[b, h, :nq, :nk])
            if mut.get("lose_last_key") and nk % 16:
                bias[nk - 1] = -np.inf
            npad = (-nk) % 16 if mut.get("pad_zero") else 0
            if npad:                                 # padding keys with score 0: K = V = 0 rows behind the real ones
                Ko, Vo = (np.concatenate([a, np.zeros((npad, DH), dtype=F32)]) for a in (Ko, Vo))
                bias = np.concatenate([bias, np.zeros(npad, dtype=F32)])
                if f is not None:
                    f, fq = (np.concatenate([a, np.ones((nq, npad), dtype=F32)], axis=1) for a in (f, fq))
            s = Qo @ Ko.T
            S = (s + bias) * sc if mut.get("mask_scaled") else s * sc + bias
            o, l = _forward(S, f, Vo, single, rb, mut.get("no_alpha", False))
            o = ro(o)
            o_delta = ro(_forward(S, None, Vo, single, rb)[0]) if mut.get("delta_undropped") else o
            with np.errstate(invalid="ignore", over="ignore"):
                delta = (dOv * o_delta).sum(axis=1, dtype=F32)
                dp = dOo @ Vo.T
                pr = (fexp if fast_b else exp32)(S - l[:, None])

                def ds_of(ff):
                    g = dp if (ff is None or mut.get("ds_no_f")) else dp * ff
                    return rb((pr * (g - delta[:, None])) * sc)
                pd = rb(pr if f is None else pr * f)
                dsk, dsq = ds_of(f), ds_of(fq)
                gv, gk = pd.T @ dOo, dsk.T @ Qo
                if tiled_b and nk + npad > 64:
                    gq = np.zeros((nq, DH), dtype=F32)
                    for k0 in range(0, nk + npad, 64):
                        t = slice(k0, min(k0 + 64, nk + npad))
                        part = dsq[:, t] @ Ko[t]
                        gq = ro(part if (k0 == 0 or mut.get("dq_last_tile")) else gq + part)
                else:
                    gq = dsq @ Ko
            out[rq, h], lse[b, h, :nq], dq[rq, h], dk[rk, h], dv[rk, h] = o, l, ro(gq), ro(gk[:nk]), ro(gv[:nk])
    res = dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)
    assert all(v.dtype == F32 for v in res.values())
    return res


def attn32(c, mut=None):
    assert c["path"] == "fp32"
    return restate(c, mut)


def attn16(c, mut=None):
    assert c["path"] == "bf16"
    return restate(c, mut)


# ---------------------------------------------------------------------------------------------- errors in the units of the bounds
def errors(c, got, skip_b=()):
    """{(output, kind): worst over the rows of that kind of max_c |err| / U} for the outputs present in `got` (shaped as attn64's).
    U sums the absolute values of the terms of the float64 sum -- what one rounding can move:  out[q] max_c sum_k P~ |V|,
    dv[k] max_c sum_q P~ |dO|, dq[q] max_c sum_k A |K|, dk[k] max_c sum_q A |Q| with A = scale P (|dP f| + |delta|) (the uncancelled
    form of dS), lse 1 + sum_k P scale sum_c |q_c k_c|.  A float64 row whose every TERM is an exact zero, U = 0 (every key of a row
    dropped, a masked key's gradient, a filler) has to be met exactly -- a row that is zero by cancellation only (dq of a row with a
    single live key, where dP f = delta) keeps its unit; NaN counts as an infinite error.  `skip_b`: query samples (and their key sides)
    left out."""
    ref = attn64(c)
    kq, kk, written = row_kinds(c)
    keep_q, keep_k = np.ones(len(kq), dtype=bool), written.copy()
    for b in skip_b:
        keep_q[c["cuq"][b]:c["cuq"][b + 1]] = False
        j = int(c["pair"][b])
        if j >= 0:
            keep_k[c["cuk"][j]:c["cuk"][j + 1]] = False
    res = {}

    def by_kind(name, e, kinds, keep):
        for k in sorted(set(kinds[keep])):
            res[name, k] = float(e[keep & (kinds == k)].max())

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for name in ("out", "dq", "dk", "dv"):
            if name not in got:
                continue
            g, w, U = np.asarray(got[name], dtype=np.float64), ref[name], ref["U"][name]
            e = np.abs(g - w).max(axis=2) / np.where(U > 0, U, 1.0)
            e = np.where(np.isnan(e), np.inf, e)
            zero = U == 0
            e[zero] = np.where((g[zero] == 0).all(axis=1), 0.0, np.inf)
            by_kind(name, e.max(axis=1), *((kq, keep_q) if name in ("out", "dq") else (kk, keep_k)))
        if "lse" in got:
            g = np.asarray(got["lse"], dtype=np.float64)
            e = np.abs(g - ref["lse"]) / ref["U"]["lse"]
            e = np.where(np.isnan(e), np.inf, e)
            for b in range(c["B"]):
                if b in skip_b or not ref["lse_ok"][b].any():
                    continue
                eb = e[b][ref["lse_ok"][b]]
                if c["kind_q"][b] == "filler":
                    eb = np.where(g[b][ref["lse_ok"][b]] == 0, 0.0, np.inf)
                res["lse", c["kind_q"][b]] = max(res.get(("lse", c["kind_q"][b]), 0.0), float(eb.max()))
    return res


GPU_MARGIN, CAUGHT_FACTOR = 8.0, 10.0
ONE_ROUNDING = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -9, "bf16/bf16": 2.0 ** -9}

# Worst values of the restatement against attn64 over cases(), per (path, output, row kind), as printed by
# test_attn_ref.py::test_restatements_are_inside_the_measured_caps (which also asserts that none is exceeded), rounded up to two digits.
# MEASURED_TABLES
MEASURED = {
    "fp32": {
        "out": {"allmask": 0.00029, "headmask": 4.9e-07, "lastonly": 5.2e-08, "nomask": 7e-07, "peaked": 9.7e-06, "ramp": 5.3e-07, "randn": 5.4e-07},
        "lse": {"allmask": 0.00011, "headmask": 8e-08, "lastonly": 7.2e-05, "nomask": 9.5e-08, "peaked": 4.6e-07, "ramp": 2.5e-07, "randn": 8.8e-08},
        "dq": {"allmask": 0.00048, "headmask": 6.3e-07, "lastonly": 6.4e-07, "nomask": 5.2e-07, "peaked": 8.7e-06, "ramp": 9.4e-07, "randn": 5.1e-07},
        "dk": {"allmask": 0.00071, "headmask": 6.7e-07, "lastonly": 4.1e-08, "lastonly q1": 1.2e-07, "nomask": 6.9e-07, "peaked": 8.4e-06, "ramp": 6e-07, "randn": 6.1e-07},
        "dv": {"allmask": 0.00074, "headmask": 7.2e-07, "lastonly": 4.1e-07, "lastonly q1": 4.5e-08, "nomask": 9.3e-07, "peaked": 8.4e-06, "ramp": 5.9e-07, "randn": 6e-07},
    },
    "bf16": {
        "out": {"allmask": 0.0064, "filler": 0, "headmask": 0.0053, "lastonly": 0.0048, "nomask": 0.0083, "peaked": 0.0066, "ramp": 0.0064, "randn": 0.0062},
        "lse": {"allmask": 0.0007, "filler": 0, "headmask": 0.00041, "lastonly": 0.0016, "nomask": 0.00065, "peaked": 4.5e-07, "ramp": 0.00062, "randn": 0.0008},
        "dq": {"allmask": 0.0072, "filler": 0, "headmask": 0.0084, "lastonly": 0.0048, "nomask": 0.014, "peaked": 0.06, "ramp": 0.029, "randn": 0.029},
        "dk": {"allmask": 0.0084, "allmask q1": 0.33, "headmask": 0.0069, "headmask q1": 0.17, "lastonly": 0.00066, "lastonly q1": 0.0011, "nomask": 0.0084, "nomask q1": 0.14, "peaked": 0.069, "peaked q1": 0.4, "ramp": 0.0062, "ramp q1": 0.066, "randn": 0.0061, "randn q1": 0.2},
        "dv": {"allmask": 0.005, "allmask q1": 0.014, "headmask": 0.0054, "headmask q1": 0.014, "lastonly": 0.0031, "lastonly q1": 0.0042, "nomask": 0.0066, "nomask q1": 0.013, "peaked": 0.0066, "peaked q1": 0.0062, "ramp": 0.0033, "ramp q1": 0.0083, "randn": 0.0065, "randn q1": 0.012},
    },
    "bf16/bf16": {
        "out": {"allmask": 0.0035, "filler": 0, "headmask": 0.0026, "lastonly": 0.0042, "nomask": 0.0037, "peaked": 0.0051, "ramp": 0.0042, "randn": 0.0036},
        "lse": {"allmask": 0.00011, "filler": 0, "headmask": 1.1e-07, "lastonly": 5.3e-08, "nomask": 9.9e-08, "peaked": 3.2e-07, "ramp": 2.6e-07, "randn": 1.1e-07},
        "dq": {"allmask": 0.0036, "filler": 0, "headmask": 0.0036, "lastonly": 0.0025, "nomask": 0.0092, "peaked": 0.028, "ramp": 0.0065, "randn": 0.0049},
        "dk": {"allmask": 0.0036, "headmask": 0.0036, "lastonly": 0.00048, "lastonly q1": 0.00092, "nomask": 0.0041, "peaked": 0.024, "ramp": 0.0029, "randn": 0.0048},
        "dv": {"allmask": 0.0039, "headmask": 0.0043, "lastonly": 0.0035, "lastonly q1": 0.0035, "nomask": 0.0037, "peaked": 0.0063, "ramp": 0.0028, "randn": 0.0049},
    },
}


def measure(case_list=None):
    """{path: {output: {kind: worst error of the restatement}}} over the case list"""
    tab = {}
    for c in (cases().values() if case_list is None else case_list):
        for (name, kind), e in errors(c, restate(c)).items():
            d = tab.setdefault(path_key(c), {}).setdefault(name, {})
            d[kind] = max(d.get(kind, 0.0), e)
    return tab


def measured(path, name, kind):
    return MEASURED[path][name][kind]


def cap(path, name, kind):
    """the measured value, at least one rounding of the path; a filler's outputs are exact"""
    return 0.0 if kind == "filler" else max(MEASURED[path][name][kind], ONE_ROUNDING[path])


def bound(path, name, kind):
    return GPU_MARGIN * cap(path, name, kind)


def worst_ratio(c, errs, cap_fn=bound):
    """{output: (worst error / bound over the row kinds, that kind)} of an `errors` result (0 / 0 counts as 0)"""
    out = {}
    for (name, kind), e in errs.items():
        b = cap_fn(path_key(c), name, kind)
        r = (0.0 if e == 0 else np.inf) if b == 0 else e / b
        if name not in out or r > out[name][0]:
            out[name] = (r, kind)
    return out
