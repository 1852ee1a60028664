"""-m gpu: the attention kernels (csrc/attn.hip, csrc/attn16.hip) at op level against tests/_attn_ref.py: out, lse, dq, dk, dv of
hamt_attn_small_fwd / _bwd and of the hamt_attn_varlen* entry points against the float64 statement, per output row in the unit of what
one rounding can move, within 8 x what the restatement of the kernels' own arithmetic reaches (per path, output and row kind); the
dropout masks rebuilt on the host from the seed and the call id; every output allocated between NaN guard rows and with NaN padding
columns that must come back untouched; every input's guard rows and padding columns NaN as well, so a stray read shows as a NaN
result.  tests/test_attn_ref.py shows on the CPU that these cases tell a wrong kernel from a right one.

Which kernel a case launches, from the rules of hamt_attn_small_* / hamt_attn16_*_launch (attn16.hip: use_s128_fwd, use_s128_bwd,
use_wide_bwd, launch_s128_fwd's KB, launch_s128_bwd's NB); every shape runs at p = 0 and p = 0.1, the starred ones at p = 0.5 too,
"io" marks bf16 in / out next to fp32 in / out:

  fp32 path   attn_fwd_kernel + attn_bwd_kernel (64 x 64 tiles)   1x1  16x17  63x65  64x64 (+ null mask)  65x63  129x130*  17x193
  bf16 path   forward                        backward                       Sq x Sk
              attn_s128_fwd KB 2             attn_s128_bwd NB 2             16x16
              attn_s128_fwd KB 2             attn_s128_bwd NB 4             33x17 io
              attn_s128_fwd KB 4             attn_s128_bwd NB 4             1x33
              attn_s128_fwd KB 6             attn_s128_bwd NB 6             17x65
              attn_s128_fwd KB 8             attn_s128_bwd NB 8             128x97  97x128* (+ null mask)
              attn_s128_fwd KB 2             attn_wide_bwd                  129x1  224x17
              attn_s128_fwd KB 10            attn_wide_bwd                  1x129  129x129 io  129x130
              attn_s128_fwd KB 12            attn_wide_bwd                  128x161
              attn_s128_fwd KB 14            attn_wide_bwd                  128x193  197x197* (+ null mask)  224x224
              attn_s128_fwd KB 16            attn16_bwd (tiled)             225x225* io  1x225  129x256
              attn_s128_fwd KB 4             attn16_bwd (tiled)             257x64
              attn16_fwd (tiled)             attn16_bwd (tiled)             65x257* io  1x257  64x320
  packed      attn_s128_fwd KB 8 + attn_s128_bwd NB 8   hamt_attn_varlen_*: lens 1, 16, 0, 17, 128, 33 (fp32 io; bf16 io at p 0.1)
              attn_s128_fwd KB 4 + attn_s128_bwd NB 6   hamt_attn_varlen_cross_*, cu_q + pair + fillers (Sq <= 80, Sk 37, p 0.1)
              attn_s128_fwd KB 6 + attn_s128_bwd NB 6   cu_q, fillers behind n_pairs (Sq <= 20, Sk 65, p 0.1, bf16 io)
              attn_s128_fwd KB 6 + attn_s128_bwd NB 6   cu_k + pair + a filler + an empty key sequence (Sq 37, Sk <= 80, p 0.1)
              attn_s128_fwd KB 4 + attn_s128_bwd NB 4   cu_k (Sq 17, Sk <= 33, p 0.5, bf16 io)
The four in / out dtype pairs of a kernel share one body (the loads and stores are the template's only typed parts): fp32 / fp32 and
bf16 / bf16 cover both of each."""
import ctypes as C

import numpy as np
import pytest
import torch

import _attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, PADC, LSE_GUARD = 3, 8, 64        # guard rows in front of and behind every matrix, padding columns per row, guard floats around lse
WORST = {}                               # (kernel, output) -> (worst error / bound, case, kind): printed by the last test of the file


def _ops():
    from vln_hamt_amd import ops
    return ops


def _lib():
    from vln_hamt_amd import _lib as L
    return L


@pytest.fixture(autouse=True)
def rng_state():
    """the device RNG words and the call counter as they were, put back after every test"""
    ops = _ops()
    st, cnt = ops.rng_state(DEV).clone(), ops._call_counter[0]
    yield ops
    ops.rng_state(DEV).copy_(st)
    ops._call_counter[0] = cnt
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Guarded:
    """a [GUARD + M + GUARD, width + PADC] matrix of NaN whose columns [0, width) of rows [GUARD, GUARD + M) are the payload"""

    def __init__(self, M, width, dtype):
        self.M, self.width = M, width
        self.buf = torch.full((2 * GUARD + M, width + PADC), float("nan"), dtype=dtype, device=DEV)
        self.ld = width + PADC

    def cols(self, c0, c1):
        return self.buf[GUARD:GUARD + self.M, c0:c1]

    def fill(self, c0, a):
        self.cols(c0, c0 + a.shape[1]).copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))

    def snapshot(self):
        self.before = _bits(self.buf).clone()

    def untouched_outside(self, written):
        """`written` [M, width] bool (host): everything else still holds the bits it held at the snapshot"""
        w = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        w[GUARD:GUARD + self.M, :self.width] = torch.from_numpy(written).to(DEV)
        return bool(torch.equal(_bits(self.buf)[~w], self.before[~w]))


def run_case(c, poison_b=None):
    """forward and backward of the case through the C entry points -> (results shaped as attn64's, list of violated guards)"""
    ops, L = _ops(), _lib()
    lib, p = L.load(), ops._p
    ops.manual_seed(R.SEED)
    rng = ops.rng_state(DEV)
    H, hd = R.H, R.HEADS
    io16 = c["io"] == "bf16"
    tdt, hdt = (torch.bfloat16, L.HAMT_BF16) if io16 else (torch.float32, L.HAMT_F32)
    Mq, Mk, B, Sq, Sk = c["q"].shape[0], c["k"].shape[0], c["B"], c["Sq"], c["Sk"]
    if c["layout"] == "self":
        src, grad = Guarded(Mq, 3 * H, tdt), Guarded(Mq, 3 * H, tdt)
        qs = ks = vs = src
        gq = gk = gv = grad
        qc, kc, vc = 0, H, 2 * H
    else:
        qs, ks, gq, gk = Guarded(Mq, H, tdt), Guarded(Mk, 2 * H, tdt), Guarded(Mq, H, tdt), Guarded(Mk, 2 * H, tdt)
        vs, gv = ks, gk
        qc, kc, vc = 0, 0, H
    for g, col, name in ((qs, qc, "q"), (ks, kc, "k"), (vs, vc, "v")):
        g.fill(col, c[name])
    o, do = Guarded(Mq, H, tdt), Guarded(Mq, H, tdt)
    do.fill(0, c["do"])
    if poison_b is not None:
        rq, rk = slice(c["cuq"][poison_b], c["cuq"][poison_b + 1]), slice(c["cuk"][poison_b], c["cuk"][poison_b + 1])
        qs.cols(qc, qc + H)[rq] = float("nan")
        ks.cols(kc, kc + H)[rk] = float("nan")
        vs.cols(vc, vc + H)[rk] = float("nan")
        do.cols(0, H)[rq] = float("nan")
    n_lse = B * hd * Sq
    lse = torch.full((2 * LSE_GUARD + n_lse,), float("nan"), device=DEV)
    lse_v = lse[LSE_GUARD:LSE_GUARD + n_lse]
    mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(DEV).contiguous()
    cuq, cuk, pair = (torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("cuq", "cuk", "pair"))
    d = L.AttnDesc(B, hd, Sq, Sk, R.DH, qs.ld, ks.ld, vs.ld, o.ld, hdt, hdt, R.SCALE, c["p"], c["call_id"],
                   L.PREC_BF16 if c["path"] == "bf16" else L.PREC_F32)
    q, k, v = qs.cols(qc, qc + H), ks.cols(kc, kc + H), vs.cols(vc, vc + H)
    dq, dk, dv = gq.cols(qc, qc + H), gk.cols(kc, kc + H), gv.cols(vc, vc + H)
    ov, dov = o.cols(0, H), do.cols(0, H)
    for g in {o, gq, gk, gv}:
        g.snapshot()
    lse_before = _bits(lse).clone()
    st = ops._stream()
    form = c["form"]
    if form == "pad":
        L.check(lib.hamt_attn_small_fwd(C.byref(d), p(q), p(k), p(v), p(mask), p(ov), p(lse_v), p(rng), st), "hamt_attn_small_fwd")
        L.check(lib.hamt_attn_small_bwd(C.byref(d), p(q), p(k), p(v), p(mask), p(ov), p(dov), p(lse_v), None, p(dq), p(dk), p(dv), p(rng), st),
                "hamt_attn_small_bwd")
    elif form == "vself":
        L.check(lib.hamt_attn_varlen_fwd(C.byref(d), p(q), p(k), p(v), p(cuq), p(ov), p(lse_v), p(rng), st), "hamt_attn_varlen_fwd")
        L.check(lib.hamt_attn_varlen_bwd(C.byref(d), p(q), p(k), p(v), p(cuq), p(ov), p(dov), p(lse_v), p(dq), p(dk), p(dv), p(rng), st),
                "hamt_attn_varlen_bwd")
    else:
        a_q, a_k = (p(cuq), None) if form == "vq" else (None, p(cuk))
        a_pair = p(pair) if c["pair_given"] else None
        L.check(lib.hamt_attn_varlen_cross_fwd(C.byref(d), p(q), p(k), p(v), a_q, a_k, c["n_pairs"], a_pair, p(mask), p(ov), p(lse_v), p(rng), st),
                "hamt_attn_varlen_cross_fwd")
        L.check(lib.hamt_attn_varlen_cross_bwd(C.byref(d), p(q), p(k), p(v), a_q, a_k, c["n_pairs"], a_pair, p(mask), p(ov), p(dov), p(lse_v),
                                               p(dq), p(dk), p(dv), p(rng), st), "hamt_attn_varlen_cross_bwd")
    torch.cuda.synchronize()
    # what may have been written: every query row's out / dq, the key rows some query sequence names, the lse of the real queries
    _, _, kw = R.row_kinds(c)
    allq = np.ones((Mq, H), dtype=bool)
    keyw = np.repeat(kw[:, None], H, axis=1)
    bad = []
    if not o.untouched_outside(allq):
        bad.append("out")
    if c["layout"] == "self":
        if not gq.untouched_outside(np.concatenate([allq, keyw, keyw], axis=1)):
            bad.append("dq | dk | dv")
    else:
        if not gq.untouched_outside(allq):
            bad.append("dq")
        if not gk.untouched_outside(np.concatenate([keyw, keyw], axis=1)):
            bad.append("dk | dv")
    ok = R.attn64(c)["lse_ok"].reshape(-1)
    lw = torch.zeros(lse.shape, dtype=torch.bool, device=DEV)
    lw[LSE_GUARD:LSE_GUARD + n_lse] = torch.from_numpy(ok).to(DEV)
    if not torch.equal(_bits(lse)[~lw], lse_before[~lw]):
        bad.append("lse")

    def host(t, M):
        return t.float().cpu().numpy().reshape(M, hd, R.DH)
    lse_h = lse_v.cpu().numpy().reshape(B, hd, Sq).copy()
    lse_h[~R.attn64(c)["lse_ok"]] = 0.0
    got = dict(out=host(ov, Mq), lse=lse_h, dq=host(dq, Mq), dk=host(dk, Mk), dv=host(dv, Mk))
    return got, bad


def check(c, got, bad, skip_b=()):
    errs = R.errors(c, got, skip_b=skip_b)
    ratios = R.worst_ratio(c, errs)
    lines = [f"{name}: {r:.3g} x its bound ({kind})" for name, (r, kind) in sorted(ratios.items())]
    print(f"[{c['name']}] " + "  ".join(lines))
    for name, (r, kind) in ratios.items():
        key = (R.kernel_of(c, name), name)
        if key not in WORST or r > WORST[key][0]:
            WORST[key] = (r, c["name"], kind)
    detail = {f"{n} {k}": f"{e:.3g} / {R.bound(R.path_key(c), n, k):.3g}" for (n, k), e in sorted(errs.items())
              if e > R.bound(R.path_key(c), n, k)}
    assert not bad, (c["name"], "written outside the output", bad)
    if not skip_b:
        _, _, written = R.row_kinds(c)
        for name in ("out", "dq"):
            assert np.isfinite(got[name]).all(), (c["name"], name, "not finite")
        for name in ("dk", "dv"):
            assert np.isfinite(got[name][written]).all(), (c["name"], name, "not finite")
        assert "lse" not in got or np.isfinite(got["lse"]).all(), (c["name"], "lse not finite")
    assert all(r <= 1.0 for r, _ in ratios.values()), (c["name"], lines, detail)


@pytest.mark.parametrize("name", list(R.cases()))
def test_case_against_float64(name):
    c = R.cases()[name]
    check(c, *run_case(c))


@pytest.mark.parametrize("i", range(len(R.nan_cases())), ids=[c["name"] for c in R.nan_cases()])
def test_nan_in_the_neighbouring_sample_stays_there(i):
    """q, k, v and dO of the middle sample are NaN: samples 0 and 2 are inside their bounds and hold no NaN (padding keys get P = 0, so
    a read that runs over into the neighbour shows only when the neighbour is NaN); the middle sample's results are not looked at"""
    c = R.nan_cases()[i]
    got, bad = run_case(c, poison_b=1)
    for b in (0, 2):
        rq, rk = slice(c["cuq"][b], c["cuq"][b + 1]), slice(c["cuk"][b], c["cuk"][b + 1])
        for nm, r in (("out", rq), ("dq", rq), ("dk", rk), ("dv", rk)):
            assert np.isfinite(got[nm][r]).all(), (c["name"], nm, b)
        assert np.isfinite(got["lse"][b]).all(), (c["name"], "lse", b)
    check(c, got, bad, skip_b=(1,))


@pytest.mark.parametrize("which", (0, 1), ids=("packed qkv buffer", "cross"))
def test_attention_through_autograd_draws_the_forward_mask_in_the_backward(which):
    """ops.attention at p = 0.1: AttnFn takes the next call id, hands it and the device RNG words to both kernels -- with another
    attention call (another call id) between its forward and its backward"""
    ops = _ops()
    ops.manual_seed(R.SEED)
    ops._call_counter[0] = R.CALL_ID - 1
    c = R.autograd_cases(R.CALL_ID)[which]
    B, H = c["B"], R.H
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    mask = dev(c["mask"]).view(B, 1, 1, c["Sk"])
    if c["layout"] == "self":
        q_src = torch.cat([dev(c["q"]), dev(c["k"]), dev(c["v"])], dim=1).requires_grad_()
        kv_src = None
    else:
        q_src, kv_src = dev(c["q"]).requires_grad_(), torch.cat([dev(c["k"]), dev(c["v"])], dim=1).requires_grad_()
    out = ops.attention(q_src, kv_src, mask, B, R.HEADS, c["p"], "bf16")
    assert ops._call_counter[0] == R.CALL_ID
    ops.attention(q_src.detach(), None if kv_src is None else kv_src.detach(), mask, B, R.HEADS, c["p"], "bf16")
    assert ops._call_counter[0] == R.CALL_ID + 1
    out.backward(dev(c["do"]))
    torch.cuda.synchronize()
    g = q_src.grad.cpu().numpy()
    gkv = g[:, H:] if kv_src is None else kv_src.grad.cpu().numpy()
    sh = lambda a: np.ascontiguousarray(a).reshape(-1, R.HEADS, R.DH)  # noqa: E731
    got = dict(out=sh(out.detach().cpu().numpy()), dq=sh(g[:, :H]), dk=sh(gkv[:, :H]), dv=sh(gkv[:, H:]))
    check(c, got, [])


def test_report_worst_ratios():
    """the worst error / bound per (kernel, output) over everything above: for the reader, not used to set anything"""
    for (kern, name), (r, case, kind) in sorted(WORST.items()):
        print(f"[attention worst] {kern:22s} {name:3s} {r:.3g} x its bound  ({case}, {kind})")
    assert all(r <= 1.0 for r, _, _ in WORST.values())
