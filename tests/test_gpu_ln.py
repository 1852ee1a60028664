"""-m gpu: the LayerNorm family (csrc/norm.hip on csrc/ln_row.h) at op level against tests/_ln_ref.py: every output of hamt_ln_fwd /
hamt_ln_bwd against the float64 statement within 8 x what the fp32 restatement of the kernels' own arithmetic reaches (per output and per
row kind, so the ill-conditioned offset rows do not widen the bound of the others), the bf16 images and everything a mask decides bit
for bit, the three reduction entry points against each other, hamt_ln_bwd_add, and the dropout masks from the integer restatement of
the mask stream.  tests/test_ln_ref.py shows on the CPU that these cases tell a wrong kernel from a right one."""
import ctypes as C

import numpy as np
import pytest
import torch

import _ln_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}                               # output -> (worst error / bound, case): printed by the last test of the file


def _ops():
    from vln_hamt_amd import ops
    return ops


def _lib():
    from vln_hamt_amd import _lib as L
    return L


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits32(a):
    a = host(a) if torch.is_tensor(a) else np.asarray(a, dtype=np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


def bits16(t):
    return np.ascontiguousarray(host(t.view(torch.int16))).view(np.uint16)


def same_bits(got, want):
    return np.array_equal(bits32(got), bits32(want))


def call(name, *args):
    L = _lib()
    L.check(getattr(L.load(), name)(*args), name)
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def rng_state():
    """the device RNG words and the call counter as they were, put back after every test"""
    ops = _ops()
    st, cnt = ops.rng_state(DEV).clone(), ops._call_counter[0]
    yield ops
    ops.rng_state(DEV).copy_(st)
    ops._call_counter[0] = cnt
    torch.cuda.synchronize()


def desc(c, M=None, Mpad=0, io16=0, p_pre=None, p_post=None, cid=0):
    return _lib().LnDesc(c["M"] if M is None else M, c["H"], float(c["eps"]), float(c["p_pre"] if p_pre is None else p_pre),
                         float(c["p_post"] if p_post is None else p_post), cid, Mpad, io16)


def ws_for(c):
    L = _lib()
    return torch.empty(L.workspace_bytes(L.WS_LN_BWD, c["M"], c["H"]) // 4, dtype=torch.float32, device=DEV)


def forward(c, x=None):
    """ops._ln_fwd on the case (seed and call id set as the smallops tests set them where a mask is drawn) -> dict of device tensors"""
    ops = _ops()
    drop = c["p_pre"] > 0 or c["p_post"] > 0
    if drop:
        ops.manual_seed(R.SEED)
        ops._call_counter[0] = R.CALL_ID - 1
    xd = dev(c["x"]) if x is None else x
    y, y16, z, mean, rstd, cid = ops._ln_fwd(xd, dev(c["res"]), dev(c["gamma"]), dev(c["beta"]), c["eps"], c["p_pre"], c["p_post"], True)
    torch.cuda.synchronize()
    assert cid == (R.CALL_ID if drop else 0) and ops._call_counter[0] == (R.CALL_ID if drop else ops._call_counter[0])
    return dict(y=y, y16=y16, z=z, mean=mean, rstd=rstd, cid=cid, gamma=dev(c["gamma"]))


def backward(c, fw):
    ops = _ops()
    if fw["cid"]:
        ops._call_counter[0] = 12345                               # the backward replays the forward's call id, not the counter
    dz, dx, dx16, dgamma, dbeta, dxsum = ops._ln_bwd(dev(c["dy"]), fw["z"], fw["mean"], fw["rstd"], fw["gamma"], c["eps"], c["p_pre"], c["p_post"],
                                                     fw["cid"], True, True, True)
    torch.cuda.synchronize()
    assert (dx is not None) == (c["p_pre"] > 0)
    return dict(dz=dz, dx=dz if dx is None else dx, dx16=dx16, dgamma=dgamma, dbeta=dbeta, dxsum=dxsum)


def bwd_direct(c, fw, dgamma=None, dbeta=None, dxsum=None, ws=None, add=None, dz=None):
    """hamt_ln_bwd / hamt_ln_bwd_add of a case without dropout, the three column outputs as given (None = NULL) -> (dz, ws)"""
    ops = _ops()
    p = ops._p
    ws = ws_for(c) if ws is None else ws
    dz = torch.full((c["M"], c["H"]), float("nan"), device=DEV) if dz is None else dz
    d = desc(c)
    dy = dev(c["dy"])
    if add is None:
        call("hamt_ln_bwd", C.byref(d), p(dy), p(fw["z"]), p(fw["mean"]), p(fw["rstd"]), p(fw["gamma"]), p(dz), None, None, p(dgamma), p(dbeta),
             p(dxsum), p(ws), p(ops.rng_state(DEV)), ops._stream())
    else:
        assert dxsum is None
        call("hamt_ln_bwd_add", C.byref(d), p(dy), p(fw["z"]), p(fw["mean"]), p(fw["rstd"]), p(fw["gamma"]), p(add), p(dz), p(dgamma), p(dbeta), p(ws),
             ops._stream())
    return dz, ws


def check(c, out, add=None, x=None, ref=None):
    """every output in `out` (host arrays) against float64 within its bound; prints and records the worst error / bound per output"""
    errs = R.errors(c, out, add=add, x=x, ref=ref)
    ratios = R.worst_ratio(errs)
    print(f"[ln {c['name']}] worst error / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        if v >= WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (v, c["name"])
    bad = {k: (e, R.bound(*k)) for k, e in errs.items() if not e <= R.bound(*k)}
    assert not bad, (c["name"], bad)


# ---------------------------------------------------------------------------------------------- every case against float64
@pytest.mark.parametrize("name", list(R.cases()))
def test_forward_and_backward_vs_float64(name):
    """z, mean, rstd, y and dz, dx, dgamma, dbeta, dxsum within the bounds; y16 / dx16 are the bf16 rounding of the returned y / dx bit for
    bit with zero padding rows; the exact-zero row gives y == beta bit for bit and finite gradients; under dropout the dropped positions
    of y and dx are exactly 0, z is exactly the residual there (R.errors counts anything else as an infinite error), and the backward
    replays the forward's call id after the counter has moved on."""
    c = R.cases()[name]
    M = c["M"]
    fw = forward(c)
    bw = backward(c, fw)
    out = {k: host(v) for k, v in list(fw.items()) + list(bw.items()) if k in R.ROW_OUTPUTS + R.COL_OUTPUTS}
    assert fw["z"].dtype == torch.float32 and fw["y16"].shape == (R.mpad(M), c["H"]) and bw["dx16"].shape == (R.mpad(M), c["H"])
    check(c, out)
    assert R.image_errors(bits16(fw["y16"]), out["y"], M) == (0, 0)
    assert R.image_errors(bits16(bw["dx16"]), out["dx"], M) == (0, 0)
    if c["p_pre"] == 0:
        assert bw["dx"] is bw["dz"]
    for r in [r for r, k in enumerate(c["kind"]) if k == "zero"][:3]:
        if c["p_post"] == 0:
            assert same_bits(out["y"][r], c["beta"]), r
        assert np.isfinite(out["dz"][r]).all() and out["mean"][r] == 0
    assert all(np.isfinite(v).all() for v in out.values())


def test_constant_rows_stay_finite():
    """variance 0 at eps = 1e-12: rstd = 1e6 times the fp32 mean's rounding, so no value is asserted, only that nothing overflows"""
    c = R.const_case()
    fw = forward(c)
    bw = backward(c, fw)
    for k in ("y", "mean", "rstd", "z"):
        assert np.isfinite(host(fw[k])).all(), k
    for k in ("dz", "dgamma", "dbeta", "dxsum"):
        assert np.isfinite(host(bw[k])).all(), k
    assert (host(fw["rstd"])[:8] <= 1.0001e6).all()                # (never above eps^-1/2: the variance is not negative)


@pytest.mark.parametrize("name", ["37x132", "1x64", "1025x768"])
def test_images_stop_at_their_padding(name):
    """y16 / dx16 as the first Mpad16 rows of a larger pre-filled buffer: rows [M, Mpad16) are zeros, the row behind keeps its fill; with
    Mpad16 = 0 nothing behind row M is written"""
    ops = _ops()
    p = ops._p
    c = R.cases()[name]
    M, H, Mp = c["M"], c["H"], R.mpad(c["M"])
    fill = torch.full((Mp + 1, H), 1.5, dtype=torch.bfloat16, device=DEV)
    fillbits = bits16(fill)[0, 0]
    x, g, b = dev(c["x"]), dev(c["gamma"]), dev(c["beta"])
    for pad in (Mp, 0):
        y16, dx16 = fill.clone(), fill.clone()
        z, y = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV)
        mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        d = desc(c, Mpad=pad)
        call("hamt_ln_fwd", C.byref(d), p(x), p(dev(c["res"])), p(g), p(b), p(z), p(y), p(y16), p(mean), p(rstd), p(ops.rng_state(DEV)), ops._stream())
        dz, ws = torch.empty(M, H, device=DEV), ws_for(c)
        call("hamt_ln_bwd", C.byref(d), p(dev(c["dy"])), p(z), p(mean), p(rstd), p(g), p(dz), None, p(dx16), None, None, None, p(ws),
             p(ops.rng_state(DEV)), ops._stream())
        for img, val in ((y16, y), (dx16, dz)):
            got = bits16(img)
            assert np.array_equal(got[:M], R.bf16_bits(host(val)))
            if pad:
                assert not got[M:Mp].any() and (got[Mp] == fillbits).all()
            else:
                assert (got[M:] == fillbits).all()


# ---------------------------------------------------------------------------------------------- the reduction paths
@pytest.mark.parametrize("name", ["37x132", "37x64", "1025x768", "4100x64", "4097x132", "37x4"])
def test_reduction_paths_agree(name):
    """H % 64 != 0 takes the scalar reduction, H % 64 == 0 the 16-byte one unless an output is not 16-byte aligned: a dgamma / dbeta / dxsum
    that starts one float into its buffer gives the float64 totals within the bound like the aligned call, and leaves the floats around it
    alone; hamt_ln_bwd with the three outputs NULL followed by hamt_ln_bwd_reduce gives the one-call totals bit for bit; every NULL
    combination leaves the other (pre-filled) outputs' neighbours and the absent outputs untouched."""
    ops = _ops()
    p = ops._p
    c = R.cases()[name]
    M, H = c["M"], c["H"]
    ref = R.ln64(c)
    fw = forward(c)
    al = torch.full((3, H + 12), 77.0, device=DEV)              # aligned outputs: al[i, :H] (row pitch a multiple of 16 bytes)
    assert (H + 12) % 4 == 0 and al.data_ptr() % 16 == 0
    dz1, ws1 = bwd_direct(c, fw, al[0, :H], al[1, :H], al[2, :H])
    un = torch.full((3, H + 12), 77.0, device=DEV)              # outputs one float in: un[i, 1 : 1 + H]
    assert un[0, 1:].data_ptr() % 16 == 4
    bwd_direct(c, fw, un[0, 1:1 + H], un[1, 1:1 + H], un[2, 1:1 + H])
    for buf, lo in ((al, 0), (un, 1)):
        got = host(buf)
        assert (got[:, :lo] == 77.0).all() and (got[:, lo + H:] == 77.0).all()
        check(c, dict(dgamma=got[0, lo:lo + H], dbeta=got[1, lo:lo + H], dxsum=got[2, lo:lo + H]), ref=ref)
    print(f"[ln {name}] unaligned totals bit-identical to the aligned ones: {same_bits(un[:, 1:1 + H].contiguous(), al[:, :H].contiguous())}")
    # NULL outputs first, the reduction on its own afterwards
    dz2, ws2 = bwd_direct(c, fw)
    assert same_bits(dz2, dz1)
    two = torch.full((3, H + 12), 77.0, device=DEV)
    call("hamt_ln_bwd_reduce", M, H, p(ws2), p(two[0, :H]), p(two[1, :H]), p(two[2, :H]), ops._stream())
    assert same_bits(two, al)
    # every combination of NULL outputs
    for mask in range(1, 7):
        part = torch.full((3, H + 12), 77.0, device=DEV)
        args = [part[i, :H] if (mask >> i) & 1 else None for i in range(3)]
        bwd_direct(c, fw, *args)
        want = host(al).copy()
        for i in range(3):
            if not (mask >> i) & 1:
                want[i] = 77.0
        assert same_bits(part, want), mask
        part2 = torch.full((3, H + 12), 77.0, device=DEV)
        call("hamt_ln_bwd_reduce", M, H, p(ws2), *[p(part2[i, :H]) if (mask >> i) & 1 else None for i in range(3)], ops._stream())
        assert same_bits(part2, want), mask


# ---------------------------------------------------------------------------------------------- hamt_ln_bwd_add
@pytest.mark.parametrize("name", ["1x64", "37x1020", "1024x64", "2048x132", "37x768"])
def test_bwd_add(name):
    """dz = float64 LayerNorm backward + add within the bound; dgamma / dbeta and the dx column sums left in the workspace are bit-identical
    to the call without `add`; a descriptor with dropout inside the LayerNorm is refused"""
    ops = _ops()
    p = ops._p
    L = _lib()
    c = R.cases()[name]
    M, H = c["M"], c["H"]
    fw = forward(c)
    plain = torch.full((3, H), float("nan"), device=DEV)
    dz0, _ = bwd_direct(c, fw, plain[0], plain[1], plain[2])
    add = dev(c["add"])
    withadd = torch.full((3, H), float("nan"), device=DEV)
    dz, ws = bwd_direct(c, fw, withadd[0], withadd[1], add=add)
    check(c, dict(dz=host(dz), dgamma=host(withadd[0]), dbeta=host(withadd[1])), add=c["add"])
    assert same_bits(withadd[:2], plain[:2])
    assert (np.abs(host(dz) - (host(dz0).astype(np.float64) + c["add"])) <= R.EPS32 * (np.abs(host(dz)) + np.abs(host(dz0)))).all()      # the plain dz plus add: a rounding of each
    call("hamt_ln_bwd_reduce", M, H, p(ws), None, None, p(withadd[2]), ops._stream())
    assert same_bits(withadd[2], plain[2])                         # `add` did not reach the dx column sums either
    for pp, pq in ((0.1, 0.0), (0.0, 0.5)):
        d = desc(c, p_pre=pp, p_post=pq, cid=R.CALL_ID)
        keep = dz.clone()
        with pytest.raises(L.HamtError):
            call("hamt_ln_bwd_add", C.byref(d), p(dev(c["dy"])), p(fw["z"]), p(fw["mean"]), p(fw["rstd"]), p(fw["gamma"]), p(add), p(dz), None, None,
                 p(ws), ops._stream())
        torch.cuda.synchronize()
        assert same_bits(dz, keep)
    with pytest.raises(L.HamtError):                               # and so is a call without `add`
        d = desc(c)
        call("hamt_ln_bwd_add", C.byref(d), p(dev(c["dy"])), p(fw["z"]), p(fw["mean"]), p(fw["rstd"]), p(fw["gamma"]), None, p(dz), None, None, p(ws),
             ops._stream())


def test_unsupported_shapes_are_refused():
    """H outside 4 .. 1024 or no multiple of 4 (forward, backward, reduction), a grouped entry whose H is no multiple of 64 or whose
    output is not 16-byte aligned: an error, and nothing is written"""
    ops = _ops()
    p = ops._p
    L = _lib()
    t = torch.full((4096,), 3.0, device=DEV)
    for H in (0, 2, 6, 1028, 2048):
        d = L.LnDesc(2, H, 1e-12, 0.0, 0.0, 0, 0, 0)
        with pytest.raises(L.HamtError):
            call("hamt_ln_fwd", C.byref(d), p(t), None, p(t), p(t), p(t), p(t), None, p(t), p(t), p(ops.rng_state(DEV)), ops._stream())
        with pytest.raises(L.HamtError):
            call("hamt_ln_bwd", C.byref(d), p(t), p(t), p(t), p(t), p(t), p(t), None, None, p(t), p(t), None, p(t), p(ops.rng_state(DEV)), ops._stream())
        with pytest.raises(L.HamtError):
            call("hamt_ln_bwd_reduce", 2, H, p(t), p(t), None, None, ops._stream())
    table = torch.zeros(64, dtype=torch.int32, device=DEV)
    for H, off in ((132, 0), (64, 1)):
        descs = (L.LnReduceDesc * 1)(L.LnReduceDesc(t.data_ptr(), t[1024 + off:].data_ptr(), None, None, 4, H, 0))
        with pytest.raises(L.HamtError):
            call("hamt_ln_bwd_reduce_grouped", 1, C.byref(descs), p(table), 4 * 64, ops._stream())
    torch.cuda.synchronize()
    assert (host(t) == 3.0).all() and not host(table).any()


# ---------------------------------------------------------------------------------------------- the grouped reduction
def test_reduce_grouped():
    """65 entries (one more than a kernarg chunk) over six backward calls of H = 64 / 128 / 768 and M on both sides of 1024 and 2048, a third
    of the outputs NULL.  Entries 0 and 1 add their dgamma into one buffer that holds 5.0 (atomic bit 0), entry 2 has the bit clear and
    overwrites a buffer that holds 5.0.  Every output against the float64 column sums of the same dy and z within the bound, the stored
    ones bit-identical to hamt_ln_bwd_reduce's; a table one entry too small is refused and writes nothing."""
    ops = _ops()
    p = ops._p
    L = _lib()
    cs = R.grouped_cases()
    prob = []
    for c in cs:
        fw = forward(c)
        _, ws = bwd_direct(c, fw)
        single = torch.full((3, c["H"]), float("nan"), device=DEV)
        call("hamt_ln_bwd_reduce", c["M"], c["H"], p(ws), p(single[0]), p(single[1]), p(single[2]), ops._stream())
        ref = R.ln64(c)
        check(c, dict(dgamma=host(single[0]), dbeta=host(single[1]), dxsum=host(single[2])), ref=ref)
        prob.append(dict(c=c, ws=ws, single=single, ref=ref, units=R.col_units(ref)))
    n = R.GROUPED_N
    assert n == 65 and cs[0]["H"] == cs[2]["H"] == 64 and R.geometry(cs[0]["M"])[0] != R.geometry(cs[2]["M"])[0]
    which = [0, 2, 0] + [(e * 5 + 1) % len(cs) for e in range(3, n)]                     # entry -> problem
    assert set(which[3:]) == set(range(len(cs))) and {cs[w]["H"] for w in which} == {64, 128, 768}
    shared = torch.full((64,), 5.0, device=DEV)
    outs, descs = [], (L.LnReduceDesc * n)()
    for e in range(n):
        H = cs[which[e]]["H"]
        o = [torch.full((H,), 5.0 if e < 3 else float("nan"), device=DEV) for _ in range(3)]
        live = [True, e % 3 != 1, e % 3 != 2] if e >= 3 else [True, e == 1, e == 2]
        if e < 2:
            o[0] = shared
        outs.append([t if l else None for t, l in zip(o, live)])
        descs[e] = L.LnReduceDesc(prob[which[e]]["ws"].data_ptr(), *[(t.data_ptr() if t is not None else None) for t in outs[e]],
                                  cs[which[e]]["M"], H, 1 if e < 2 else 0)
    assert outs[64][0] is not None and sum(t is None for o in outs for t in o) >= n // 2
    table = torch.zeros(n * L.LNRED_TABLE_ENTRY // 4, dtype=torch.int32, device=DEV)
    with pytest.raises(L.HamtError):
        call("hamt_ln_bwd_reduce_grouped", n, C.byref(descs), p(table), (n - 1) * L.LNRED_TABLE_ENTRY, ops._stream())
    torch.cuda.synchronize()
    assert not host(table).any() and (host(shared) == 5.0).all()
    call("hamt_ln_bwd_reduce_grouped", n, C.byref(descs), p(table), n * L.LNRED_TABLE_ENTRY, ops._stream())
    for e in range(2, n):
        for i, t in enumerate(outs[e]):
            if t is not None:
                assert same_bits(t, prob[which[e]]["single"][i]), (e, i)
    a, b = prob[0], prob[2]
    want = 5.0 + a["ref"]["dgamma"] + b["ref"]["dgamma"]
    unit = R.EPS32 * (5.0 + a["units"]["dgamma"] + b["units"]["dgamma"])
    err = np.abs(host(shared) - want) / unit
    print(f"[ln grouped] two entries added into one dgamma: worst error / bound {err.max() / R.bound('dgamma'):.3f}")
    assert (err <= R.bound("dgamma")).all()
    assert same_bits(outs[1][1], b["single"][1])                   # entry 1's dbeta has its bit clear: stored


# ---------------------------------------------------------------------------------------------- dropout
def test_pre_and_post_masks_are_the_restated_independent_streams():
    """both masks at once: the kept positions read off the GPU's z (!= residual) and y (!= 0) are the restated masks of call_id and of
    call_id ^ POST_SALT, and they agree where two independent masks of these rates would (keep_rate4), within 5 standard deviations"""
    c = R.cases()["both 1030x768 p 0.5/0.1"]
    fw = forward(c)
    z, y = host(fw["z"]), host(fw["y"])
    rows = np.array([k in ("randn", "big", "small") for k in c["kind"]])
    kp, kq = (z != c["res"])[rows], (y != 0)[rows]
    assert np.array_equal(kp, (c["fpre"] != 0)[rows]) and np.array_equal(kq, (c["fpost"] != 0)[rows])
    assert same_bits(np.where(c["fpre"] == 0, z, 0), np.where(c["fpre"] == 0, c["res"], 0))
    rp, rq = R.keep_rate4(c["p_pre"]), R.keep_rate4(c["p_post"])
    want = rp * rq + (1 - rp) * (1 - rq)
    sd = np.sqrt(want * (1 - want) / kp.size)
    agree = float((kp == kq).mean())
    print(f"[ln masks] agreement of the pre and post masks {agree:.5f}, independent masks {want:.5f} +- {sd:.5f}")
    assert abs(agree - want) <= 5 * sd and not np.array_equal(kp, kq)
    assert abs(kp.mean() - rp) <= 5 * np.sqrt(rp * (1 - rp) / kp.size) and abs(kq.mean() - rq) <= 5 * np.sqrt(rq * (1 - rq) / kq.size)


def test_dxsum_under_p_pre_sums_dx_not_dz():
    c = R.cases()["pre 1030x64 p 0.5"]
    fw = forward(c)
    bw = backward(c, fw)
    dz, dx, dxsum = host(bw["dz"]), host(bw["dx"]), host(bw["dxsum"])
    assert same_bits(dx, dz * c["fpre"])                           # dx = dz * f, one fp32 product, exactly 0 where dropped
    ref = R.ln64(c)
    unit = R.EPS32 * R.col_units(ref)["dxsum"]
    assert (np.abs(dxsum - dx.astype(np.float64).sum(0)) <= R.bound("dxsum") * unit).all()
    assert (np.abs(dxsum - dz.astype(np.float64).sum(0)) > R.CAUGHT_FACTOR * R.bound("dxsum") * unit).any()


# ---------------------------------------------------------------------------------------------- formats
@pytest.mark.parametrize("fmt", [torch.bfloat16, torch.float16])
def test_16_bit_x_and_z_on_offset_rows(fmt):
    """x as bf16 / half equals the same values given as fp32 (y, mean, rstd bit for bit), on a case with offset rows and a residual.  The z
    saved in the 16-bit format gives a dz within that rounding of the dz from the fp32-saved z: z' = z (1 + d) moves xhat_c by at most
    D_c = |z_c| rstd |d| and c2 = mean(u xhat) by at most E = mean(|u| D), so dz_c by at most rstd (D_c |c2| + (|xhat_c| + D_c) E), plus the
    fp32 bound of either dz.  |d| is taken as 2^-9 (bf16) / 2^-12 (half): the rounding of a value at the top of its binade, half of the
    formats' unit roundoff 2^-8 / 2^-11 that z itself is held to -- the sums of absolute values above leave room for that factor.  Below
    half's smallest normal number, 2^-14, the rounding is absolute, 2^-25, and D_c is taken from that."""
    ops = _ops()
    c = R.cases()["37x132"]
    assert c["res"] is not None and "off100" in c["kind"]
    x16 = dev(c["x"]).to(fmt)
    xv = host(x16.float())
    saved = ops.LN_Z16
    try:
        ops.LN_Z16 = True
        a = forward(c, x=x16)
        ops.LN_Z16 = False
        b = forward(c, x=x16)
    finally:
        ops.LN_Z16 = saved
    f = forward(c, x=x16.float())
    assert a["z"].dtype == fmt and b["z"].dtype == torch.float32 and f["z"].dtype == torch.float32
    for k in ("y", "mean", "rstd"):
        assert same_bits(a[k], f[k]) and same_bits(b[k], f[k]), k
    assert same_bits(b["z"], f["z"]) and np.array_equal(bits16(a["y16"]), bits16(f["y16"]))
    ref = R.ln64(c, x=xv)
    check(c, {k: host(f[k]) for k in ("y", "mean", "rstd", "z")}, x=xv, ref=ref)
    u = 2.0 ** -9 if fmt == torch.bfloat16 else 2.0 ** -12
    zr = host(a["z"].float()).astype(np.float64)
    sub = 0.0 if fmt == torch.bfloat16 else 2.0 ** -25             # half a step of half's subnormals: the 1e-3 randn rows reach below 2^-14
    assert (np.abs(zr - ref["z"]) <= np.maximum(np.abs(ref["z"]) * (2 * u + 2 * R.EPS32), sub)).all() and not np.array_equal(zr, ref["z"])
    dza, dzb = host(backward(c, a)["dz"]), host(backward(c, b)["dz"])
    check(c, dict(dz=dzb), x=xv, ref=ref)
    rs = ref["rstd"][:, None]
    D = np.maximum(np.abs(ref["z"]) * u, sub) * rs
    uu = ref["a"] * c["gamma"].astype(np.float64)
    c2 = np.abs((uu * ref["xh"]).mean(axis=1, keepdims=True))
    E = (np.abs(uu) * D).mean(axis=1, keepdims=True)
    kinds = np.array([R.bound("dz", k) for k in c["kind"]])[:, None]
    bnd = rs * (D * c2 + (np.abs(ref["xh"]) + D) * E) + 2 * kinds * np.abs(ref["dz"]).max(axis=1, keepdims=True)
    diff = np.abs(dza.astype(np.float64) - dzb)
    live = bnd > 0
    print(f"[ln z as {fmt}] worst |dz(z16) - dz(z32)| / bound {np.max(diff[live] / bnd[live]):.3f}")
    assert (diff <= bnd).all()
    assert diff.max() > 0                                            # (the 16-bit z was really what the backward read)


def test_zz_report_the_margins():
    """not a check: the worst error / bound per output over the tests of this file that ran before it"""
    for k, (v, name) in sorted(WORST.items()):
        print(f"[ln margins] {k:7s} worst error / bound {v:.3f}  ({name})")
