"""-m gpu: the small reduction, activation-gradient, dropout, cast and elementwise kernels (hamt_colsum / hamt_smallk_wgrad of
csrc/gemm.hip, the elementwise half of csrc/elementwise.hip) at op level against tests/_smallops_ref.py: float64 within a derived
summation bound for the reductions, the fp32 statement bit for bit for everything that is one rounded operation, the integer
restatement of the counter-based RNG for the dropout masks.  tests/test_smallops_ref.py shows on the CPU that the cases tell a wrong
kernel from a right one and that the RNG restatement is a sound generator (no statistics are taken here)."""
import numpy as np
import pytest
import torch

import _smallops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vln_hamt_amd import ops
    return ops


def _lib():
    from vln_hamt_amd import _lib as L
    return L


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(DEV)


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


def _ps():
    ops = _ops()
    return ops._p, ops._stream


# ---------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("M", R.COLSUM_M)
def test_colsum_vs_float64_per_column(M, dtype):
    """A strided view (column offset 3, ldx = N + 5) of fp32 / bf16 rows; plain, accumulate=True into a non-zero out, and an out that
    starts one float into its buffer (the scalar reduce_partials_kernel also where N % 4 == 0).  Per column
    |err| <= eps32 (ceil(rows per chunk / 4) + 2 + ceil(chunks / 4) + 2) sum|x|.  The unaligned result is held to float64 like the
    aligned one, not to its bits: the scalar kernel adds the chunk sums as four interleaved phases, (c0 + c4 + ..) + (c1 + c5 + ..) ...,
    the 16-byte kernel in chunk order, so the two differ in the last bit from four chunks on."""
    ops = _ops()
    for N in R.COLSUM_N:
        c = R.colsum_case(M, N, dtype)
        x = (dev(c["buf"]) if dtype == "f32" else dev_bf16(c["bits"]))[:, 3:3 + N]
        assert x.stride(0) == N + 5 and x.dtype == (torch.float32 if dtype == "f32" else torch.bfloat16)
        want, bound = R.colsum_f64(c["x"]), R.colsum_bound(c["x"])
        plain = ops.colsum(x)
        acc = dev(c["out0"])
        ops.colsum(x, out=acc, accumulate=True)
        buf = torch.full((N + 9,), 1234.5, device=DEV)
        ops.colsum(x, out=buf[1:1 + N])
        torch.cuda.synchronize()
        assert buf.data_ptr() % 16 == 0 and float(buf[0]) == 1234.5 and bool((buf[1 + N:] == 1234.5).all())
        e1, e3 = np.abs(host(plain) - want), np.abs(host(buf[1:1 + N]) - want)
        e2 = np.abs(host(acc) - R.colsum_f64(c["x"], c["out0"], True))
        b2 = R.colsum_bound(c["x"], c["out0"])
        print(f"[colsum {dtype} {M}x{N}] worst error / bound: plain {np.max(e1 / bound):.3f}, accumulate {np.max(e2 / b2):.3f}, unaligned out {np.max(e3 / bound):.3f}")
        assert (e1 <= bound).all() and (e2 <= b2).all() and (e3 <= bound).all(), (M, N)
        assert e1.max() <= 1e-5 * max(1.0, np.abs(want).max())          # (and never looser than test_colsum's bound)
        if M <= 3 * 64:                                                  # up to three chunks both reduce kernels add in the same order
            assert same_bits(buf[1:1 + N], plain), (M, N)


# ---------------------------------------------------------------------------------------------- small-K weight gradient
@pytest.mark.parametrize("M", R.SMALLK_M)
@pytest.mark.parametrize("K", R.SMALLK_K)
def test_smallk_wgrad_vs_float64(K, M):
    """strided dy (ld N + 3, column offset 2) and x (ld K + 4, column offset 1), accumulate 0 and 1; per element
    |err| <= eps32 (the colsum chain) sum_m |dy x| (+ |dW| before)"""
    _p, _stream = _ps()
    for N in R.SMALLK_N:
        c = R.smallk_case(M, N, K)
        dy, x = dev(c["dyb"])[:, 2:2 + N], dev(c["xb"])[:, 1:1 + K]
        ws = torch.empty(64 * N * K, device=DEV)
        for accumulate in (0, 1):
            dw = dev(c["dw0"]) if accumulate else torch.full((N, K), float("nan"), device=DEV)
            call("hamt_smallk_wgrad", M, N, K, _p(dy), N + 3, _p(x), K + 4, _p(dw), accumulate, _p(ws), _stream())
            want = R.smallk_wgrad_f64(c["dy"], c["x"], c["dw0"], bool(accumulate))
            bound = R.smallk_bound(c["dy"], c["x"], c["dw0"] if accumulate else None)
            err = np.abs(host(dw) - want)
            print(f"[smallk_wgrad M {M} N {N} K {K} accumulate {accumulate}] worst error / bound {np.nanmax(err / bound):.3f}")
            assert (err <= bound).all(), (M, N, K, accumulate)


def test_linear_with_a_4_wide_input_takes_the_smallk_wgrad():
    from test_gpu_model import _CountCalls
    ops = _ops()
    c = R.smallk_case(65, 65, 4)
    x = dev(c["x"])
    w = dev(c["dw0"]).requires_grad_(True)
    b = torch.zeros(65, device=DEV, requires_grad=True)
    with _CountCalls("hamt_smallk_wgrad") as cnt:
        y = ops.linear(x, w, b, prec="fp32")
        y.backward(dev(c["dy"]))
        torch.cuda.synchronize()
    assert cnt.n["hamt_smallk_wgrad"] == 1
    assert (np.abs(host(w.grad) - R.smallk_wgrad_f64(c["dy"], c["x"])) <= R.smallk_bound(c["dy"], c["x"])).all()
    assert (np.abs(host(b.grad) - R.colsum_f64(c["dy"])) <= R.colsum_bound(c["dy"])).all()


# ---------------------------------------------------------------------------------------------- activation gradients
@pytest.mark.parametrize("n", R.ACT_SIZES)
def test_act_bwd(n):
    """GELU': within 8 x the fp32 restatement's own error of the float64 value (units of eps32 |g|); ReLU': g where h > 0, else +0, bit
    for bit (h = +-0.0 and +-1e-20 included).  n = 4 (2048 * 256) + 4 takes a second pass of the capped grid."""
    _p, _stream = _ps()
    h, g = R.act_case(n)
    hd, gd = dev(h), dev(g)
    dx = torch.full((n,), float("nan"), device=DEV)
    call("hamt_act_bwd", n, _p(gd), _p(hd), 1, _p(dx), _stream())
    e = R.dgelu_errors(h, g, host(dx))
    print(f"[act_bwd gelu n {n}] worst {np.nanmax(e):.3f} eps32 |g| at h = {h[int(np.nanargmax(e))]} (bound {R.DGELU_BOUND})")
    assert not np.isnan(e).any() and (e <= R.DGELU_BOUND).all()
    dx.fill_(float("nan"))
    call("hamt_act_bwd", n, _p(gd), _p(hd), 2, _p(dx), _stream())
    assert same_bits(dx, R.drelu(h, g))


def test_relu_backward_through_linear():
    """LinearFn hands hamt_act_bwd the ReLU OUTPUT: the gradient passes where the output is > 0"""
    ops = _ops()
    rng = np.random.Generator(np.random.PCG64(3))
    x, w = rng.standard_normal((9, 8)).astype(np.float32), rng.standard_normal((12, 8)).astype(np.float32)
    go = rng.standard_normal((9, 12)).astype(np.float32)
    xd = dev(x).requires_grad_(True)
    y = ops.linear(xd, dev(w), None, act=ops.ACT_RELU, prec="fp32")
    y.backward(dev(go))
    torch.cuda.synchronize()
    pre = x.astype(np.float64) @ w.astype(np.float64).T
    sure = np.abs(pre) > 1e-4
    assert ((host(y) > 0) == (pre > 0))[sure].all()
    want = (go * (host(y) > 0)).astype(np.float64) @ w
    assert np.abs(host(xd.grad) - want).max() <= 2e-5 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------- dropout
@pytest.fixture
def rng_state():
    """the device RNG words and the call counter as they were, put back afterwards"""
    ops = _ops()
    st, cnt = ops.rng_state(DEV).clone(), ops._call_counter[0]
    yield ops
    ops.rng_state(DEV).copy_(st)
    ops._call_counter[0] = cnt
    torch.cuda.synchronize()


def _dropout_case(n, seed=70):
    rng = np.random.Generator(np.random.PCG64(seed))
    x, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    x[:4] = (0.0, -0.0, 1e-30, -3.0)
    return x, g


@pytest.mark.parametrize("n", [1000, 1 << 20, 2048 * 256 + 7])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_fn_is_the_restated_mask_forward_and_backward(rng_state, p, n):
    """DropoutFn with (seed 1234, epoch 0, call id CALL_ID): y = x * factor and dx = g * factor bit for bit, factor = fp32 1 / (1 - p)
    where the restated 24-bit draw is >= p, else 0 (element TIE_INDEX of the larger launches draws exactly 0.5)"""
    ops = rng_state
    x, g = _dropout_case(n)
    ops.manual_seed(R.SEED)
    ops._call_counter[0] = R.CALL_ID - 1
    xg = dev(x).requires_grad_(True)
    y = ops.DropoutFn.apply(xg, p)
    assert ops._call_counter[0] == R.CALL_ID
    ops._call_counter[0] = 12345                                          # the backward replays the forward's call id, not the counter
    (dx,) = torch.autograd.grad(y, xg, dev(g))
    torch.cuda.synchronize()
    f = R.drop_scale(R.rng_key(R.SEED, 0, R.CALL_ID), n, p)
    assert 0 < (f == 0).sum() < n
    assert same_bits(y, x * f), int((bits32(y) != bits32(x * f)).sum())
    assert same_bits(dx, g * f)


def test_dropout_factor_depends_on_the_element_not_on_the_launch(rng_state):
    ops = rng_state
    _p, _stream = _ps()
    ops.manual_seed(R.SEED)
    st = ops.rng_state(DEV)
    x, _ = _dropout_case(1 << 20)
    xd = dev(x)
    big, small, ident = torch.empty_like(xd), torch.empty(1000, device=DEV), torch.empty_like(xd)
    call("hamt_dropout", 1 << 20, _p(xd), _p(big), 0.5, R.CALL_ID, _p(st), _stream())
    call("hamt_dropout", 1000, _p(xd), _p(small), 0.5, R.CALL_ID, _p(st), _stream())
    assert same_bits(big[:1000], small)
    call("hamt_dropout", 1 << 20, _p(xd), _p(ident), 0.0, R.CALL_ID, _p(st), _stream())
    assert same_bits(ident, x)                                            # p = 0: the identity


def test_dropout_follows_the_epoch_and_the_call_id(rng_state):
    ops = rng_state
    n, p = 4099, 0.3
    x, _ = _dropout_case(n)
    ops.manual_seed(R.SEED)
    outs = {}
    for epoch, cid in ((0, 77), (0, 78), (1, 77), (2, 77)):
        while int(ops.rng_state(DEV)[1]) < epoch:
            ops.advance_rng_epoch(DEV)
        ops._call_counter[0] = cid - 1
        outs[epoch, cid] = y = ops.DropoutFn.apply(dev(x), p)
        torch.cuda.synchronize()
        assert same_bits(y, x * R.drop_scale(R.rng_key(R.SEED, epoch, cid), n, p)), (epoch, cid)
    assert len({bits32(y).tobytes() for y in outs.values()}) == 4


@pytest.mark.parametrize("Rr,Cc,p", [(77, 104, 0.1), (300, 768, 0.5)])
def test_cast_pad_bf16_dropout(rng_state, Rr, Cc, p):
    """bf16(x * factor) with the restated (row, group-of-4) mask of drop_scale4, zero padding rows, and the same bytes from an input
    that starts one float into its buffer (the scalar load branch)"""
    ops = rng_state
    rng = np.random.Generator(np.random.PCG64(80 + Rr))
    x = rng.standard_normal((Rr, Cc)).astype(np.float32)
    ops.manual_seed(R.SEED)
    y = ops.cast_pad16_dropout(dev(x), p, 77)
    flat = torch.zeros(Rr * Cc + 1, device=DEV)
    shifted = flat[1:].view(Rr, Cc)
    shifted.copy_(dev(x))
    assert shifted.data_ptr() % 16 == 4
    y2 = ops.cast_pad16_dropout(shifted, p, 77)
    torch.cuda.synchronize()
    assert y.shape[0] > Rr and y.shape == (-(-Rr // 64) * 64, Cc) and y.dtype == torch.bfloat16
    f = R.drop_scale4(R.rng_key(R.SEED, 0, 77), Rr, Cc, p)
    assert 0 < (f == 0).sum() < f.size
    got = bits16(y)
    assert np.array_equal(got[:Rr], R.bf16_bits(x * f)), int((got[:Rr] != R.bf16_bits(x * f)).sum())
    assert not got[Rr:].any()
    assert np.array_equal(bits16(y2), got)


# ---------------------------------------------------------------------------------------------- exact one-liners
@pytest.mark.parametrize("n", [5, 1024 * 256 + 3])
def test_extend_mask(n):
    _p, _stream = _ps()
    m = np.resize(np.array([0, 1, 2, 255, 0, 0, 1], dtype=np.uint8), n)
    out = torch.full((n,), float("nan"), device=DEV)
    call("hamt_extend_mask", n, _p(dev(m)), _p(out), _stream())
    assert same_bits(out, R.extend_mask32(m))
    b = (m != 0).reshape(1, n)
    got = _ops().extend_mask(dev(b))
    torch.cuda.synchronize()
    assert got.shape == (1, 1, 1, n) and same_bits(got.reshape(-1), R.extend_mask32(b.reshape(-1)))


@pytest.mark.parametrize("n", list(range(1, 18)) + [4099])
def test_cast_f32_bf16(n):
    """round to nearest even (ties both ways), +-inf, +-0, subnormals; NaN stays NaN"""
    x = R.cast_case(n)
    y = _ops().cast_bf16(dev(x))
    torch.cuda.synchronize()
    got, want = bits16(y), R.bf16_bits(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan]), (x[~nan][got[~nan] != want[~nan]], got[~nan][got[~nan] != want[~nan]])
    assert np.isnan(R.bf16_value(got[nan])).all()


@pytest.mark.parametrize("B,S,H", [(1, 1, 4), (5, 36, 768), (67, 3, 12)])
def test_mean_mid(B, S, H):
    ops = _ops()
    rng = np.random.Generator(np.random.PCG64(90 + B))
    x, go = rng.standard_normal((B, S, H)).astype(np.float32), rng.standard_normal((B, H)).astype(np.float32)
    xg = dev(x).requires_grad_(True)
    y = ops.mean_mid(xg)
    (dx,) = torch.autograd.grad(y, xg, dev(go))
    torch.cuda.synchronize()
    x64 = x.astype(np.float64)
    assert (np.abs(host(y) - x64.mean(axis=1)) <= R.EPS32 * (S + 1) * np.abs(x64).sum(axis=1) / S).all()
    assert same_bits(dx, np.broadcast_to(R.mean_mid_bwd32(go, S)[:, None, :], (B, S, H)))


@pytest.mark.parametrize("B,S,H,how", [(3, 1, 4, "cls"), (5, 36, 128, "cls"), (5, 36, 128, "stride_h_plus_2"), (4, 1, 12, "stride_h_plus_2")])
def test_mul_bcast(B, S, H, how):
    """c = t[:, 0] of a (B, 7, H) tensor (row stride 7 H) / a c whose row stride H + 2 is no multiple of 4 (the .contiguous() branch):
    y and da are one product each, bit for bit; dc[b] = sum_s dy a within eps32 (S + 1) sum|dy a|"""
    ops = _ops()
    rng = np.random.Generator(np.random.PCG64(100 + B + S))
    a, go = rng.standard_normal((B, S, H)).astype(np.float32), rng.standard_normal((B, S, H)).astype(np.float32)
    t = rng.standard_normal((B, 7, H) if how == "cls" else (B, H + 2)).astype(np.float32)
    tg = dev(t).requires_grad_(True)
    cv, c = (tg[:, 0], t[:, 0]) if how == "cls" else (tg[:, :H], t[:, :H])
    assert cv.stride(0) == (7 * H if how == "cls" else H + 2)
    ag = dev(a).requires_grad_(True)
    y = ops.mul_bcast(ag, cv)
    da, dt = torch.autograd.grad(y, (ag, tg), dev(go))
    torch.cuda.synchronize()
    assert same_bits(y, a * c[:, None, :]) and same_bits(da, go * c[:, None, :])
    dc = host(dt)[:, 0] if how == "cls" else host(dt)[:, :H]
    rest = host(dt)[:, 1:] if how == "cls" else host(dt)[:, H:]
    prod = go.astype(np.float64) * a
    assert (np.abs(dc - prod.sum(axis=1)) <= R.EPS32 * (S + 1) * np.abs(prod).sum(axis=1)).all()
    assert not rest.any()


def test_add3_and_fill_where_zero():
    ops = _ops()
    rng = np.random.Generator(np.random.PCG64(110))
    a, b, c = (rng.standard_normal((5, 36, 128)).astype(np.float32) for _ in range(3))
    assert same_bits(ops.add3(dev(a), dev(b), dev(c)), R.add3_32(a, b, c))
    assert same_bits(ops.add3(dev(a), dev(b)), R.add3_32(a, b))
    n = 2048 * 256 + 1                                                    # one element into the second pass of the capped grid
    x, flag = rng.standard_normal(n).astype(np.float32), (rng.random(n) > 0.5).astype(np.int64)
    flag[-1] = 0
    xg = dev(x).requires_grad_(True)
    f = ops.fill_where_zero(xg, dev(flag), -float("inf"))
    (dx,) = torch.autograd.grad(f, xg, dev(x))
    torch.cuda.synchronize()
    assert same_bits(f, np.where(flag == 0, np.float32(-np.inf), x)) and same_bits(dx, np.where(flag == 0, np.float32(0), x))


@pytest.mark.parametrize("B,S,H", [(3, 5, 130), (64, 16, 768), (2, 7, 4)])
def test_sum_rows_adds_to_out_in_both_modes(B, S, H):
    """hamt_sum_rows ADDS to `out` (include/hamt.h): mode 0 out[H] += sum over (b, s), mode 1 out[S, H] += sum over b.  Bound per element:
    eps32 (longest chain of additions) (sum|x| + |out|), the chain = rows per chunk + chunks + 2 in mode 0, B + 1 in mode 1."""
    _p, _stream = _ps()
    rng = np.random.Generator(np.random.PCG64(120 + B))
    x = rng.standard_normal((B, S, H)).astype(np.float32)
    xd = dev(x)
    rows = B * S
    chunks = 64 if rows >= 64 * 16 else max(1, (rows + 15) // 16)
    rpc = -(-rows // chunks)
    for mode, shape, axes, chain in ((0, (H,), (0, 1), rpc + chunks + 2), (1, (S, H), (0,), B + 1)):
        out0 = (2 + np.abs(rng.standard_normal(shape))).astype(np.float32)
        out, ws = dev(out0), torch.empty(64 * H, device=DEV)
        call("hamt_sum_rows", B, S, H, _p(xd), mode, _p(out), _p(ws), _stream())
        want = x.astype(np.float64).sum(axis=axes) + out0
        bound = R.EPS32 * chain * (np.abs(x.astype(np.float64)).sum(axis=axes) + np.abs(out0))
        assert (np.abs(host(out) - want) <= bound).all(), mode
        assert (np.abs(host(out) - (want - out0)) > bound).all(), mode          # (an overwriting kernel would land here)
