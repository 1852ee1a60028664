"""-m gpu: the loss kernels of csrc/loss.hip at op level, through ops.cross_entropy, ops.kl_div_logsoftmax and ops.mse_loss, forward and
backward, against the float64 restatement of tests/_smallops_ref.py.  Every error is scaled per ROW (eps32 max(1, |lse|, max finite |x|),
times |g_r| for the gradient), never per tensor: a wrong row with a small upstream weight cannot hide behind a row with a large one.
tests/test_smallops_ref.py shows on the CPU that fp32 arithmetic in the kernel's order stays 8 x inside the bounds on these cases and
that a missing max subtraction, dropped tail columns, a dropped wave, a wrong row stride, a shifted label, a gradient on an ignored row,
a KL gradient without sum(t) and a NaN for 0 log 0 each exceed them tenfold."""
import numpy as np
import pytest
import torch

import _smallops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vln_hamt_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(host(got)).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


def _ce_input(c):
    """the logits of a case on the device, in the memory layout the case names"""
    ops = _ops()
    if c["layout"] == "view":
        x = dev(c["buf"])[:, :c["C"]]
    elif c["layout"] == "empty_rows":
        x = ops.empty_rows(c["R"], c["C"], DEV)
        x.copy_(dev(c["x"]))
    else:
        x = dev(c["x"].T).t()
        assert x.stride(1) != 1 or c["R"] == 1
    assert x.shape == (c["R"], c["C"]) and (c["layout"] == "colstride" or c["R"] == 1 or x.stride(0) == c["ld"])
    return x.detach().requires_grad_(True)


@pytest.mark.parametrize("i", range(len(R.ce_cases())), ids=[c["name"].replace(" ", "_") for c in R.ce_cases()])
def test_cross_entropy_vs_float64_per_row(i):
    c = R.ce_cases()[i]
    xg = _ce_input(c)
    loss = _ops().cross_entropy(xg, dev(c["label"]))
    (dx,) = torch.autograd.grad(loss, xg, dev(c["g"]))
    torch.cuda.synchronize()
    assert loss.shape == (c["R"],) and dx.shape == (c["R"], c["C"])
    assert dx.stride(1) == 1 and (c["R"] == 1 or dx.stride(0) % 8 == 0), dx.stride()      # rows 32-byte aligned for the GEMMs behind it
    el, et = R.ce_errors(c, host(loss), host(dx))
    print(f"[ce {c['name']}] loss: worst row {el.max():.3f} units (bound {R.CE_LOSS_BOUND}); dx / g: worst row {et.max():.3f} units (bound {R.CE_TERM_BOUND})")
    assert (el <= R.CE_LOSS_BOUND).all(), (c["name"], "loss", int(el.argmax()), c["kinds"][int(el.argmax())], el.max())
    assert (et <= R.CE_TERM_BOUND).all(), (c["name"], "dx", int(et.argmax()), c["kinds"][int(et.argmax())], et.max())


@pytest.mark.parametrize("how", ["empty", "slice"])
def test_cross_entropy_of_no_rows(how):
    """R = 0 (a batch without a masked token): an empty loss, an empty gradient, no error -- for an empty tensor of its own (torch hands
    out a null pointer for it) and for an empty slice of a live one"""
    x = torch.empty(0, 37, device=DEV) if how == "empty" else torch.zeros(4, 37, device=DEV)[:0]
    xg = x.detach().requires_grad_(True)
    loss = _ops().cross_entropy(xg, torch.empty(0, dtype=torch.int64, device=DEV))
    (dx,) = torch.autograd.grad(loss, xg, torch.empty(0, device=DEV))
    torch.cuda.synchronize()
    assert loss.shape == (0,) and dx.shape == (0, 37)


@pytest.mark.parametrize("i", range(len(R.kl_cases())), ids=[c["name"].replace(" ", "_") for c in R.kl_cases()])
def test_kl_vs_float64_per_row(i):
    c = R.kl_cases()[i]
    xg = dev(c["x"]).requires_grad_(True)
    t = dev(c["t"])
    assert t.dtype == (torch.float64 if c["t"].dtype == np.float64 else torch.float32)
    loss = _ops().kl_div_logsoftmax(xg, t)
    (dx,) = torch.autograd.grad(loss, xg, dev(c["g"]))
    torch.cuda.synchronize()
    assert loss.shape == (c["R"],) and dx.shape == (c["R"], c["C"]) and (c["R"] == 1 or dx.stride(0) % 8 == 0)
    el, et = R.kl_errors(c, host(loss), host(dx))
    print(f"[kl {c['name']}] loss: worst row {el.max():.3f} units (bound {R.KL_LOSS_BOUND}); dx / g: worst row {et.max():.3f} units (bound {R.KL_TERM_BOUND})")
    assert (el <= R.KL_LOSS_BOUND).all(), (c["name"], "loss", int(el.argmax()), c["kinds"][int(el.argmax())], el.max())
    assert (et <= R.KL_TERM_BOUND).all(), (c["name"], "dx", int(et.argmax()), c["kinds"][int(et.argmax())], et.max())


@pytest.mark.parametrize("n", R.MSE_SIZES)
def test_mse_is_the_fp32_statement_bit_for_bit(n):
    """d * d and (2 g) (x - t), each operation rounded once; n = 2048 * 256 + 5 takes a second pass of the capped grid"""
    x, t, g = R.mse_case(n)
    xg = dev(x).requires_grad_(True)
    loss = _ops().mse_loss(xg, dev(t))
    (dx,) = torch.autograd.grad(loss, xg, dev(g))
    torch.cuda.synchronize()
    assert same_bits(loss, R.mse32(x, t)) and same_bits(dx, R.mse_bwd32(x, t, g))


def test_mse_bf16_target():
    x, t, g = R.mse_case(257)
    bits = R.bf16_bits(t)
    t16 = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).to(DEV)
    xg = dev(x.reshape(1, 257)).requires_grad_(True)
    loss = _ops().mse_loss(xg, t16.reshape(1, 257))
    (dx,) = torch.autograd.grad(loss, xg, dev(g.reshape(1, 257)))
    torch.cuda.synchronize()
    tv = R.bf16_value(bits)
    assert (tv != t).any()
    assert same_bits(loss.reshape(-1), R.mse32(x, tv)) and same_bits(dx.reshape(-1), R.mse_bwd32(x, tv, g))
