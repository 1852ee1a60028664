"""-m gpu: the packed attention entry points (hamt_attn_varlen_*, hamt_attn_varlen_cross_*) with 129 .. 256 tokens on a side, on the cases
of tests/_attn_long_ref.py through test_gpu_attn.py's run_case / check: out, lse, dq, dk, dv against the float64 statement per output row
within 8 x the committed caps, NaN guard rows and padding columns around every buffer, the untouched key rows no query sequence names.
The forward is attn_s128_fwd_kernel (two chunks of 128 queries, KB up to 16), the backward the PACKED form of attn_wide_bwd_kernel:

  self    lens 1, 129, 0, 250, 256, 144, 17, 128 (descriptor 256, p 0.1);  lens 250, 1, 0, 129, 177, 64 (descriptor 250, bf16 in / out)
  cu_q    Sq <= 250 on 70 keys, pair + fillers (p 0.1);  Sq <= 128 on 140 keys, fillers behind n_pairs (p 0.1, bf16 in / out)
  cu_k    70 queries on lens_k 3, 250, 0, 129, 17, pair + a filler + an empty key side (p 0.1);  200 queries on 256, 1, 130 (p 0.5, bf16 io)

tests/test_attn_long_ref.py shows on the CPU that these cases tell a wrong kernel from a right one."""
import numpy as np
import pytest
import torch

import _attn_long_ref as LR
import _attn_ref as R
from test_gpu_attn import _lib, check, rng_state, run_case  # noqa: F401  (rng_state: the autouse fixture, here as there)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(LR.cases()))
def test_long_case_against_float64(name):
    c = LR.cases()[name]
    got, bad = run_case(c)
    assert _lib().last_kernel() == LR.bwd_kernel(c) == "attn_wide_bwd_kernel<packed>"
    with LR.long_caps():
        check(c, got, bad)


def test_a_short_packed_call_stays_on_the_s128_backward():
    c = LR.short_case()
    assert max(c["Sq"], c["Sk"]) <= 128 and c["form"] != "pad"
    got, bad = run_case(c)
    assert _lib().last_kernel() == LR.bwd_kernel(c) == "attn_s128_bwd_kernel"
    check(c, got, bad)


def test_two_runs_agree_bit_for_bit():
    """no atomics, no accumulation through memory: forward and backward of a case with dropout, fillers and a shared key buffer twice"""
    c = LR.cases()["long self 256 p 0.1"]
    a, bad_a = run_case(c)
    b, bad_b = run_case(c)
    assert not bad_a and not bad_b
    for name in R.OUTPUTS:
        assert np.array_equal(np.ascontiguousarray(a[name]).view(np.int32), np.ascontiguousarray(b[name]).view(np.int32)), name


def test_nan_in_the_neighbouring_sequence_stays_there():
    """q, k, v and dO of the middle sequence (250 rows) are NaN: sequences 0 (130 rows) and 2 (37 rows) hold no NaN and meet float64"""
    c = LR.nan_case()
    got, bad = run_case(c, poison_b=1)
    for b in (0, 2):
        rq, rk = slice(c["cuq"][b], c["cuq"][b + 1]), slice(c["cuk"][b], c["cuk"][b + 1])
        for nm, r in (("out", rq), ("dq", rq), ("dk", rk), ("dv", rk)):
            assert np.isfinite(got[nm][r]).all(), (nm, b)
        assert np.isfinite(got["lse"][b]).all(), ("lse", b)
    with LR.long_caps():
        check(c, got, bad, skip_b=(1,))


@pytest.mark.parametrize("form", ("vself", "vq", "vk"))
def test_descriptor_257_is_refused(form):
    """above 256 tokens the entry points refuse and launch nothing: the output buffers keep their NaN"""
    L = _lib()
    kw = dict(vself=dict(lens_q=(5, 3, 2)), vq=dict(lens_q=(5, 3, 2), n_pairs=3), vk=dict(lens_k=(5, 3, 2)))[form]
    Sq, Sk = (257, 257) if form == "vself" else ((257, 16) if form == "vq" else (16, 257))
    c = R.make_case("refused " + form, "bf16", Sq, Sk, form=form, seed=795, **kw)
    with pytest.raises(L.HamtError, match="256"):
        run_case(c)
    torch.cuda.synchronize()
