"""-m gpu: hamt_range_audit (csrc/audit.hip) against its numpy restatement (tests/_range_audit_ref.py), op level.  Every record must
match EXACTLY: the kernel counts and takes an integer maximum, there is no rounding to allow for.

Every operand sits inside a larger allocation whose other elements -- in front, behind, in the ld - N gap columns -- are NaN, inf and
at-the-limit patterns (a read outside [M, N] changes the record: tests/test_range_audit_ref.py proves it per kind of error), and every
record starts from non-zero values (adding, not overwriting).  Shapes: the issue's six -- (1, 8), (3, 7) with ld 9, (5, 136) from a base
one element off alignment, (64, 128) contiguous, (257, 776) with ld 784, M = 0 -- plus ragged tails behind full vectors, and, because
(257, 776) is one pass of the kernel's 1024 x 256 lanes, (1031, 2059) with ld 2064, where lanes come round a second time."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _range_audit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


@functools.lru_cache(maxsize=1)
def _cases():
    """the cases and their expected records, computed once and shared (nothing below writes into them)"""
    cs = R.cases()
    return cs, {k: R.fold(v) for k, v in cs.items()}


def _operand(call):
    """(the whole allocation on the device, the [M, N] view of x inside it)"""
    raw = call["buf"]
    host = torch.from_numpy(raw.view(np.int16 if raw.dtype == np.uint16 else np.int32).copy())
    buf = host.to(DEV).view(TORCH_DT[call["fmt"]])
    assert buf.data_ptr() % 16 == 0
    x = torch.as_strided(buf, (call["M"], call["N"]), (call["ld"], 1), call["off"])
    return buf, x


def _rec0():
    return torch.tensor(R.REC0, dtype=torch.int64, device=DEV)


CASE_NAMES = [f"{f}/{s[0]}" for f in R.FMT for s in R.SHAPES] + [f"{f}/two_calls" for f in R.FMT]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_record_matches_restatement(name):
    from vln_hamt_amd import ops
    cs, want = _cases()
    rec = _rec0()
    keep = []
    for call in cs[name]:
        buf, x = _operand(call)
        keep.append(buf)
        if call["M"] > 0:
            assert (x.data_ptr() % 16 == 0) == (call["off"] % 8 == 0 if call["fmt"] != "f32" else call["off"] % 4 == 0)
        assert ops.range_audit(x, rec) is rec
    got = rec.cpu().tolist()
    print(f"[{name}] record {got} (largest finite |x| {R.bits_f32(got[2]):.6g})")
    assert got == want[name], (name, got, want[name])
    for call, buf in zip(cs[name], keep):       # the operand and its surroundings are read only
        raw = call["buf"]
        back = buf.view(torch.int16 if raw.dtype == np.uint16 else torch.int32).cpu().numpy().view(raw.dtype)
        assert np.array_equal(back, raw), name


def test_two_records_updated_alternately():
    """two operands, two records, calls interleaved a b a b: each record sees its own operand twice and nothing of the other"""
    from vln_hamt_amd import ops
    cs, _ = _cases()
    a, b = cs["f16/3x7_ld9"][0], cs["bf16/9x77_ld80"][0]
    table = torch.tensor([R.REC0, R.REC0], dtype=torch.int64, device=DEV)
    (ka, xa), (kb, xb) = _operand(a), _operand(b)
    for _ in range(2):
        ops.range_audit(xa, table[0])
        ops.range_audit(xb, table[1])
    got = table.cpu().tolist()
    assert got[0] == R.fold([a, a]) and got[1] == R.fold([b, b]), got


def test_argument_errors_leave_the_record_alone():
    from vln_hamt_amd import _lib as L
    lib = L.load()
    cs, _ = _cases()
    buf, x = _operand(cs["f16/64x128"][0])
    rec = _rec0()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, rp = C.c_void_p(x.data_ptr()), C.c_void_p(rec.data_ptr())
    bad = {
        "null x": (None, L.HAMT_F16, 64, 128, 128, rp),
        "null rec": (xp, L.HAMT_F16, 64, 128, 128, None),
        "dtype u8": (xp, L.HAMT_U8G, 64, 128, 128, rp),
        "dtype 7": (xp, 7, 64, 128, 128, rp),
        "N = 0": (xp, L.HAMT_F16, 64, 0, 128, rp),
        "N < 0": (xp, L.HAMT_F16, 64, -8, 128, rp),
        "ld < N": (xp, L.HAMT_F16, 64, 128, 127, rp),
        "M < 0": (xp, L.HAMT_F16, -1, 128, 128, rp),
    }
    for what, args in bad.items():
        rc = lib.hamt_range_audit(*args, st)
        assert rc == -1, (what, rc)                          # HAMT_ERR_ARG
        assert "hamt_range_audit" in L.last_error(), (what, L.last_error())
    torch.cuda.synchronize()
    assert rec.cpu().tolist() == list(R.REC0)


def test_op_refuses_what_the_kernel_cannot_take():
    from vln_hamt_amd import ops
    from vln_hamt_amd._lib import HamtError
    rec = _rec0()
    x = torch.zeros(4, 16, dtype=torch.float16, device=DEV)
    for t, r in ((x.t(), rec),                                               # inner stride 16
                 (x.to(torch.float64), rec), (x.view(-1), rec),              # dtype, rank
                 (x, rec.to(torch.int32)), (x, torch.zeros(8, dtype=torch.int64, device=DEV)[::2]), (x, rec.cpu())):
        with pytest.raises(HamtError):
            ops.range_audit(t, r)
    torch.cuda.synchronize()
    assert rec.cpu().tolist() == list(R.REC0)
