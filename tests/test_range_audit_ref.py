"""CPU: the numpy restatement of hamt_range_audit's record (tests/_range_audit_ref.py) and the cases of tests/test_gpu_range_audit.py --
hand-checked small records, and the proof that the cases are sensitive: every deliberate error in FAULTS changes the expected record of
at least one case, so a kernel that makes it cannot pass the GPU test."""
import functools

import numpy as np
import pytest

import _range_audit_ref as R


@functools.lru_cache(maxsize=1)
def _cases():
    return R.cases()


def test_hand_checked_record_half():
    # x = [[-65504, 65472, +inf, NaN, -0, subnormal, -inf, 65504]]: two at the limit, three non-finite, largest finite 65504
    call = R.make_call("f16", 1, 8)
    assert call["buf"][R.PAD:R.PAD + 8].tolist() == [0xFBFF, 0x7BFE, 0x7C00, 0x7E01, 0x8000, 0x0001, 0xFC00, 0x7BFF]
    assert R.audit_record(call, [0, 0, 0, 0]) == [2, 3, R.f32_bits(65504.0), 1]
    assert R.audit_record(call, list(R.REC0)) == [5, 8, R.f32_bits(65504.0), 8]
    # a record that already holds a larger maximum keeps it
    assert R.audit_record(call, [0, 0, R.f32_bits(1e6), 0])[2] == R.f32_bits(1e6)


def test_hand_checked_record_other_formats():
    for fmt in ("bf16", "f32"):
        call = R.make_call(fmt, 1, 8)
        rec = R.audit_record(call, [0, 0, 0, 0])
        assert rec[0] == 0 and rec[1] == 3 and rec[3] == 1, (fmt, rec)        # nothing is "at the limit" outside half
    assert R.audit_record(R.make_call("bf16", 1, 8), [0, 0, 0, 0])[2] == 0x7C00 << 16
    assert R.audit_record(R.make_call("f32", 1, 8), [0, 0, 0, 0])[2] == R.f32_bits(70000.0)


def test_widening_is_exact():
    assert R.widen("f16", 0x7BFF) == R.f32_bits(65504.0)
    assert R.widen("f16", 0x0001) == R.f32_bits(2.0 ** -24)              # the smallest half subnormal is a normal float32
    assert R.widen("f16", 0x3C00) == R.f32_bits(1.0)
    assert R.widen("bf16", 0x3F80) == R.f32_bits(1.0)
    assert R.widen("f32", 0x12345678) == 0x12345678
    assert R.encode("bf16", np.array([1.0, 65504.0], dtype=np.float32)).tolist() == [0x3F80, 0x4780]     # 65504 rounds to 65536 in bf16


def test_no_rows_still_counts_the_call():
    for fmt in R.FMT:
        assert R.fold(_cases()[f"{fmt}/0x8"]) == [R.REC0[0], R.REC0[1], R.REC0[2], R.REC0[3] + 1]


def _units(fmt, M, N):
    """units of work of the kernel's vector path: N // V vectors and one ragged tail per row (csrc/audit.hip)"""
    V = R.FMT[fmt][4]
    return M * (N // V + (1 if N % V else 0))


def test_the_large_case_takes_more_than_one_grid_stride_pass():
    shapes = {s[0]: s for s in R.SHAPES}
    _, M, N, ld, off = shapes["1031x2059_ld2064"]
    for fmt in R.FMT:
        es = 2 if fmt != "f32" else 4
        assert (ld * es) % 16 == 0 and (off * es) % 16 == 0 and N % R.FMT[fmt][4] != 0          # aligned rows, a ragged tail: the vector path
        assert _units(fmt, M, N) > R.GRID_LANES, (fmt, _units(fmt, M, N))
    _, M, N, _, _ = shapes["257x776_ld784"]
    assert all(_units(fmt, M, N) < R.GRID_LANES for fmt in R.FMT)                                # (the issue's largest shape is one pass)


def test_every_case_adds_to_the_preloaded_record():
    for name, calls in _cases().items():
        rec = R.fold(calls)
        assert rec[3] == R.REC0[3] + len(calls), name
        assert rec[0] >= R.REC0[0] and rec[1] >= R.REC0[1] and rec[2] >= R.REC0[2], name
        if calls[0]["M"] > 0:
            assert rec[1] > R.REC0[1] and rec[2] > R.REC0[2], name          # every operand holds non-finite values and a large finite one
            assert (rec[0] > R.REC0[0]) == name.startswith("f16/"), name


def test_poison_surrounds_every_operand():
    """the element in front of x, the gap columns and the row behind x are NaN / inf / at-the-limit patterns"""
    for name, calls in _cases().items():
        for c in calls:
            _, mask, inf, limit, _ = R.FMT[c["fmt"]]
            keep = np.zeros(c["buf"].size, dtype=bool)
            idx = c["off"] + np.arange(c["M"])[:, None] * c["ld"] + np.arange(c["N"])[None, :]
            keep[idx.reshape(-1)] = True
            out = c["buf"][~keep].astype(np.uint64) & mask
            assert out.size >= 2 * R.PAD and bool(np.all(out >= (inf if limit is None else limit) - (1 if limit is None else 0))), name


@pytest.mark.parametrize("fault", R.FAULTS)
def test_cases_are_sensitive_to(fault):
    changed = [name for name, calls in _cases().items() if R.fold(calls, fault=fault) != R.fold(calls)]
    print(f"{fault}: changes {len(changed)} of {len(_cases())} cases")
    assert changed, fault
    if fault in ("read_col_N", "read_row_M", "nonfinite_in_max", "zero_exp_nonfinite", "drop_tail"):
        assert {n.split("/")[0] for n in changed} == set(R.FMT), (fault, changed)      # ... in all three formats
    if fault == "replace_max":
        assert len([n for n in changed if n.endswith("two_calls")]) == 3, changed


def test_ops_range_audit_refuses_cpu_tensors():
    import torch
    from vln_hamt_amd import ops
    from vln_hamt_amd._lib import HamtError
    with pytest.raises(HamtError):
        ops.range_audit(torch.zeros(4, 8, dtype=torch.float16), torch.zeros(4, dtype=torch.int64))
