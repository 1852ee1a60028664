"""CPU: which kernel hamt_gemm runs a problem on (csrc/gemm_plan.h, asked through hamt_gemm_plan -- nothing is launched).

Two records pin it: the kernel names the GPU tests assert after real launches (tests/_gemm_cases.py), and a trimmed sweep of the
dispatch as it was before it became one function, in the default environment and under every dispatch switch
(tests/golden/gemm_plan_parent.txt; method in profiles/gemm_plan_refactor_parity.txt)."""
import os
import subprocess
import sys

import pytest

from _gemm_cases import (BENCH_GEMMS, EPI_OF, KG_GEMMS, ROOT, SPLITK_GEMMS, SPLITK_SWITCHES, plan_desc, plan_golden_rows, plan_mismatches,
                         splitk_mismatches)

ENVIRONMENTS = ["default", "HAMT_P8=0", "HAMT_P8=1", "HAMT_Q4=0", "HAMT_Q4=1", "HAMT_KG=1", "HAMT_KG=3223", "HAMT_KG=3232", "HAMT_KG=3224",
                "HAMT_KG=6423", "HAMT_KG=6432", "HAMT_KG=12822", "HAMT_KG=322", "HAMT_FAST_BM=32", "HAMT_FAST_BM=64", "HAMT_FAST_BM=128",
                "HAMT_FAST_BM=256", "HAMT_KS=4", "HAMT_P8_BN=192", "HAMT_P8_BN=256", "HAMT_NO_FAST=1"]
SWITCHES = sorted({e.split("=")[0] for e in ENVIRONMENTS[1:]})


def _lib():
    from vln_hamt_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert not any(s in os.environ for s in SWITCHES), "the dispatch switches are read once per process: run this file without them"
    return L


@pytest.mark.parametrize("layout,M,N,K,epi,cdt,kernel", [g for g in BENCH_GEMMS if g[6]], ids=[f"{s[0]}-{s[1]}x{s[2]}x{s[3]}-{s[4]}-{s[5]}" for s in BENCH_GEMMS if s[6]])
def test_plan_names_the_kernel_the_gpu_test_asserts(layout, M, N, K, epi, cdt, kernel):
    L = _lib()
    ks, name = L.gemm_plan(plan_desc(L.GemmDesc, layout, M, N, K, EPI_OF[epi], L.HAMT_F32 if cdt == "f32" else L.HAMT_BF16))
    assert (ks, name) == (1, kernel)


@pytest.mark.parametrize("layout,shape,variant", KG_GEMMS)
def test_plan_k_groups(layout, shape, variant):
    """the three calls of test_gemm_k_groups that assert a kernel: plain (the q4 tile takes it where the K-group tile would have 128 rows),
    bias + accumulate, aux multiply into a bf16 C"""
    L = _lib()
    plain = "gemm_q4_kernel" if variant.startswith("gemm_kg_kernel<128") else variant
    for e, dc, want in ((0, L.HAMT_F32, plain), (L.EPI_BIAS | L.EPI_ACCUM, L.HAMT_F32, variant), (L.EPI_MUL_AUX, L.HAMT_BF16, variant)):
        ks, name = L.gemm_plan(plan_desc(L.GemmDesc, layout, *shape, e, dc))
        assert ks == 1 and name.startswith(want), (e, ks, name)


def test_plan_rejects_bad_arguments():
    L = _lib()
    assert L.load().hamt_gemm_plan(None, 0, None, 0) < 0
    d = plan_desc(L.GemmDesc, "nt", 512, 2048, 8192, 0, L.HAMT_F32)
    assert L.load().hamt_gemm_plan(d, 0, None, 0) == 1                  # no name wanted; no workspace, no split
    assert L.gemm_plan(d)[0] == L.load().hamt_gemm_ksplit(d) > 1       # as much workspace as it asks for


def test_golden_record_is_what_it_claims():
    rows = plan_golden_rows()
    assert 0 < len(rows) <= 8000
    assert {r[0] for r in rows} == set(ENVIRONMENTS)
    # every tile height of gemm_fast_kernel that splits does so in the record (32 rows: only under HAMT_FAST_BM=32)
    assert {r[9].split("<")[1].split(",")[0] for r in rows if r[8] > 1} == {"32", "64", "128"}
    assert all(r[9].startswith("gemm_fast_kernel<") for r in rows if r[8] > 1)
    # a generic kernel never splits: rows it ran with a workspace sized for > 1 slices before, in every environment
    generic_ws = [r for r in rows if r[9].startswith(("gemm_bf16_kernel", "gemm_f32_kernel")) and r[7] > 1]
    assert {r[0] for r in generic_ws} == set(ENVIRONMENTS)
    assert all(r[8] == 1 for r in generic_ws)
    assert all(r[7] == r[8] for r in set(rows) - set(generic_ws))


def test_golden_default_environment():
    L = _lib()
    rows = [r for r in plan_golden_rows() if r[0] == "default"]
    bad = plan_mismatches(lambda d, ws_bytes: L.gemm_plan(d, ws_bytes), L.GemmDesc, rows)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("setting", ENVIRONMENTS[1:])
def test_golden_under_switch(setting):
    """one child process per setting (the switches are read once per process); it loads the library with ctypes alone"""
    _lib()
    k, v = setting.split("=")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_gemm_cases.py"), setting], env={**os.environ, k: v}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_splitk_cases_split_as_recorded():
    """SPLITK_GEMMS (the problems test_gpu_splitk.py launches): slices and kernel, with the workspace each row offers.  The rows of the
    default environment in this process, the rows under a switch in one child per switch."""
    L = _lib()
    assert {r[0] for r in SPLITK_GEMMS} == {None, *SPLITK_SWITCHES}
    rows = [r for r in SPLITK_GEMMS if r[0] is None]
    bad = splitk_mismatches(lambda d, ws_bytes: L.gemm_plan(d, ws_bytes), lambda d: L.load().hamt_gemm_ksplit(d), L.GemmDesc, rows, L.HAMT_F32)
    assert not bad, bad
    assert all(r[8].startswith("gemm_fast_kernel<64, ") for r in rows)      # no 128-row tile splits by itself
    for setting in SPLITK_SWITCHES:
        k, v = setting.split("=")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_gemm_cases.py"), setting, "splitk"], env={**os.environ, k: v}, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
