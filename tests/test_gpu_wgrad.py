"""-m gpu: what the grouped weight-gradient launch computes -- hamt_wgrad_grouped / hamt_wgrad_grouped_ex (csrc/gemm_fast.hip) on the
64 x 128, 128 x 128 and both 256 x 256 tiles -- against tests/_wgrad_ref.py, at the smallest shapes at which each mechanism exists
(tests/test_gpu_ops.py keeps the step's own shapes).  Per call (tests/_wgrad_gpu.py: run_case):
  (a) hamt_debug_wgrad_times reports one kernel launch per tile class the case names, on the tile rows it names -- the demoted
      problems (keff or keff2 of one k-tile) on the small tiles next to neighbours on the 256 class -- and hamt_debug_wgrad_variants
      the kernel family: wgrad_grouped_p8_kernel for 256 rows, wgrad_grouped_kernel for them in the child under HAMT_WGRAD_P8=0;
  (b) every element of dW (or of the bf16 wire array) and every row of db is finite and within the derived per-element bound of float64;
  (c) every ss slot a tile of that size owns is within EPS32 (c + 2) of the float64 sum of squares of the fp32 dW read back, every
      other slot is +0.0;
  (d) nothing is written outside [M, N) of dW (ldw > N, rows below M), behind row M of db, behind the last ss slot, behind the table,
      or into a db / ss the problem did not pass;
  (e) a second call gives the same bits.
tests/test_wgrad_ref.py shows on the CPU that bounds and cases tell a wrong kernel from a right one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _wgrad_gpu as G
import _wgrad_ref as R

pytestmark = pytest.mark.gpu
CASES = [(s, cid) for s in R.SETTINGS for cid, _ in R.cases(s)]


@pytest.mark.parametrize("setting,cid", CASES, ids=[f"{s}-{c}" for s, c in CASES])
def test_wgrad_cases_vs_float64(setting, cid):
    G.run_case(setting, cid, dict(R.cases(setting))[cid])


def _copy(descs):
    out = type(descs)()
    C.memmove(out, descs, C.sizeof(descs))
    return out


@pytest.mark.parametrize("setting", ["64", "128", "auto256"])
def test_two_phase_launch_replays_from_the_table(setting):
    """hamt_wgrad_grouped_ex, what a captured step replays: phase 1 (table) then phase 2 (kernels) equals phase 3 bit for bit; the host
    array phase 1 read is then overwritten; the operands and the accumulated-onto outputs get other contents IN PLACE (same pointers),
    and phase 2 alone, twice, gives the bits of a fresh phase-3 call on those contents."""
    cs = dict(R.cases(setting))
    probs = cs["edges-a"] + cs["second-pair"][:8] + cs["k-valid"][:6]
    with G.tile_setting(setting):
        fresh = G.Call(probs)
        rows = fresh.launch(3)
        want = fresh.read()
        call = G.Call(probs)
        first, later = call.descs, _copy(call.descs)
        assert call.launch(1, descs=first) == [] and call.untouched() == []      # the table only: no grouped kernel, no output
        C.memset(first, 0xFF, C.sizeof(first))
        assert call.launch(2, descs=later) == rows
        assert G.same_bits(call.read(), want), "phase 1 + phase 2 differ from phase 3"
        other = [p._replace(seed=p.seed + 50) for p in probs]
        fresh2 = G.Call(other)
        fresh2.launch(3)
        want2 = fresh2.read()
        assert not G.same_bits(want2, want)
        call.fill(other)
        for replay in range(2):
            call.reset()
            assert call.launch(2, descs=later) == rows
            assert G.same_bits(call.read(), want2), f"replay {replay} of phase 2 differs from a fresh call on the new contents"
    worst = G.new_worst()
    for i, (p, pre, g) in enumerate(zip(other, fresh2.pre, want2)):
        G.check_problem(f"{setting} replay [{i}]", p, pre, g, worst)
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("setting", ["64", "128", "256"])
def test_a_problem_alone_equals_the_problem_among_others(setting):
    """Under a forced tile class a problem's tile rows, its units and each tile's k order depend on the problem alone; what the other
    problems of a call change is the XCD a unit is queued on and its place in that queue.  So the bits are those of the problem run alone
    -- on every class, the demoted problems of the 256 setting included (they run on the 64-row tiles either way)."""
    cs = dict(R.cases(setting))
    probs = cs["edges-b"] + cs["units"][:2] + cs["second-pair"][-4:]
    with G.tile_setting(setting):
        together = G.Call(probs)
        together.launch()
        got = together.read()
        for i in (0, 3, 5, 8, 9, 10, len(probs) - 1):
            alone = G.Call([probs[i]])
            assert alone.launch() == [probs[i].rows]
            assert G.same_bits(alone.read(), [got[i]]), f"{setting}: problem {i} {probs[i]} alone differs from the same problem among {len(probs)}"


def test_one_phase_256_tile_in_a_child(tmp_path):
    """wgrad_grouped_kernel<256, 256, 2, 4> behind HAMT_WGRAD_P8=0 (read once per process): one fresh python runs the 256-class cases, the
    wire outputs included (epi_store<EPI, 4> from the MFMA layout), with checks (a) - (e) inside -- (a) holds every 256-row launch of
    the child to the one-phase kernel, and every one of this process to the two-phase kernel"""
    out = tmp_path / "p8_0.txt"
    r = subprocess.run([sys.executable, os.path.join(G.ROOT, "tests", "_wgrad_gpu.py"), str(out)], env={**os.environ, "HAMT_WGRAD_P8": "0"},
                       capture_output=True, text=True, timeout=300)
    print(f"[wgrad HAMT_WGRAD_P8=0] worst error / bound per case:\n{out.read_text() if out.exists() else ''}")
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert len(out.read_text().splitlines()) == sum(any(p.rows == 256 for p in ps) for _, ps in R.cases("256")) >= 9


def test_zero_length_reduction_and_empty_call():
    """K = 0 with accumulate semantics changes no byte and needs no table; n = 0 returns OK; next to a real problem it stays a no-op"""
    L = G._L()
    probs = [R.prob(65, 129, 64, 64, acc=1, db=2, wide=False), R.prob(64, 128, 128, 64, acc=1, db=0, wide=False, seed=1)]
    with G.tile_setting("auto"):
        call = G.Call(probs)
        zero = _copy(call.descs)
        for d in zero:
            d.K, d.K_valid = 0, 0
        assert call.launch(descs=zero, table=None, table_bytes=0) == [] and call.untouched() == []
        assert call.launch(descs=None, n=0, table=None, table_bytes=0) == []
        L.check(L.load().hamt_wgrad_grouped(0, None, None, 0, G._stream()), "hamt_wgrad_grouped")
        assert call.untouched() == []
        mixed = _copy(call.descs)
        mixed[1].K = 0
        assert call.launch(descs=mixed) == [64]
        got = call.read()
        assert np.array_equal(got[1]["dw"], call.pre[1]["dw"]) and np.array_equal(got[1]["ss"], call.pre[1]["ss"])
        worst = G.new_worst()
        G.check_problem("next to K = 0", probs[0], call.pre[0], got[0], worst)
        assert all(v <= 1.0 for v in worst.values()), worst


def test_refusals_write_nothing():
    """the launcher's HAMT_CHECK_ARG refusals that this file's cases come near (not all of them: a null operand, operands of 4 GiB, K2 % 64,
    K2_valid > K2 and the second pair's leading dimensions are not here), on a call that holds problems of both launch classes: HamtError, and every byte of
    every output as it was -- the short table included, whose check once ran after the first class had been launched; a table of
    exactly the needed size is accepted"""
    L = G._L()
    probs = [R.prob(257, 255, 128, 256, acc=1, db=2), R.prob(65, 129, 64, 64, wide=False, seed=1), R.prob(8, 16, 64, 64, wide=False, acc=1, seed=2),
             R.prob(65, 129, 128, 64, wide=False, wire=0.5, seed=3)]
    BIG, NARROW, TINY, WIRE = range(4)
    needed = R.table_entries(probs, lambda p: p.rows)
    assert needed == 4
    with G.tile_setting("auto256"):
        call = G.Call(probs)

        def refused(what, i=None, table=0, table_bytes=None, **fields):
            d = _copy(call.descs)
            for k, v in fields.items():
                setattr(d[i], k, v)
            with pytest.raises(L.HamtError):
                call.launch(descs=d, table=table, table_bytes=table_bytes)
            assert call.untouched() == [], f"refused for {what}, yet written: {call.untouched()}"

        d0, dw = call.descs[BIG], call.descs[WIRE]
        refused("K % 64", BIG, K=100, K_valid=0)
        refused("ldy < 64", TINY, ldy=56)
        refused("ldx < 128", TINY, ldx=120)
        refused("ld % 8", BIG, ldy=d0.ldy + 4)
        refused("ldw < N", BIG, ldw=d0.N - 1)
        refused("an operand slice 8 bytes off", BIG, dy=d0.dy + 8)
        refused("K_valid > K", BIG, K_valid=d0.K + 1)
        refused("wire with accum_dw", WIRE, accum_dw=1)
        refused("wire with ldw % 8 != 0", WIRE, ldw=dw.ldw + 4)
        refused("dy2 without x2", BIG, dy2=d0.dy, K2=d0.K, ldy2=d0.ldy, ldx2=d0.ldx)
        refused("dy2 with a wire output", WIRE, dy2=dw.dy, x2=dw.x, K2=dw.K, ldy2=dw.ldy, ldx2=dw.ldx)
        refused("K = 0 with store semantics", NARROW, K=0, K_valid=0)
        refused("a misaligned table", table=8, table_bytes=call.table_bytes - 8)
        refused("a table one entry short", table_bytes=(needed - 1) * L.WGRAD_TABLE_ENTRY)
        assert call.launch(table_bytes=needed * L.WGRAD_TABLE_ENTRY) == [64, 256]
        got = call.read()
        worst = G.new_worst()
        for i, (p, pre, g) in enumerate(zip(probs, call.pre, got)):
            G.check_problem(f"table of exactly {needed} entries [{i}]", p, pre, g, worst)
        assert all(v <= 1.0 for v in worst.values()), worst
        assert bool((call.table[needed * L.WGRAD_TABLE_ENTRY:] == G.TABLE_BYTE).all()), "the table was written behind the needed entries"
