"""Not gpu: the host side of the owned-item RangerLars update (optim/rangerlars.py `item_table(..., cuts)`, `owned_item_runs`;
parallel.ShardedItemSync's cuts) -- the table without cuts is the one it always was, a table with cuts keeps every item inside one
parameter and one owner, the ranks' item runs partition the table -- and a float64 restatement showing that the GPU comparisons of
tests/test_gpu_ralamb_items.py can tell a skipped item, an item run twice and a stale trust ratio from a correct run.  Plus the
code-object check of the three kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ralamb_items_ref as R  # noqa: E402


def test_item_table_without_cuts_is_unchanged():
    from vln_hamt_amd.optim.rangerlars import item_table
    for ends, (nitems, want) in R.RECORDED.items():
        for kw in ({}, {"cuts": ()}, {"cuts": []}):
            tab, n = item_table(np.array(ends), ends[-1], **kw)
            assert n == nitems and tab.dtype == np.int32 and tab.tolist() == want, ends
    # cuts that fall on item boundaries the table has anyway change nothing either
    tab, n = item_table(R.ENDS, R.N, cuts=(32, 4128, 4128 + 4096))
    assert tab.tolist() == R.RECORDED[tuple(R.ENDS.tolist())][1]


def _check_table(ends, n, cuts):
    from vln_hamt_amd.optim.rangerlars import ITEM4, item_table
    tab, nitems = item_table(ends, n, cuts)
    assert tab.dtype == np.int32 and tab.size == 2 * nitems + len(ends) + 2
    starts, param, first = R.split(tab, nitems, len(ends))
    assert starts[0] == 0 and starts[-1] == n // 4 and (np.diff(starts) > 0).all() and (np.diff(starts) <= ITEM4).all()      # tile [0, n/4) in order
    assert first[0] == 0 and first[-1] == nitems and (np.diff(first) >= 0).all()
    begins = np.concatenate([[0], ends[:-1]])
    bounds = np.array(sorted(set([0, n]) | set(int(c) for c in cuts)))
    for j in range(nitems):
        lo, hi, q = 4 * starts[j], 4 * starts[j + 1], param[j]
        assert begins[q] <= lo and hi <= ends[q], (j, "straddles a parameter")
        k = np.searchsorted(bounds, lo, side="right")
        assert bounds[k - 1] <= lo and hi <= bounds[k], (j, "straddles a cut")
    for q in range(len(ends)):
        its = np.arange(first[q], first[q + 1])
        assert (param[its] == q).all() and (param == q).sum() == its.size
        if its.size:
            assert 4 * starts[its[0]] == begins[q] and 4 * starts[its[-1] + 1] == ends[q]
    return tab, nitems


def test_item_table_with_cuts():
    from vln_hamt_amd.optim.rangerlars import item_table
    tab, nitems = _check_table(R.ENDS, R.N, R.CUTS)
    assert nitems == 12 + 2                       # the cut on the parameter boundary adds no item; the other two split one item each
    _check_table(R.TWO_REGION_ENDS, R.TWO_REGION_N, (8, 2688, 5376, 21504, 21504 + 3072))
    _check_table(np.array([8, 8, 4096, 4104, 16400, 53280]), 53280, (8, 16, 4100 * 4, 40000))      # an empty parameter, a cut at its place
    for bad in ((4,), (12,), (-8,), (R.N + 8,)):
        with pytest.raises(ValueError):
            item_table(R.ENDS, R.N, bad)


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_owned_item_runs_of_the_ranks_partition_the_table(world):
    """parallel.ShardedItemSync's construction on an arena with both regions: cuts = every chunk boundary of every static range"""
    from vln_hamt_amd.optim.rangerlars import item_table, owned_item_runs
    from vln_hamt_amd.parallel import shard_cuts
    n, n_a = R.TWO_REGION_N, R.TWO_REGION_NA
    sc = shard_cuts(n, n_a, world, 4)
    ranges = [(lo, hi) for lo, hi in zip(sc[:-1], sc[1:]) if hi > lo]
    assert any(hi <= n_a for lo, hi in ranges) and any(lo >= n_a for lo, hi in ranges)
    cuts = {lo + r * ((hi - lo) // world) for lo, hi in ranges for r in range(world + 1)}
    tab, nitems = _check_table(R.TWO_REGION_ENDS, n, cuts)
    seen = np.zeros(nitems, dtype=np.int64)
    elems = 0
    starts = tab[:nitems + 1].astype(np.int64)
    for rank in range(world):
        owned = [(lo + rank * ((hi - lo) // world), (hi - lo) // world) for lo, hi in ranges]
        runs = owned_item_runs(tab, nitems, owned)
        assert all(c > 0 for _, c in runs) and all(a[0] + a[1] < b[0] for a, b in zip(runs, runs[1:])), runs      # maximal, in order
        for f, c in runs:
            seen[f:f + c] += 1
            elems += 4 * int(starts[f + c] - starts[f])
        assert sum(c for _, c in owned) == sum(4 * int(starts[f + c] - starts[f]) for f, c in runs)
    assert (seen == 1).all() and elems == n
    # a table built WITHOUT the cuts has items that straddle two owners: refused, not rounded
    if world > 1:
        plain, k = item_table(R.TWO_REGION_ENDS, n)
        with pytest.raises(ValueError, match="straddles"):
            for rank in range(world):
                owned_item_runs(plain, k, [(lo + rank * ((hi - lo) // world), (hi - lo) // world) for lo, hi in ranges])


def _item_runs():
    from vln_hamt_amd.optim.rangerlars import item_table, owned_item_runs
    tab, nitems = item_table(R.ENDS, R.N, R.CUTS)
    return tab, nitems, [owned_item_runs(tab, nitems, [s])[0] for s in R.SEGMENTS]


def _ranged(c, tab, nitems, runs, order_m, order_a, mutate=None):
    st = R.ItemRestatement(c, tab, nitems)
    for k in order_m:
        f, n = runs[k]
        if mutate == "skip" and k == R.MIDDLE:
            f, n = f + 1, n - 1                    # the range's first item is never run
        st.moments(f, n)
        if mutate == "twice" and k == R.MIDDLE:
            st.moments(f, 1)                       # ... or run a second time (overlapping ranges: its slot is written twice)
    if mutate == "stale":
        st.apply(*runs[order_a[0]])                # an apply before the trust pass: the trust ratios of the step before
    st.trust()
    for k in order_a[1:] if mutate == "stale" else order_a:
        st.apply(*runs[k])
    return st


def _close(st, want, stats):
    for k in ("p", "g", "m", "v", "slow"):
        a, b = st.a[k], want[k]
        ok = np.isfinite(b)
        if not (np.array_equal(np.isfinite(a), ok) and np.allclose(a[ok], b[ok], rtol=1e-11, atol=1e-14)):
            return False
    return all(np.allclose(st.stats[q], s, rtol=1e-11) for q, s in stats.items())


@pytest.mark.parametrize("step", [0, 1])
def test_float64_ranged_update_equals_the_whole_and_mutations_do_not(step):
    from test_gpu_rangerlars import _restate
    c = R.make_case(step)
    tab, nitems, runs = _item_runs()
    assert sorted(runs) == runs and runs[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(runs, runs[1:])) and sum(runs[-1]) == nitems
    want, stats = _restate(c, R.MAX_NORM, R.GSQ, R.B1, R.B2, R.EPS)
    for order_m, order_a in (([0, 1, 2, 3], [0, 1, 2, 3]), ([2, 0, 3, 1], [3, 1, 0, 2]), ([3, 2, 1, 0], [1, 3, 2, 0])):
        st = _ranged(c, tab, nitems, runs, order_m, order_a)
        assert _close(st, want, stats), (order_m, order_a)
        inactive = [j for j in range(nitems) if c["active"][st.param[j]] == 0]
        assert np.isnan(st.partials[inactive]).all() and np.isfinite(np.delete(st.partials, inactive, 0)).all()     # one write per active slot
    for mutate in ("skip", "twice", "stale"):
        assert not _close(_ranged(c, tab, nitems, runs, [2, 0, 3, 1], [3, 1, 0, 2], mutate), want, stats), mutate


def test_ralamb_item_kernels_have_no_spills_and_no_scratch(tmp_path):
    """the three kernel bodies (each serves the whole-table launch and the item-range entry point) in the gfx950 code object"""
    import test_kernel_resources as tkr
    if not (os.path.exists(tkr.READELF) and os.path.exists(tkr.OBJCOPY)):
        pytest.skip("ROCm LLVM tools not installed")
    from vln_hamt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    seen = {}
    for co in tkr._code_objects(_lib.LIB_PATH, str(tmp_path)):
        notes = subprocess.run([tkr.READELF, "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and "ralamb_" in name.group(1):
                seen[name.group(1)] = tuple(int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in
                                            ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    kernels = {k: [v for n, v in seen.items() if k in n] for k in ("ralamb_moments_kernel", "ralamb_trust_kernel", "ralamb_apply_kernel")}
    assert all(len(v) == 1 for v in kernels.values()) and len(seen) == 3, seen      # one body per pass
    assert all(v[0][:3] == (0, 0, 0) for v in kernels.values()), seen
    assert kernels["ralamb_moments_kernel"][0][3] == 2 * 4 * 2 * 4 and kernels["ralamb_trust_kernel"][0][3] == 0 and kernels["ralamb_apply_kernel"][0][3] == 0, seen
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ("hamt_ralamb_moments_items", "hamt_ralamb_trust", "hamt_ralamb_apply_items")) and lib.hamt_version() == 2
