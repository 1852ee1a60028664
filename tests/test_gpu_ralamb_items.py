"""-m gpu: the item-range entry points of the Ralamb update (include/hamt.h hamt_ralamb_moments_items / hamt_ralamb_trust /
hamt_ralamb_apply_items) at op level, on the arena of tests/_ralamb_items_ref.py (under 30 000 elements: two tiny tensors, one item
exactly, a full item + a 2-float4 item, three items, an inactive tensor, one with active == 2; cuts inside the 24-element tensor, on a
tensor boundary and in the middle of an item), with two steps' worth of tables (both N_sma branches x the three Lookahead actions,
with and without weight decay, clip active):
  * disjoint item ranges in scrambled orders == one hamt_ralamb_table launch, bit for bit, every arena and table;
  * one range alone changes no byte outside its own elements and partial slots (0xFF guards around every arena included);
  * the union against the float64 restatement and the bound of test_ralamb_table_op_vs_float64;
  * refused calls return HAMT_ERR_ARG and change nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ralamb_items_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                  # elements of 0xFF bytes in front of and behind every arena
ARENAS = ("p", "g", "m", "v", "slow", "p16", "stats", "partials")
HAMT_OK, HAMT_ERR_ARG = 0, -1


def _table():
    from vln_hamt_amd.optim.rangerlars import item_table, owned_item_runs
    tab, nitems = item_table(R.ENDS, R.N, R.CUTS)
    runs = [owned_item_runs(tab, nitems, [s])[0] for s in R.SEGMENTS]
    assert sum(c for _, c in runs) == nitems
    return tab, nitems, runs


class State:
    """device arenas of one case, each inside a buffer with 0xFF guards; `buf` is what the comparisons look at"""

    def __init__(self, c, tab, nitems, stats=7.0):
        self.c, self.nitems, self.np_ = c, nitems, len(c["ends"])
        self.buf, self.a = {}, {}
        src = {k: torch.from_numpy(c[k]) for k in ("p", "g", "m", "v", "slow")}
        p16 = torch.full((c["n"],), float("nan")).to(torch.bfloat16)
        for i in range(self.np_):
            if c["active"][i] != 0:
                p16[c["begins"][i]:c["ends"][i]] = 0
        src["p16"] = p16
        src["stats"] = torch.full((self.np_ * 4,), float(stats)) if np.isscalar(stats) else torch.as_tensor(stats, dtype=torch.float32).reshape(-1)
        src["partials"] = torch.full((2 * nitems,), float("nan"))
        for k, t in src.items():
            b = torch.empty(t.numel() + 2 * GUARD, dtype=t.dtype, device=DEV)
            b.view(torch.uint8).fill_(0xFF)
            b[GUARD:GUARD + t.numel()].copy_(t)
            self.buf[k], self.a[k] = b, b[GUARD:GUARD + t.numel()]
        self.items = torch.from_numpy(tab).to(DEV)
        self.hyp, self.rl = torch.from_numpy(c["hyp"]).to(DEV), torch.from_numpy(c["rl"]).to(DEV)
        self.gn = torch.tensor([R.GSQ], device=DEV)

    def bytes(self):
        torch.cuda.synchronize()
        return {k: b.view(torch.uint8).cpu().numpy().copy() for k, b in self.buf.items()}

    def host(self, k):
        torch.cuda.synchronize()
        return self.a[k].float().cpu().numpy() if k == "p16" else self.a[k].cpu().numpy()

    # ---- the four entry points; `over`: arguments replaced by name (the bad-argument test)
    def _args(self, **over):
        from vln_hamt_amd.ops import _p, _stream
        d = {k: _p(t) for k, t in self.a.items()}
        d.update(items=_p(self.items), hyp=_p(self.hyp), rl=_p(self.rl), gn=_p(self.gn), nitems=self.nitems, np=self.np_, stream=_stream())
        d.update(over)
        return d

    def whole(self):
        from vln_hamt_amd import _lib as L
        d = self._args()
        return L.load().hamt_ralamb_table(d["p"], d["g"], d["m"], d["v"], d["p16"], d["slow"], d["items"], d["nitems"], d["hyp"], d["rl"], d["np"],
                                          d["partials"], d["stats"], d["gn"], R.MAX_NORM, R.B1, R.B2, 1 - R.B1, 1 - R.B2, R.EPS, 1, d["stream"])

    def moments(self, first, count, **over):
        from vln_hamt_amd import _lib as L
        d = self._args(**over)
        return L.load().hamt_ralamb_moments_items(d["p"], d["g"], d["m"], d["v"], d["items"], d["nitems"], first, count, d["hyp"], d["rl"], d["np"],
                                                  d["partials"], d["gn"], R.MAX_NORM, R.B1, R.B2, 1 - R.B1, 1 - R.B2, R.EPS, 1, d["stream"])

    def trust(self, **over):
        from vln_hamt_amd import _lib as L
        d = self._args(**over)
        return L.load().hamt_ralamb_trust(d["items"], d["nitems"], d["hyp"], d["np"], d["partials"], d["stats"], d["stream"])

    def apply(self, first, count, **over):
        from vln_hamt_amd import _lib as L
        d = self._args(**over)
        return L.load().hamt_ralamb_apply_items(d["p"], d["m"], d["v"], d["p16"], d["slow"], d["items"], d["nitems"], first, count, d["hyp"],
                                                d["rl"], d["np"], d["stats"], R.EPS, d["stream"])


_results = {}


def _union(step):
    """(whole-launch bytes, ranged-update bytes, ranged State) of one step's tables, computed once for the tests that need them"""
    if step not in _results:
        tab, nitems, runs = _table()
        c = R.make_case(step)
        a = State(c, tab, nitems)
        init = a.bytes()
        assert a.whole() == HAMT_OK
        b = State(c, tab, nitems)
        for k in (2, 0, 3, 1):
            assert b.moments(*runs[k]) == HAMT_OK
        assert b.trust() == HAMT_OK
        for k in (3, 1, 0, 2):
            assert b.apply(*runs[k]) == HAMT_OK
        _results[step] = (init, a.bytes(), b.bytes(), b)
    return _results[step]


@pytest.mark.parametrize("step", [0, 1])
def test_union_of_item_ranges_is_the_whole(step):
    init, whole, ranged, _ = _union(step)
    for k in ARENAS:
        assert np.array_equal(whole[k], ranged[k]), k
    for k in ("p", "m", "v", "slow", "p16", "stats", "partials", "g"):
        assert not np.array_equal(whole[k], init[k]), (k, "the update changed nothing")


@pytest.mark.parametrize("step", [0, 1])
def test_union_of_item_ranges_vs_float64(step):
    """bound and restatement of test_ralamb_table_op_vs_float64 (per tensor, max|got - ref| <= TOL * max|ref|)"""
    from _adamw_ref import TOL
    from test_gpu_rangerlars import _restate
    _, _, _, st = _union(step)
    c = st.c
    want, stats = _restate(c, R.MAX_NORM, R.GSQ, R.B1, R.B2, R.EPS)
    got = {k: st.host(k).astype(np.float64) for k in ("p", "g", "m", "v", "slow", "p16")}
    got_stats = st.host("stats").reshape(-1, 4)
    for i in range(len(c["ends"])):
        sl = slice(c["begins"][i], c["ends"][i])
        if c["active"][i] == 0:
            assert all(np.isnan(got[k][sl]).all() for k in got) and (got_stats[i] == 7.0).all()
            continue
        for k in ("p", "m", "v", "slow"):
            ref = want[k][sl]
            err = float(np.abs(got[k][sl] - ref).max()) / max(float(np.abs(ref).max()), 1e-30)
            print(f"[ralamb items vs float64] step {step} tensor {i} ({R.SIZES[i]}) {k}: {err:.2e}")
            assert err <= TOL, (i, k, err)
        assert np.array_equal(got["g"][sl], c["g"][sl] if c["active"][i] == 2 else np.zeros_like(c["g"][sl])), i
        assert np.array_equal(st.host("p16")[sl], torch.from_numpy(st.host("p")[sl]).to(torch.bfloat16).float().numpy()), i
        # (the norms and the trust ratio themselves: bit-equal to the whole launch's above, which test_ralamb_table_op_vs_float64 bounds;
        #  a wrong trust ratio is in p)
        assert got_stats[i, 3] == 0.0 and np.isfinite(got_stats[i]).all(), (i, got_stats[i], stats[i])


def _elem_mask(nbytes_per_elem, n, spans):
    """uint8 mask over a guarded buffer: True where a byte may change"""
    m = np.zeros((n + 2 * GUARD) * nbytes_per_elem, dtype=bool)
    for lo, hi in spans:
        m[(GUARD + lo) * nbytes_per_elem:(GUARD + hi) * nbytes_per_elem] = True
    return m


@pytest.mark.parametrize("step", [0, 1])
def test_one_item_range_touches_nothing_else(step):
    tab, nitems, runs = _table()
    c = R.make_case(step)
    f, n = runs[R.MIDDLE]
    lo, hi = R.SEGMENTS[R.MIDDLE][0], sum(R.SEGMENTS[R.MIDDLE])
    assert 4 * int(tab[f]) == lo and 4 * int(tab[f + n]) == hi and n >= 3
    stats0 = np.tile(np.array([1.5, 3.0, 0.5, 0.0], dtype=np.float32), len(c["ends"]))
    st = State(c, tab, nitems, stats=stats0)
    init = st.bytes()
    # an empty range: HAMT_OK, nothing launched, nothing changed
    assert st.moments(f, 0) == HAMT_OK and st.apply(nitems, 0) == HAMT_OK
    same = st.bytes()
    assert all(np.array_equal(same[k], init[k]) for k in ARENAS)
    # pass 1 alone: m, v, g inside the range's elements; the range's partial slots; nothing else
    assert st.moments(f, n) == HAMT_OK
    after = st.bytes()
    may = {"m": _elem_mask(4, R.N, [(lo, hi)]), "v": _elem_mask(4, R.N, [(lo, hi)]), "g": _elem_mask(4, R.N, [(lo, hi)]),
           "partials": _elem_mask(4, 2 * nitems, [(2 * f, 2 * (f + n))])}
    for k in ARENAS:
        changed = after[k] != init[k]
        assert not (changed & ~may[k]).any() if k in may else not changed.any(), (k, "pass 1 wrote outside its range")
    for k in ("m", "v", "g", "partials"):
        assert (after[k] != init[k]).any(), k
    assert np.isfinite(st.host("partials")[2 * f:2 * (f + n)]).all() and np.isnan(np.delete(st.host("partials"), np.s_[2 * f:2 * (f + n)])).all()
    # pass 3 alone (the trust ratios given): p, p16 and -- where the table has a Lookahead action -- slow inside the range's elements
    assert st.apply(f, n) == HAMT_OK
    last = st.bytes()
    may = {"p": _elem_mask(4, R.N, [(lo, hi)]), "slow": _elem_mask(4, R.N, [(lo, hi)]), "p16": _elem_mask(2, R.N, [(lo, hi)])}
    for k in ARENAS:
        changed = last[k] != after[k]
        assert not (changed & ~may[k]).any() if k in may else not changed.any(), (k, "pass 3 wrote outside its range")
    assert (last["p"] != after["p"]).any() and (last["p16"] != after["p16"]).any() and (last["slow"] != after["slow"]).any()


def test_item_range_calls_refuse_bad_arguments():
    from vln_hamt_amd import _lib as L
    tab, nitems, runs = _table()
    st = State(R.make_case(0), tab, nitems)
    init = st.bytes()
    off = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)
    bad_m = [st.moments(nitems, 1), st.moments(nitems - 1, 2), st.moments(-1, 2), st.moments(0, -1), st.moments(0, nitems + 1),
             st.moments(0, nitems, p=None), st.moments(0, nitems, g=None), st.moments(0, nitems, m=None), st.moments(0, nitems, v=None),
             st.moments(0, nitems, items=None), st.moments(0, nitems, hyp=None), st.moments(0, nitems, rl=None), st.moments(0, nitems, partials=None),
             st.moments(0, nitems, nitems=0), st.moments(0, nitems, np=0),
             st.moments(0, nitems, hyp=off(st.hyp, 4)), st.moments(0, nitems, rl=off(st.rl, 8)), st.moments(0, nitems, partials=off(st.a["partials"], 4)),
             st.moments(0, nitems, m=off(st.a["m"], 4))]
    bad_t = [st.trust(items=None), st.trust(hyp=None), st.trust(partials=None), st.trust(stats=None), st.trust(nitems=0), st.trust(np=0),
             st.trust(hyp=off(st.hyp, 4)), st.trust(stats=off(st.a["stats"], 8)), st.trust(partials=off(st.a["partials"], 4))]
    bad_a = [st.apply(nitems, 1), st.apply(1, nitems), st.apply(-2, 1), st.apply(0, -1),
             st.apply(0, nitems, p=None), st.apply(0, nitems, m=None), st.apply(0, nitems, v=None), st.apply(0, nitems, items=None),
             st.apply(0, nitems, hyp=None), st.apply(0, nitems, rl=None), st.apply(0, nitems, stats=None), st.apply(0, nitems, np=0),
             st.apply(0, nitems, stats=off(st.a["stats"], 4)), st.apply(0, nitems, rl=off(st.rl, 4)), st.apply(0, nitems, slow=off(st.a["slow"], 4)),
             st.apply(0, nitems, p16=off(st.a["p16"], 2))]
    assert set(bad_m) == set(bad_t) == set(bad_a) == {HAMT_ERR_ARG}, (bad_m, bad_t, bad_a)
    assert "hamt_ralamb_apply_items" in L.last_error()
    after = st.bytes()
    assert all(np.array_equal(after[k], init[k]) for k in ARENAS)
    # the optional arenas may be NULL: no shadow, no slow weights (every Lookahead action is then ignored)
    assert st.moments(0, nitems) == HAMT_OK and st.trust() == HAMT_OK and st.apply(0, nitems, p16=None, slow=None) == HAMT_OK
    last = st.bytes()
    assert np.array_equal(last["p16"], init["p16"]) and np.array_equal(last["slow"], init["slow"]) and not np.array_equal(last["p"], init["p"])
