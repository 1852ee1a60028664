"""CPU half of the AdamW op-level tests: the cases of tests/_adamw_ref.py have the layout the kernel's paths need, fp32 arithmetic
stays well inside the 2e-6 bound on them (so the GPU half can hold the kernel to it), and every mistake the GPU half is meant to catch
-- a neighbour's hyper-parameters, a missing clip coefficient, a global instead of a per-parameter step count -- moves every active
tensor by far more than the bound (so the GPU half would notice)."""
import numpy as np
import pytest

import _adamw_ref as R

COEF = R.clip_coef(25.0, 1.0)          # 1 / (5 + 1e-6): the clip of test A


@pytest.fixture(scope="module")
def case():
    yield R.make_case()
    R.make_case.cache_clear()            # (9 M floats x 4 arrays: not kept for the rest of the session)
    R.small_case.cache_clear()


@pytest.fixture(scope="module")
def want(case):
    return R.restate(case, COEF)


def _active(c):
    return c["flags"] != 0


def test_layout(case):
    c = case
    nt = len(c["sizes"])
    assert nt == 1 + R.N_TINY + len(R.MEDIUM)
    assert c["n"] > R.SWEEP and c["n"] % 512 == 0 and c["ends"][-1] < c["n"]          # a second sweep; padding that belongs to no tensor
    assert (c["begins"] % 8 == 0).all() and (c["ends"] % 8 == 0).all() and (c["begins"][1:] == c["ends"][:-1]).all()
    # the large tensor ends a little before the wrap, the tiny run straddles it: block 0's second chunk starts about half-way into the run
    assert R.SWEEP - 60000 < c["ends"][0] < R.SWEEP < c["ends"][R.N_TINY] < R.SWEEP + 60000
    assert (c["sizes"][1:1 + R.N_TINY] >= 8).all() and (c["sizes"][1:1 + R.N_TINY] <= 40).all()
    at_wrap = int(np.searchsorted(c["ends"], R.SWEEP, side="right"))
    assert 1000 < at_wrap < 2000
    per_block = np.searchsorted(c["ends"], R.SWEEP + R.CHUNK, side="right") - at_wrap
    assert 100 < per_block < 500                                                        # each following block starts this many rows later
    assert tuple(c["sizes"][-len(R.MEDIUM):]) == R.MEDIUM
    lo, sz = c["begins"][-len(R.MEDIUM):], c["sizes"][-len(R.MEDIUM):]
    assert ((lo // R.CHUNK) != ((lo + sz - 1) // R.CHUNK)).any()
    # flags: 0, 1 and 2 all there; large, all-zero and last tensor active; NaN in every flag-0 slot and nowhere else
    f = c["flags"]
    assert set(np.unique(f)) == {0.0, 1.0, 2.0} and f[0] == 1 and f[-1] != 0 and f[c["zero"]] != 0
    assert c["sizes"][c["zero"]] == 4096
    dead = np.repeat(f == 0, np.diff(np.concatenate([c["begins"], [c["n"]]])))
    for k in ("p", "g", "m", "v"):
        assert (np.isnan(c[k]) == dead).all(), k
        assert not c[k][c["begins"][c["zero"]]:c["ends"][c["zero"]]].any()
    # a flag-0 tensor directly between two active ones, all three inside one 16-KiB chunk
    i = np.arange(1, nt - 1)
    between = (f[i] == 0) & (f[i - 1] != 0) & (f[i + 1] != 0) & (c["begins"][i - 1] // R.CHUNK == (c["ends"][i + 1] - 1) // R.CHUNK)
    assert between.sum() > 100
    # adjacent rows never share all of lr, step size and wd (the last row's neighbour in shifted() is row 0)
    h = c["hyp"][:, :3]
    assert (h != np.roll(h, -1, axis=0)).any(axis=1).all()
    assert (h[:, 1] != np.roll(h[:, 1], -1)).all()
    assert len(np.unique(h[:, 0])) == 2 and set(np.unique(h[:, 2])) == {np.float32(0.0), np.float32(0.05)}
    assert len(np.unique(np.round(h[:, 1] / h[:, 0], 5))) == 9
    # lr and wd alternate on different periods: all four combinations occur
    assert len({(a, b) for a, b in zip(h[:, 0].tolist(), h[:, 2].tolist())}) == 4


def test_small_case_layout():
    s = R.small_case()
    assert 39000 < s["n"] < 41000 and s["n"] % 512 == 0 and s["ends"][-1] < s["n"]
    assert set(np.unique(s["flags"])) == {0.0, 1.0, 2.0} and s["flags"][-1] != 0
    assert s["n"] > 4 * R.CHUNK and (s["begins"] % 8 == 0).all()
    h = s["hyp"][:, :3]
    assert (h[:-1] != h[1:]).any(axis=1).all()


@pytest.mark.parametrize("eps", [1e-6, 1e-8])
def test_fp32_arithmetic_has_headroom(case, eps):
    """adamw_one's operations in numpy float32 against the float64 restatement: at least 4 x inside the bound on every tensor"""
    c = dict(case, eps=eps)
    ref, got = R.restate(c, COEF), R.emulate32(c, COEF)
    act = _active(c)
    for k in ("p", "m", "v"):
        err = R.tensor_max(c, got[k].astype(np.float64) - ref[k])[act]
        scale = np.maximum(R.tensor_max(c, ref[k])[act], 1e-30)
        worst = float((err / scale).max())
        print(f"[adamw fp32 emulation, eps {eps:g}] {k}: worst per-tensor error {worst:.2e} of max|ref| (bound {R.TOL:g})")
        assert worst * 4 <= R.TOL, (k, worst)
    assert np.array_equal(got["g"].view(np.int32), ref["g"].astype(np.float32).view(np.int32))


def _moved(c, a, b):
    """per active tensor: max|a.p - b.p| over 20 x its tolerance in b"""
    act = _active(c)
    d = R.tensor_max(c, a["p"] - b["p"])[act]
    tol = R.TOL * R.tensor_max(c, b["p"])[act]
    live = tol > 0                                  # (the all-zero tensor stays zero under any hyper-parameters: tolerance 0)
    assert live.sum() == act.sum() - 1
    return float((d[live] / (20 * tol[live])).min())


@pytest.mark.parametrize("which", ["arena", "cut"])
def test_cases_are_sensitive(case, want, which):
    c, ref = (case, want) if which == "arena" else (R.small_case(), R.restate(R.small_case(), COEF))
    nb = _moved(c, R.restate(R.shifted(c), COEF), ref)
    nc = _moved(c, R.restate(c, 1.0), ref)
    print(f"[adamw case {which}] least movement over 20 x tolerance: neighbour's row {nb:.1f}, clip dropped {nc:.1f}")
    assert nb >= 1.0, nb
    assert nc >= 1.0, nc
    # the other arrays and the untouched slots: what the GPU half compares bit for bit
    dead = np.isnan(c["p"])
    for k in ("p", "g", "m", "v"):
        assert np.array_equal(ref[k][dead].view(np.int64), c[k][dead].astype(np.float64).view(np.int64))
    f = np.repeat(c["flags"], np.diff(np.concatenate([c["begins"], [c["n"]]])))
    assert not ref["g"][f == 1].any() and np.array_equal(ref["g"][f == 2], c["g"][f == 2].astype(np.float64))
    keep = R.restate(c, COEF, zero_grad=0)
    assert np.array_equal(keep["g"][f != 0], c["g"][f != 0].astype(np.float64))


def test_clip_coef():
    assert R.clip_coef(None, 1.0) == 1.0 and R.clip_coef(25.0, 0.0) == 1.0 and R.clip_coef(25.0, -1.0) == 1.0
    assert R.clip_coef(0.25, 1.0) == 1.0
    assert R.clip_coef(25.0, 1.0) == 1.0 / (5.0 + 1e-6)


def test_python_case_step_counts_are_visible():
    """test E's schedule: parameters PY_LAG miss steps 2 and 3, so in steps 4 and 5 their own step count is 2 behind the global one; the
    single-step restatement from the same state must move them by >= 20 x the bound when it uses the global count instead.  The clip
    coefficient is below 1 in some steps and exactly 1 in others."""
    tr = R.py_run(True)
    assert [t["coef"] < 1.0 for t in tr] == [True, False, True, False, True]
    assert [t["coef"] == 1.0 for t in tr] == [False, True, False, True, False]
    assert tr[-1]["counts"].tolist() == [5 if i not in R.PY_LAG else 3 for i in range(len(R.PY_SHAPES))]
    grads = R.py_case()["grads"]
    for i in R.PY_LAG:
        assert grads[1][i] is None and grads[2][i] is None and grads[3][i] is not None and grads[0][i] is not None
    worst = np.inf
    for s in (3, 4):
        p0, m0, v0 = tr[s]["before"]
        for i in R.PY_LAG:
            assert tr[s]["used"][i] == s + 1 - 2
            g = grads[s][i].reshape(-1)
            own = R.py_update(s, i, tr[s]["used"][i], p0[i], g, m0[i], v0[i], tr[s]["coef"])[0]
            glob = R.py_update(s, i, s + 1, p0[i], g, m0[i], v0[i], tr[s]["coef"])[0]
            worst = min(worst, float(np.abs(own - glob).max()) / (20 * R.TOL * float(np.abs(own).max())))
    print(f"[adamw python case] global instead of own step count: least movement over 20 x tolerance {worst:.1f}")
    assert worst >= 1.0, worst
    # the clip, per step where it applies, on every parameter with a gradient: seen in exp_avg (in the first step p itself hardly
    # depends on the coefficient: m / sqrt(v) is scale free up to eps)
    for s in (0, 2, 4):
        p0, m0, v0 = tr[s]["before"]
        for i, g in enumerate(grads[s]):
            if g is None:
                continue
            a = R.py_update(s, i, tr[s]["used"][i], p0[i], g.reshape(-1), m0[i], v0[i], tr[s]["coef"])[1]
            b = R.py_update(s, i, tr[s]["used"][i], p0[i], g.reshape(-1), m0[i], v0[i], 1.0)[1]
            assert float(np.abs(a - b).max()) >= 20 * R.TOL * float(np.abs(a).max()), (s, i)
