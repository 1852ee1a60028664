"""CPU half of the LayerNorm op-level tests: the fp32 restatement of csrc/norm.hip (tests/_ln_ref.py) stays inside the caps that
test_gpu_ln.py's bounds are derived from, every mistake a rewrite of the kernels could make moves a named case by at least 10 x the GPU
bound of the output it corrupts, and the case table reaches every instantiation, geometry, threshold and row kind.  No GPU, no torch."""
import numpy as np
import pytest

import _ln_ref as R


def _caught(c, mut, output, add=None):
    """worst error / GPU bound of `output` with the mistake switched on"""
    errs = R.errors(c, R.ln32(c, mut, add=add), add=add)
    return R.worst_ratio({k: v for k, v in errs.items() if k[0] == output})[output]


def test_float64_backward_is_the_derivative_of_the_float64_forward():
    """central differences of sum(dy * y) in x, gamma, beta on a 3 x 12 case with both masks: the reference checks itself"""
    base = R._make_case("fd", 3, 12, 7, 1e-6, True, 0.1, 0.5, kinds=("randn", "off30", "big"))
    ref = R.ln64(base)
    dy = base["dy"].astype(np.float64)

    def loss(**kw):
        c = dict(base)
        c.update(kw)
        return float((R.ln64(c, x=kw.get("x"))["y"] * dy).sum())
    h = 1e-6
    for (r, col) in ((0, 0), (1, 5), (2, 11), (0, 7)):
        step = h * max(1.0, abs(float(base["x"][r, col])))
        xp, xm = base["x"].astype(np.float64), base["x"].astype(np.float64)
        xp[r, col] += step
        xm[r, col] -= step
        fd = (loss(x=xp) - loss(x=xm)) / (2 * step)
        assert abs(fd - ref["dx"][r, col]) <= 1e-5 * np.abs(ref["dx"][r]).max(), (r, col, fd, ref["dx"][r, col])
    for col in (0, 6, 11):
        for name, grad in (("gamma", "dgamma"), ("beta", "dbeta")):
            p, m = base[name].astype(np.float64), base[name].astype(np.float64)
            p[col] += h
            m[col] -= h
            fd = (loss(**{name: p}) - loss(**{name: m})) / (2 * h)
            assert abs(fd - ref[grad][col]) <= 1e-6 * max(1.0, np.abs(ref[grad]).max()), (name, col)
    a = R.ln64(base, add=base["add"])
    assert np.array_equal(a["dz"], ref["dz"] + base["add"]) and np.array_equal(a["dgamma"], ref["dgamma"]) and np.array_equal(a["dbeta"], ref["dbeta"])
    assert np.array_equal(ref["dxsum"], ref["dx"].sum(axis=0)) and not np.array_equal(ref["dx"], ref["dz"])


def test_fp32_restatement_is_inside_the_measured_caps():
    row, col = {}, {}
    for c in R.cases().values():
        for add in ((None,) if (c["p_pre"] > 0 or c["p_post"] > 0) else (None, c["add"])):
            out = R.ln32(c, add=add)
            assert R.image_errors(out["y16"], out["y"], c["M"]) == (0, 0) and R.image_errors(out["dx16"], out["dx"], c["M"]) == (0, 0)
            for (name, kind), e in R.errors(c, out, add=add).items():
                assert e <= R.measured(name, kind), (c["name"], name, kind, e)
                d = col if kind is None else row.setdefault(name, {})
                d[name if kind is None else kind] = max(d.get(name if kind is None else kind, 0.0), e)
    for name in R.ROW_OUTPUTS:
        print(f"[ln32 vs float64] {name:5s} " + "  ".join(f"{k} {row[name][k]:.2g} (cap {R.measured(name, k):.2g})" for k in R.KINDS))
    print("[ln32 vs float64] column sums in units of eps32 U_c: " + "  ".join(f"{n} {col[n]:.2f} (cap {R.measured(n):.2g})" for n in R.COL_OUTPUTS))
    for name in R.ROW_OUTPUTS:                          # the caps are the measured values, not something wider
        for k in R.KINDS:
            assert R.measured(name, k) <= 1.11 * row[name][k], (name, k)
    assert all(R.measured(n) <= 1.1 * col[n] + 0.05 for n in R.COL_OUTPUTS)
    # the offset rows' caps are theirs alone: the well-conditioned rows stay at a few roundings
    for name in ("y", "dz", "dx", "rstd", "mean"):
        for k in ("randn", "big", "small"):
            assert R.cap(name, k) <= 4e-7 and R.cap(name, k) < R.cap("y", "off100") / 100


# (mistake, switches, case, corrupted output, with `add`)
MISTAKES = [
    ("one-pass variance", dict(one_pass=True), "37x132", "rstd", False),
    ("one-pass variance, seen in y", dict(one_pass=True), "1025x768", "y", False),
    ("eps outside the square root", dict(eps_outside=True), "37x64", "rstd", False),
    ("divisor H - 1", dict(div_hm1=True), "37x1020", "rstd", False),
    ("divisor the padded width", dict(div_padded=True), "37x260", "mean", False),
    ("dead columns of the last vector counted", dict(count_dead=True), "37x516", "rstd", False),
    ("c1 dropped", dict(no_c1=True), "37x768", "dz", False),
    ("c2 dropped", dict(no_c2=True), "37x768", "dz", False),
    ("rstd missing on dz", dict(no_rstd=True), "37x4", "dz", False),
    ("dgamma from dy gamma", dict(dgamma_dyg=True), "37x516", "dgamma", False),
    ("dgamma before the post mask", dict(dg_before_post=True), "post 130x256 p 0.5", "dgamma", False),
    ("dbeta before the post mask", dict(dg_before_post=True), "post 37x132 p 0.1", "dbeta", False),
    ("mean / rstd of the neighbouring row", dict(neighbour_stats=True), "5x64", "dz", False),
    ("4 waves: wave 2 dropped", dict(drop_wave=2), "37x256", "dbeta", False),
    ("8 waves: wave 1 dropped", dict(drop_wave=1), "1024x64", "dgamma", False),
    ("8 waves: upper wave 6 dropped", dict(drop_wave=6), "1025x768", "dbeta", False),
    ("16 waves: wave 3 dropped", dict(drop_wave=3), "2048x132", "dbeta", False),
    ("16 waves: middle wave 5 dropped", dict(drop_wave=5), "2049x1024", "dgamma", False),
    ("16 waves: upper wave 12 dropped", dict(drop_wave=12), "4095x64", "dbeta", False),
    ("last block's partial dropped", dict(drop_last_block=True), "1025x132", "dbeta", False),
    ("second trip dropped", dict(drop_trip2=True), "4100x64", "dbeta", False),
    ("second trip dropped, one row", dict(drop_trip2=True), "4097x132", "dgamma", False),
    ("dxsum sums dz", dict(dxsum_dz=True), "pre 37x132 p 0.1", "dxsum", False),
    ("add leaks into dxsum", dict(add_leaks=True), "1x64", "dxsum", True),
    ("add leaks into dgamma", dict(add_leaks=True), "37x1020", "dgamma", True),
    ("pre and post keys swapped", dict(swap_keys=True), "both 70x260 p 0.1/0.5", "y", False),
    ("pre and post keys swapped, seen in dx", dict(swap_keys=True), "both 70x260 p 0.1/0.5", "dx", False),
    ("both masks from one key", dict(one_key=True), "both 1030x768 p 0.5/0.1", "y", False),
    ("mask per column", dict(per_column=True), "post 37x132 p 0.1", "y", False),
    ("mask per column, pre", dict(per_column=True), "pre 1030x64 p 0.5", "z", False),
    ("p_pre not applied to dx", dict(pre_not_on_dx=True), "pre 1030x64 p 0.5", "dx", False),
    ("dropped positions of y not exactly 0", dict(dropped_not_zero=True), "post 37x132 p 0.1", "y", False),
]


@pytest.mark.parametrize("what,mut,case,output,with_add", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_mistake_is_caught(what, mut, case, output, with_add):
    c = R.cases()[case]
    add = c["add"] if with_add else None
    clean = _caught(c, None, output, add)
    ratio = _caught(c, mut, output, add)
    print(f"[{what}] {case}: {output} at {ratio:.3g} x its GPU bound (unswitched: {clean:.3g})")
    assert clean <= 1.0 / R.GPU_MARGIN + 1e-12
    assert ratio >= R.CAUGHT_FACTOR


def test_wave_mistakes_name_waves_of_the_geometry_they_claim():
    for what, mut, case, _, _ in MISTAKES:
        if "drop_wave" in mut:
            nwv = R.geometry(R.cases()[case]["M"])[0]
            assert what.startswith(f"{nwv} waves") and mut["drop_wave"] < nwv, what
    assert R.geometry(4097)[1] == 256 and 4097 > 256 * 16 and R.geometry(1025) == (8, 129)


def test_unzeroed_padding_rows_are_caught():
    c = R.cases()["37x132"]
    good, bad = R.ln32(c), R.ln32(c, dict(pad_unzeroed=True))
    for img, val in (("y16", "y"), ("dx16", "dx")):
        assert R.image_errors(good[img], good[val], c["M"]) == (0, 0)
        assert R.image_errors(bad[img], bad[val], c["M"]) == (0, (R.mpad(37) - 37) * 132)
    off = good["y16"].copy()
    off[3, 5] ^= 1                                                 # one bf16 ulp in one element shows as well
    assert R.image_errors(off, good["y"], c["M"]) == (1, 0)


def grouped_problem():
    """the entries of test_gpu_ln.py's grouped reduction, restated: two entries add into one pre-filled dgamma (bit 0), a third overwrites"""
    rng = np.random.Generator(np.random.PCG64(5))
    ws = [rng.standard_normal((nb, 3, 64)).astype(R.F32) for nb in (10, 129, 7)]
    entries = [dict(ws=ws[0], out=("shared", None, None), atomic=1), dict(ws=ws[1], out=("shared", "b1", None), atomic=1),
               dict(ws=ws[2], out=("own", None, "s2"), atomic=0)]
    start = dict(shared=np.full(64, 5.0), b1=np.full(64, 9.0), own=np.full(64, 5.0), s2=np.full(64, -3.0))
    want = dict(shared=5.0 + ws[0][:, 0].astype(np.float64).sum(0) + ws[1][:, 0].astype(np.float64).sum(0), b1=ws[1][:, 1].astype(np.float64).sum(0),
                own=ws[2][:, 0].astype(np.float64).sum(0), s2=ws[2][:, 2].astype(np.float64).sum(0))
    unit = dict(shared=5.0 + np.abs(ws[0][:, 0]).sum(0) + np.abs(ws[1][:, 0]).sum(0), b1=np.abs(ws[1][:, 1]).sum(0), own=np.abs(ws[2][:, 0]).sum(0),
                s2=np.abs(ws[2][:, 2]).sum(0))
    return entries, start, want, unit


def test_grouped_atomic_bit_read_inverted_is_caught():
    entries, start, want, unit = grouped_problem()
    good, bad = R.grouped32(entries, start), R.grouped32(entries, start, dict(invert_atomic=True))
    bnd = R.bound("dbeta")
    for k in want:
        assert (np.abs(good[k] - want[k]) / (R.EPS32 * unit[k])).max() <= bnd / R.GPU_MARGIN
    for k in ("shared", "own", "b1"):
        assert (np.abs(bad[k] - want[k]) / (R.EPS32 * unit[k])).max() >= R.CAUGHT_FACTOR * bnd, k


def test_case_table_holds_what_the_gpu_half_needs():
    cs = R.cases()
    plain = R.plain_cases()
    assert len(plain) == len(R.M_NARROW) + len(R.H_AT_37) + 2 and len(cs) == len(plain) + len(R.DROPOUT)
    # every NV, each with a partly live last vector and with a full one where H allows it
    assert {R.nv_of(c["H"]) for c in plain if c["H"] % 256} == {1, 2, 3, 4} and {R.nv_of(c["H"]) for c in plain if c["H"] % 256 == 0} >= {1, 3, 4}
    assert {c["H"] for c in plain} == {4, 12, 64, 132, 256, 260, 516, 768, 1020, 1024}
    # every geometry, both sides of each threshold, below one block's waves, past the 256-block cap with a remainder
    Ms = {c["M"] for c in plain}
    assert Ms >= {1, 3, 5, 37, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4097, 4100}
    assert {R.geometry(M)[0] for M in Ms} == {4, 8, 16}
    assert R.geometry(1023)[0] == 4 and R.geometry(1024)[0] == 8 and R.geometry(2047)[0] == 8 and R.geometry(2048)[0] == 16
    assert R.geometry(4095) == (16, 256) and 4095 < 16 * 256 < 4097 and 4100 == 4096 + 4 and R.geometry(3)[1] == 1
    # both reduce kernels behind every geometry
    for nwv in (4, 8, 16):
        assert {c["H"] % 64 == 0 for c in plain if R.geometry(c["M"])[0] == nwv} == {True, False}
    # every row kind, both eps, residual in half of the cases, dy with a zero row and 1e3 next to 1e-3, per-column gamma / beta
    for c in plain:
        if c["M"] >= 37:
            assert set(c["kind"]) == set(R.KINDS), c["name"]
            scales = np.abs(c["dy"]).max(axis=1)
            assert (scales == 0).any() and scales.max() > 1e3 and 0 < scales[scales > 0].min() < 1e-2
        assert min(len(set(c["gamma"].tolist())), len(set(c["beta"].tolist()))) >= 0.99 * c["H"]
        zero = [r for r, k in enumerate(c["kind"]) if k == "zero"]
        assert all(not c["x"][r].any() and (c["res"] is None or not c["res"][r].any()) for r in zero)
    assert {c["eps"] for c in plain} == {1e-12, 1e-6}
    assert abs(sum(c["res"] is not None for c in plain) - len(plain) / 2) <= 1
    assert {(c["p_pre"] > 0, c["p_post"] > 0) for c in R.dropout_cases()} == {(True, False), (False, True), (True, True)}
    assert {max(c["p_pre"], c["p_post"]) for c in R.dropout_cases()} == {0.1, 0.5}
    for c in R.dropout_cases():
        for f, p in ((c["fpre"], c["p_pre"]), (c["fpost"], c["p_post"])):
            assert (f is None) == (p == 0)
            if f is not None:
                assert 0 < (f == 0).sum() < f.size and set(np.unique(f).tolist()) == {0.0, float(R.inv_keep32(p))}
    # constant rows: the restatement is finite on them, and that is all that is asked
    cc = R.const_case()
    out = R.ln32(cc)
    assert all(np.isfinite(out[k]).all() for k in R.ROW_OUTPUTS + R.COL_OUTPUTS)


def test_pre_and_post_masks_of_a_case_are_independent_streams():
    c = R.cases()["both 1030x768 p 0.5/0.1"]
    kp, kq = c["fpre"] != 0, c["fpost"] != 0
    rp, rq = R.keep_rate4(0.5), R.keep_rate4(0.1)
    agree = float((kp == kq).mean())
    want = rp * rq + (1 - rp) * (1 - rq)
    sd = np.sqrt(want * (1 - want) / kp.size)
    assert abs(agree - want) <= 5 * sd, (agree, want, sd)
    one = R.mask_factors(c, one_key=True)
    assert float(((one[0] != 0) == (one[1] != 0)).mean()) > want + 50 * sd           # (what one key for both would look like)
