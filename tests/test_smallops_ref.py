"""CPU half of the loss / dropout / small-reduction op-level tests.  Before test_gpu_losses.py and test_gpu_smallops.py rely on the cases
and bounds of tests/_smallops_ref.py, this file shows that
  1. the kernels' arithmetic restated in numpy float32 (same order of operations) stays inside the bounds on every case, and prints its
     worst errors: the module constants *_MEASURED, from which the GPU bounds are taken (8 x), are caps on what is printed here;
  2. every mistake the GPU half is meant to catch moves at least one case by ten times its bound or more;
  3. the integer restatement of the counter-based RNG is a sound generator: keep rates, row and column means of a mask, and the
     independence of two call ids and of two epochs."""
import math

import numpy as np
import pytest

import _smallops_ref as R


# ---------------------------------------------------------------------------------------------- 1. the fp32 restatement
def test_cases_have_what_the_gpu_half_needs():
    ce = {c["name"]: c for c in R.ce_cases()}
    assert [(c["R"], c["C"]) for c in R.ce_cases()][:7] == [(5, 1), (7, 37), (4, 255), (4, 256), (4, 257), (19, 1003), (6, 30522)]
    assert ce["7x37 in 40"]["ld"] == 40 and ce["19x1003 in 1008"]["ld"] == 1008 and ce["6x30522 empty_rows"]["ld"] % 4 == 0
    sap = ce["7x37 in 40"]["x"]
    assert (np.isinf(sap).sum(axis=1) == 37 // 2).sum() >= 3                  # half the columns of some rows are -inf
    labels = np.concatenate([c["label"] for c in R.ce_cases()])
    assert {-100, -1, 0}.issubset(set(labels.tolist())) and any((c["label"] == c["C"] - 1).any() for c in R.ce_cases())
    for c in R.ce_cases():
        if c["R"] >= 7:                                                        # the upstream weights: 0, a negative one, 1e-3 next to 1e3
            g = c["g"].tolist()
            assert 0.0 in g and min(g) < 0 and any(a == np.float32(1e-3) and b == np.float32(1e3) for a, b in zip(g, g[1:]))
        want, _, _ = R.ce_f64(c["x"], c["label"])
        for r, (kind, lab) in enumerate(zip(c["kinds"], c["labs"])):
            if lab == "ninf":
                assert want[r] == np.inf
            elif kind == "one" and lab == "fin":
                assert want[r] == 0.0 and np.isfinite(c["x"][r]).sum() == 1
            else:
                assert np.isfinite(want[r])
    kinds = {k for c in R.kl_cases() for k in c["kinds"]}
    assert kinds == {"softmax", "third_zero", "onehot", "zero", "half_mass"}
    assert any(c["t"].dtype == np.float64 for c in R.kl_cases()) and [(c["R"], c["C"]) for c in R.kl_cases()][::2] == [(3, 1), (11, 40), (4, 257), (5, 1000)]
    for c in R.kl_cases():
        for r, k in enumerate(c["kinds"]):
            s = c["t32"][r].astype(np.float64).sum()
            assert {"zero": s == 0, "half_mass": abs(s - 0.5) < 1e-6, "third_zero": (c["t32"][r] == 0).sum() == c["C"] // 3}.get(k, abs(s - 1) < 1e-6), (c["name"], r)


def test_fp32_restatement_is_inside_the_bounds():
    """prints the worst errors of the fp32 restatement; the *_MEASURED constants of _smallops_ref.py are caps on them, the GPU bounds 8 x"""
    worst_l = worst_t = 0.0
    for c in R.ce_cases():
        loss, dx = R.ce32(c["x"], c["label"], c["g"])
        el, et = R.ce_errors(c, loss, dx)
        print(f"[ce fp32 restatement] {c['name']}: loss {el.max():.3f} units, dx / g {et.max():.3f} units")
        worst_l, worst_t = max(worst_l, el.max()), max(worst_t, et.max())
    print(f"[ce fp32 restatement] worst: loss {worst_l:.3f} (cap {R.CE_LOSS_MEASURED}), dx / g {worst_t:.3f} (cap {R.CE_TERM_MEASURED})")
    assert worst_l <= R.CE_LOSS_MEASURED and worst_t <= R.CE_TERM_MEASURED
    assert worst_l >= R.CE_LOSS_MEASURED / 2 and worst_t >= R.CE_TERM_MEASURED / 2      # (caps, not slack: within 2 x of what is measured)
    worst_l = worst_t = 0.0
    for c in R.kl_cases():
        loss, dx = R.kl32(c["x"], c["t32"], c["g"])
        el, et = R.kl_errors(c, loss, dx)
        print(f"[kl fp32 restatement] {c['name']}: loss {el.max():.3f} units, dx / g {et.max():.3f} units")
        worst_l, worst_t = max(worst_l, el.max()), max(worst_t, et.max())
    print(f"[kl fp32 restatement] worst: loss {worst_l:.3f} (cap {R.KL_LOSS_MEASURED}), dx / g {worst_t:.3f} (cap {R.KL_TERM_MEASURED})")
    assert worst_l <= R.KL_LOSS_MEASURED and worst_t <= R.KL_TERM_MEASURED
    assert worst_l >= R.KL_LOSS_MEASURED / 2 and worst_t >= R.KL_TERM_MEASURED / 2
    h, g = R.act_block()
    e = R.dgelu_errors(h, g, g * R.dgelu32(h)).max()
    print(f"[gelu' fp32 restatement] worst {e:.3f} eps32 |g| (cap {R.DGELU_MEASURED})")
    assert R.DGELU_MEASURED / 2 <= e <= R.DGELU_MEASURED
    assert set(np.float32(R.ACT_SPECIALS).tolist()) <= set(h.tolist()) and np.signbit(h[1]) and h[1] == 0


def test_single_rounded_ops_agree_with_float64_rounded_once():
    """the 'exact fp32 statements' are what a correctly rounded fp32 operation gives: float64 arithmetic rounded once (two roundings for
    the two-operation ones)"""
    x, t, g = R.mse_case(257)
    d = (x.astype(np.float64) - t).astype(np.float32)
    assert np.array_equal(R.mse32(x, t), (d.astype(np.float64) ** 2).astype(np.float32))
    assert np.array_equal(R.mse_bwd32(x, t, g), (2.0 * g.astype(np.float64) * d).astype(np.float32))
    assert float(R.inv_keep32(0.5)) == 2.0 and float(R.inv_keep32(0.1)) == float(np.float32(1.0 / float(np.float32(1) - np.float32(0.1))))
    m = R.extend_mask32(np.array([0, 1, 2, 255], dtype=np.uint8))
    assert m[0] == -10000.0 and (m[1:] == 0).all() and np.signbit(m[1:]).all()
    assert np.array_equal(R.bf16_bits(np.array([0x3F808000, 0x3F818000, 0x3F808001], dtype=np.uint32).view(np.float32)),
                          np.array([0x3F80, 0x3F82, 0x3F81], dtype=np.uint16))          # ties to even, both ways; just above a tie


# ---------------------------------------------------------------------------------------------- 2. the mistakes
def _ce_worst(**mut):
    """worst error / bound over the CE cases (loss, dx / g) of a mistaken restatement"""
    wl = wt = 0.0
    for c in R.ce_cases():
        x = c["x"]
        if mut.get("row_stride_c"):                  # row r read at r C instead of r ldx
            x = c["buf"].reshape(-1)[:c["R"] * c["C"]].reshape(c["R"], c["C"])
        loss, dx = R.ce32(x, c["label"], c["g"], **{k: v for k, v in mut.items() if k != "row_stride_c"})
        el, et = R.ce_errors(c, loss, dx)
        wl, wt = max(wl, el.max() / R.CE_LOSS_BOUND), max(wt, et.max() / R.CE_TERM_BOUND)
    return wl, wt


CE_MISTAKES = {"no max subtraction": dict(sub_max=False), "tail columns dropped": dict(drop_tail=True), "wave 0 dropped": dict(drop_wave=0),
               "wave 1 dropped": dict(drop_wave=1), "wave 2 dropped": dict(drop_wave=2), "wave 3 dropped": dict(drop_wave=3),
               "row r read at r C": dict(row_stride_c=True), "label off by one": dict(label_shift=1)}


@pytest.mark.parametrize("name", list(CE_MISTAKES))
def test_ce_mistake_exceeds_the_bound_tenfold(name):
    wl, wt = _ce_worst(**CE_MISTAKES[name])
    print(f"[ce mistake] {name}: loss {wl:.3g} x bound, dx / g {wt:.3g} x bound")
    assert wl >= 10 and wt >= 10


def test_ce_ignored_row_with_the_ordinary_gradient_exceeds_the_bound():
    wl, wt = _ce_worst(ignore=False)
    assert wl <= 1 / 8 and wt >= 10                  # (the loss is untouched by this one)


def test_ce_scale_3_alone_cannot_see_a_missing_max():
    """why the cases go beyond N(0, 1) * 3: there, a kernel without the max subtraction is inside the bound"""
    for c in R.ce_cases():
        keep = [r for r, k in enumerate(c["kinds"]) if k == "s3" and c["label"][r] >= 0]
        if not keep or c["C"] < 37:
            continue
        sub = dict(c, R=len(keep), x=c["x"][keep], label=c["label"][keep], g=c["g"][keep], kinds=["s3"] * len(keep), labs=[c["labs"][r] for r in keep])
        el, _ = R.ce_errors(sub, *R.ce32(sub["x"], sub["label"], sub["g"], sub_max=False))
        assert el.max() <= R.CE_LOSS_BOUND, c["name"]


@pytest.mark.parametrize("name,mut", [("gradient without sum(t)", dict(with_tsum=False)), ("t log t at 0 as NaN", dict(nan_at_zero=True))])
def test_kl_mistake_exceeds_the_bound_tenfold(name, mut):
    wl = wt = 0.0
    for c in R.kl_cases():
        el, et = R.kl_errors(c, *R.kl32(c["x"], c["t32"], c["g"], **mut))
        wl, wt = max(wl, el.max() / R.KL_LOSS_BOUND), max(wt, et.max() / R.KL_TERM_BOUND)
    print(f"[kl mistake] {name}: loss {wl:.3g} x bound, dx / g {wt:.3g} x bound")
    assert max(wl, wt) >= 10 and (wt >= 10 if "with_tsum" in mut else wl >= 10)


def test_tanh_gelu_exceeds_the_bound_tenfold():
    h, g = R.act_block()
    e = R.dgelu_errors(h, g, g.astype(np.float64) * R.dgelu_tanh_f64(h)).max() / R.DGELU_BOUND
    print(f"[gelu' mistake] tanh approximation: {e:.3g} x bound")
    assert e >= 10
    assert np.array_equal(R.drelu(np.array([0.0, -0.0, 1e-20, -1e-20], dtype=np.float32), np.ones(4, np.float32)), [0, 0, 1, 0])


@pytest.mark.parametrize("M", R.COLSUM_M)
def test_colsum_mistakes_exceed_the_bound_tenfold(M):
    for N in R.COLSUM_N:
        c = R.colsum_case(M, N, "bf16")
        want, bound = R.colsum_f64(c["x"], c["out0"], True), R.colsum_bound(c["x"], c["out0"])
        assert (np.abs(R.colsum_f64(c["x"]) - want) >= 10 * bound).all(), "accumulate ignored"
        want, bound = R.colsum_f64(c["x"]), R.colsum_bound(c["x"])
        as_half = R.fp16_value(c["bits"][:, 3:3 + N])
        with np.errstate(invalid="ignore"):
            d = np.abs(as_half.sum(axis=0) - want)
        assert (np.isnan(d) | (d >= 10 * bound)).any(), "bf16 bits read as fp16"
        if M > 1:                                    # the strided view: rows read at stride N instead of ldx
            wrong = c["buf"].reshape(-1)[3:3 + M * N].reshape(M, N)
            assert (np.abs(wrong.astype(np.float64).sum(axis=0) - want) >= 10 * bound).any(), "row stride"
    assert [R.chunk_chain(m) for m in (1, 64, 65, 4095, 4096, 4097)] == [1 + 2 + 1 + 2, 16 + 2 + 1 + 2, 9 + 2 + 1 + 2, 16 + 2 + 16 + 2, 16 + 2 + 16 + 2, 17 + 2 + 16 + 2]


@pytest.mark.parametrize("K", R.SMALLK_K)
def test_smallk_wgrad_mistakes_exceed_the_bound_tenfold(K):
    for M in R.SMALLK_M[1:]:
        for N in R.SMALLK_N:
            c = R.smallk_case(M, N, K)
            want, bound = R.smallk_wgrad_f64(c["dy"], c["x"]), R.smallk_bound(c["dy"], c["x"])
            wrong_x = c["xb"].reshape(-1)[1:1 + M * K].reshape(M, K)              # x read at stride K instead of ldx
            assert (np.abs(R.smallk_wgrad_f64(c["dy"], wrong_x) - want) >= 10 * bound).any()
            acc = R.smallk_wgrad_f64(c["dy"], c["x"], c["dw0"], True)
            assert (np.abs(want - acc) >= 10 * R.smallk_bound(c["dy"], c["x"], c["dw0"])).any()


# ---------------------------------------------------------------------------------------------- 3. the RNG restatement
N_DRAWS = 1 << 20
KEYS = [(cid, epoch) for cid in (1, 77, 78) for epoch in (0, 1)]


def test_mix32_and_key_are_32_bit():
    assert R.mix32_int(0) == 0 and R.mix32_int(1) == int(R.mix32(np.array([1]))[0]) < 2 ** 32
    x = np.array([0, 1, 0xFFFFFFFF, 0x9E3779B9, 12345], dtype=np.uint64)
    assert [R.mix32_int(int(v)) for v in x] == R.mix32(x).tolist()
    assert len(set(R.mix32(np.arange(1 << 16)).tolist())) == 1 << 16                  # a bijection: no collisions
    assert len({R.rng_key(R.SEED, e, c) for c, e in KEYS}) == len(KEYS)
    assert R.rng_key(R.SEED + (5 << 32), 0, 1)[0] == R.rng_key(R.SEED, 0, 1)[0] and R.rng_key(R.SEED + (5 << 32), 0, 1)[1] != R.rng_key(R.SEED, 0, 1)[1]


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_rates(p):
    q, q4 = R.keep_rate(p), R.keep_rate4(p)
    assert abs(q - (1 - p)) < 1e-7 and abs(q4 - (1 - p)) < 2e-5
    for cid, epoch in KEYS:
        key = R.rng_key(R.SEED, epoch, cid)
        z = (R.drop_keep(key, N_DRAWS, p).mean() - q) / math.sqrt(q * (1 - q) / N_DRAWS)
        z4 = (R.drop_keep4(key, 1024, 1024, p).mean() - q4) / math.sqrt(q4 * (1 - q4) / N_DRAWS)
        print(f"[rng] p {p} call {cid} epoch {epoch}: keep rate {z:+.2f} sigma (drop_scale), {z4:+.2f} sigma (drop_scale4)")
        assert abs(z) <= 4 and abs(z4) <= 4


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_mask_rows_columns_and_independence(p):
    q = R.keep_rate4(p)
    key = R.rng_key(R.SEED, 0, 77)
    m = R.drop_keep4(key, 1024, 1024, p)
    sd = math.sqrt(q * (1 - q) / 1024)
    zr, zc = np.abs(m.mean(axis=1) - q).max() / sd, np.abs(m.mean(axis=0) - q).max() / sd
    print(f"[rng] p {p}: worst row mean {zr:.2f} sigma, worst column mean {zc:.2f} sigma")
    assert zr <= 6 and zc <= 6
    a = q * q + (1 - q) * (1 - q)
    sa = math.sqrt(a * (1 - a) / N_DRAWS)
    for what, other in (("call ids 77 / 78", R.rng_key(R.SEED, 0, 78)), ("epochs 0 / 1", R.rng_key(R.SEED, 1, 77))):
        z4 = ((m == R.drop_keep4(other, 1024, 1024, p)).mean() - a) / sa
        q1 = R.keep_rate(p)
        a1 = q1 * q1 + (1 - q1) * (1 - q1)
        z1 = ((R.drop_keep(key, N_DRAWS, p) == R.drop_keep(other, N_DRAWS, p)).mean() - a1) / math.sqrt(a1 * (1 - a1) / N_DRAWS)
        print(f"[rng] p {p}: masks of {what} agree {z4:+.2f} sigma (drop_scale4), {z1:+.2f} sigma (drop_scale) from q^2 + (1 - q)^2")
        assert abs(z4) <= 4 and abs(z1) <= 4


def test_the_dropout_case_holds_a_draw_on_the_threshold():
    """u == p exactly at one element of the GPU half's p = 0.5 launches: `u > p` instead of `u >= p` flips it"""
    key = R.rng_key(R.SEED, 0, R.CALL_ID)
    n = 2048 * 256 + 7
    assert R.TIE_INDEX < n
    a, b = R.drop_keep(key, n, 0.5), R.drop_keep(key, n, 0.5, u_gt_p=True)
    assert a[R.TIE_INDEX] and not b[R.TIE_INDEX] and (a != b).sum() == 1
    assert np.array_equal(R.drop_keep(key, 1000, 0.5), a[:1000])                     # the factor depends on the element, not on the launch size
    f = R.drop_scale(key, 1000, 0.1)
    assert set(np.unique(f).tolist()) == {0.0, float(R.inv_keep32(0.1))}
