"""CPU half of the attention op-level tests: the restatements of csrc/attn.hip and csrc/attn16.hip (tests/_attn_ref.py) stay inside the
caps that test_gpu_attn.py's bounds are derived from, the host masks are the kernels' streams, every mistake a rewrite of the kernels
could make moves a named case by at least 10 x the GPU bound of an output it corrupts, and the case table reaches every kernel, every
KB / NB instantiation, every threshold and every row kind.  No GPU, no torch."""
import numpy as np
import pytest

import _attn_ref as R


def test_float64_backward_is_the_derivative_of_the_float64_forward():
    """central differences of sum(dO * O) in q, k, v on a small cross case with a mask and dropout: the reference checks itself"""
    base = R.make_case("fd", "bf16", 5, 7, p=0.5, B=3, seed=900, rot=0)
    ref = R.attn64(base)
    assert (base["F"] == 0).any() and (base["F"] > 1).any()

    def loss(**kw):
        c = dict(base)
        c.update(kw)
        return float((R.attn64(c)["out"].reshape(-1, R.H) * base["do"].astype(np.float64)).sum())
    h = 1e-5
    for name, grad, picks in (("q", "dq", ((0, 0), (7, 70), (14, 127))), ("k", "dk", ((1, 3), (9, 64), (20, 100))), ("v", "dv", ((0, 5), (13, 99), (6, 127)))):
        for (r, col) in picks:
            up, dn = base[name].astype(np.float64), base[name].astype(np.float64)
            up[r, col] += h
            dn[r, col] -= h
            fd = (loss(**{name: up}) - loss(**{name: dn})) / (2 * h)
            want = ref[grad].reshape(-1, R.H)[r, col]
            assert abs(fd - want) <= 1e-6 * max(1.0, np.abs(ref[grad]).max()), (name, r, col, fd, want)


def test_restatements_are_inside_the_measured_caps():
    tab = R.measure()
    for path in tab:
        for name in R.OUTPUTS:
            print(f"[restatement vs float64] {path:9s} {name:3s} " + "  ".join(f"{k} {v:.2g} (cap {R.measured(path, name, k):.2g})" for k, v in sorted(tab[path][name].items())))
    for path in tab:
        for name in R.OUTPUTS:
            assert set(tab[path][name]) == set(R.MEASURED[path][name]), (path, name)
            for k, v in tab[path][name].items():
                m = R.measured(path, name, k)
                assert v <= m, (path, name, k, v, m)
                assert m <= 1.11 * v + 1e-12, (path, name, k, v, m)          # the caps are the measured values, not something wider
    # what the caps say: the well-conditioned rows of the fp32 path stay at a few roundings of fp32, of the bf16 path of bf16
    for name in R.OUTPUTS:
        for k in ("randn", "nomask", "ramp", "headmask"):
            assert R.cap("fp32", name, k) <= 1e-6, (name, k)
    for path in ("bf16", "bf16/bf16"):
        for name in ("out", "dv", "dk"):
            for k in ("randn", "nomask", "ramp", "headmask", "allmask", "lastonly"):
                assert R.cap(path, name, k) <= 5 * 2.0 ** -9, (path, name, k)
    assert R.cap("bf16", "out", "filler") == 0 and R.cap("bf16", "lse", "peaked") == 2.0 ** -9


def test_the_case_table_reaches_every_kernel_instantiation_threshold_and_kind():
    cs = list(R.cases().values())
    b16 = [c for c in cs if c["path"] == "bf16" and c["form"] == "pad"]
    single = [c for c in b16 if R.fwd_kernel(c) == "attn_s128_fwd_kernel"]
    assert {R.fwd_kb(c) for c in single} == {2, 4, 6, 8, 10, 12, 14, 16}
    assert {1, 128, 129} <= {c["Sq"] for c in single} and {1, 16, 17, 33, 65, 97, 129, 161, 193, 225, 256} <= {c["Sk"] for c in single}
    assert {(c["Sq"], c["Sk"]) for c in b16 if R.fwd_kernel(c) == "attn16_fwd_kernel"} >= {(1, 257), (65, 257), (64, 320)}
    s128 = [c for c in b16 if R.bwd_kernel(c) == "attn_s128_bwd_kernel"]
    assert {R.bwd_nb(c) for c in s128} == {2, 4, 6, 8} and {(16, 16), (33, 17), (17, 65), (128, 97), (97, 128)} <= {(c["Sq"], c["Sk"]) for c in s128}
    assert {(c["Sq"], c["Sk"]) for c in b16 if R.bwd_kernel(c) == "attn_wide_bwd_kernel"} >= {(129, 1), (1, 129), (129, 129), (197, 197), (224, 224), (224, 17)}
    assert {(c["Sq"], c["Sk"]) for c in b16 if R.bwd_kernel(c) == "attn16_bwd_kernel"} >= {(225, 225), (1, 225), (257, 64), (65, 257)}
    assert {(c["Sq"], c["Sk"]) for c in cs if c["path"] == "fp32"} == set(R.FP32_SHAPES)
    # dropout: every kernel at 0, 0.1 and 0.5; the family pairs; bf16 in / out on every bf16 kernel; a null mask on both paths
    for kern_of in (R.fwd_kernel, R.bwd_kernel):
        for kern in {kern_of(c) for c in cs}:
            assert {c["p"] for c in cs if kern_of(c) == kern} >= {0.0, 0.1, 0.5}, kern
            if kern not in ("attn_fwd_kernel", "attn_bwd_kernel"):
                assert any(c["io"] == "bf16" for c in cs if kern_of(c) == kern), kern
    fam = {(R.fwd_kernel(c), R.bwd_kernel(c)) for c in cs if c["p"] > 0}
    assert {("attn_s128_fwd_kernel", "attn_wide_bwd_kernel"), ("attn_s128_fwd_kernel", "attn16_bwd_kernel"), ("attn16_fwd_kernel", "attn16_bwd_kernel")} <= fam
    assert {c["path"] for c in cs if c["mask"] is None and c["form"] == "pad"} == {"fp32", "bf16"}
    assert {c["form"] for c in cs if c["p"] > 0} == {"pad", "vself", "vq", "vk"}
    assert any(c["form"] == "vself" and 0 in np.diff(c["cuq"]) for c in cs)
    assert any(c["form"] == f and c["pair_given"] and (c["pair"] < 0).any() for c in cs for f in ("vq",)) and any(c["form"] == "vk" and c["pair_given"] for c in cs)
    for c in cs:                                                  # every key side is named by at most one query sequence
        named = c["pair"][c["pair"] >= 0]
        assert len(set(named.tolist())) == len(named), c["name"]
        assert c["B"] >= 3
    # row kinds: every kind on every kernel's cases, the row maximum of a ramp row in the last 16 keys, a fully masked first tile
    for kern_of in (R.fwd_kernel, R.bwd_kernel):
        for kern in {kern_of(c) for c in cs}:
            assert {k for c in cs if kern_of(c) == kern for k in c["kind_q"]} >= set(R.KINDS), kern
    for c in cs:
        ref = R.attn64(c)
        for b, j, rq, rk in R.pairs(c):
            if j >= 0 and c["kind_k"][j] == "ramp":
                nk = rk.stop - rk.start
                for h in range(R.HEADS):
                    hs = slice(h * R.DH, (h + 1) * R.DH)
                    S = c["q"][rq, hs].astype(np.float64) @ c["k"][rk, hs].astype(np.float64).T * R.SCALE + c["mask"][j, :nk]
                    assert (S.argmax(axis=1) >= nk - 16).all(), c["name"]
            if j >= 0 and c["kind_k"][j] == "peaked" and rk.stop - rk.start > 1:
                l = ref["lse"][b, :, :rq.stop - rq.start]
                assert 10 < np.median(l) < 100, (c["name"], np.median(l))
    assert any(c["Sk"] > 64 and "headmask" in c["kind_k"] and (c["mask"][c["kind_k"].index("headmask"), :64] == R.MASKED).all() for c in cs)


def test_host_masks_are_the_kernels_streams():
    """keep rates of both streams against the exact rates of _smallops_ref, the two streams differ, 1 / (1 - p) in fp32"""
    for p in (0.1, 0.5):
        c16 = R.make_case("rate16", "bf16", 128, 128, p=p, B=8, seed=901)
        c32 = R.make_case("rate32", "fp32", 128, 128, p=p, B=8, seed=901)
        for c, rate in ((c16, R.keep_rate4(p)), (c32, R.keep_rate(p))):
            F = c["F"]
            n = F.size
            assert set(np.unique(F).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
            assert abs((F > 0).mean() - rate) <= 4 * np.sqrt(rate * (1 - rate) / n), (c["name"], p, (F > 0).mean(), rate)
        assert 0.3 * p < ((c16["F"] > 0) != (c32["F"] > 0)).mean() < 2.5 * p
        assert np.array_equal(R.factor_table(c16, stream32=True), c32["F"])
    # the packed forms hash (sequence index, descriptor Sq): the same seed and call id on a padded case of that Sq draw the same table
    v = R.cases()["packed self p 0.1 bf16io"]
    pad = R.make_case("pad", "bf16", 128, 128, p=0.1, B=v["B"], seed=902)
    assert np.array_equal(v["F"], pad["F"])


def _ratio(c, mut, output):
    errs = R.errors(c, R.restate(c, mut))
    return R.worst_ratio(c, {k: v for k, v in errs.items() if k[0] == output})[output][0]


# (mistake, switches, case, corrupted output)
MISTAKES = [
    ("dS without the dropout factor on dP", dict(ds_no_f=True), "bf16 129x1 p 0.1", "dq"),
    ("dS without the dropout factor on dP, fp32 path", dict(ds_no_f=True), "fp32 129x130 p 0.5", "dk"),
    ("delta from the undropped P", dict(delta_undropped=True), "bf16 197x197 p 0.1", "dq"),
    ("delta from the undropped P, seen in dk", dict(delta_undropped=True), "fp32 65x63 p 0.1", "dk"),
    ("mask hashed per key, not per group of four", dict(per_key=True), "bf16 97x128 p 0.5", "out"),
    ("mask hashed per key, seen in dv", dict(per_key=True), "bf16 225x225 p 0.1", "dv"),
    ("row hash built with Sk in place of Sq", dict(row_sk=True), "bf16 33x17 p 0.1", "out"),
    ("row hash built with Sk in place of Sq, packed", dict(row_sk=True), "packed q pair p 0.1", "dq"),
    ("h B + b in place of b heads + h", dict(hb_swap=True), "bf16 128x97 p 0.1", "out"),
    ("h B + b in place of b heads + h, fp32 path", dict(hb_swap=True), "fp32 63x65 p 0.1", "dv"),
    ("inv_keep left out", dict(no_inv_keep=True), "fp32 129x130 p 0.5", "out"),
    ("inv_keep left out, bf16 backward", dict(no_inv_keep=True), "bf16 65x257 p 0.5", "dv"),
    ("last key of a partial 16-block lost", dict(lose_last_key=True), "bf16 33x17", "out"),
    ("last key of a partial 16-block lost, tiled backward", dict(lose_last_key=True), "bf16 65x257", "dk"),
    ("padding keys scored 0 instead of -inf", dict(pad_zero=True), "bf16 224x17", "out"),
    ("padding keys scored 0, seen in lse", dict(pad_zero=True), "fp32 63x65", "lse"),
    ("mask row of sample b + 1", dict(mask_next=True), "bf16 17x65", "out"),
    ("mask row of sample b + 1, wide backward", dict(mask_next=True), "bf16 129x129", "dk"),
    ("online rescale alpha left out", dict(no_alpha=True), "bf16 65x257", "out"),
    ("online rescale alpha left out, fp32 path", dict(no_alpha=True), "fp32 129x130", "out"),
    ("(s + mask) scale", dict(mask_scaled=True), "bf16 16x16", "out"),
    ("(s + mask) scale, backward", dict(mask_scaled=True), "fp32 17x193", "dq"),
    ("dQ of the last key tile stored, not accumulated", dict(dq_last_tile=True), "bf16 225x225 bf16io", "dq"),
    ("dQ of the last key tile stored, fp32 path", dict(dq_last_tile=True), "fp32 63x65", "dq"),
    ("fp32-path stream on the bf16 path", dict(stream32=True), "bf16 197x197 p 0.1", "out"),
    ("fp32-path stream on the packed form", dict(stream32=True), "packed self p 0.1 bf16io", "dv"),
    ("dq masked with another draw than dk / dv", dict(dq_other_draw=True), "bf16 197x197 p 0.1", "dq"),
    ("dq masked with another draw, Sq != Sk", dict(dq_other_draw=True), "bf16 224x17 p 0.1", "dq"),
]


@pytest.mark.parametrize("what,mut,case,output", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_mistake_is_caught(what, mut, case, output):
    c = R.cases()[case]
    clean, wrong = _ratio(c, None, output), _ratio(c, mut, output)
    print(f"[{what}] {case}: {output} at {clean:.3g} x its GPU bound without, {wrong:.3g} x with the mistake")
    assert clean <= 1.0 / R.GPU_MARGIN + 1e-12, (what, case, output, clean)
    assert wrong > R.CAUGHT_FACTOR, (what, case, output, wrong)


def test_every_switch_of_the_restatement_is_listed():
    doc = R.restate.__doc__.split("`mut` switches the mistakes on:")[1]
    names = {w.strip(",") for line in doc.splitlines() for w in line.split()[1:]}
    assert names == {k for _, mut, _, _ in MISTAKES for k in mut}, names


def test_a_dq_only_mistake_leaves_the_other_outputs_alone():
    """the wide backward hashes the mask in both phases: a phase A with another draw moves dq and nothing else"""
    c = R.cases()["bf16 197x197 p 0.1"]
    assert R.bwd_kernel(c) == "attn_wide_bwd_kernel"
    a, b = R.restate(c), R.restate(c, dict(dq_other_draw=True))
    assert all(np.array_equal(a[k], b[k]) for k in ("out", "lse", "dk", "dv")) and not np.array_equal(a["dq"], b["dq"])
