"""CPU half of the op-level tests of the packed attention forms with 129 .. 256 tokens on a side (tests/_attn_long_ref.py): the
restatement stays inside the committed caps, the caps are the measured values merged with _attn_ref's, the case list reaches both query
chunks, key blocks 9 .. 16 and every edge named below, and every mistake a 256-row rewrite of the packed kernels could make moves an
output of a named case past CAUGHT_FACTOR x its GPU bound.  No GPU, no torch."""
import numpy as np
import pytest

import _attn_long_ref as LR
import _attn_ref as R


def test_restatement_is_inside_the_committed_caps():
    new, merged = R.measure(LR.long_cases()), LR.merged_measure()
    for path in merged:
        for name in R.OUTPUTS:
            print(f"[long restatement vs float64] {path:9s} {name:3s} " + "  ".join(f"{k} {v:.2g} (cap {LR.MEASURED[path][name][k]:.2g})" for k, v in sorted(new[path][name].items())))
    assert set(new) == set(LR.MEASURED) == {"bf16", "bf16/bf16"}
    for path in merged:
        for name in R.OUTPUTS:
            assert set(merged[path][name]) == set(LR.MEASURED[path][name]), (path, name)
            for k, v in merged[path][name].items():
                m = LR.MEASURED[path][name][k]
                assert v <= m, (path, name, k, v, m)
                assert m <= 1.11 * v + 1e-12, (path, name, k, v, m)      # the merged maximum, not something wider
            for k, m in R.MEASURED[path][name].items():
                assert LR.MEASURED[path][name][k] >= m                    # never below the table of the short cases
    with LR.long_caps():
        for c in LR.long_cases():
            for name, (r, kind) in R.worst_ratio(c, R.errors(c, R.restate(c))).items():
                assert r <= 1.0 / R.GPU_MARGIN + 1e-12, (c["name"], name, kind, r)
    assert R.MEASURED["bf16"]["dq"]["headmask"] == 0.0084                 # the block put _attn_ref's table back


def test_the_case_list_reaches_the_long_paths_and_their_edges():
    cs = list(LR.cases().values())
    assert 5 <= len(cs) <= 8 and all(c["path"] == "bf16" and c["B"] < 10 and LR.bwd_kernel(c) == "attn_wide_bwd_kernel<packed>" for c in cs)
    assert all(R.fwd_kernel(c) == "attn_s128_fwd_kernel" for c in cs)
    assert LR.bwd_kernel(LR.short_case()) == "attn_s128_bwd_kernel"
    assert {c["form"] for c in cs} == {"vself", "vq", "vk"} and {c["io"] for c in cs} == {"f32", "bf16"}
    assert {c["p"] for c in cs} == {0.0, 0.1, 0.5}
    assert {R.fwd_kb(c) for c in cs} >= {6, 10, 16}                        # 70, 140 and 250 / 256 keys
    lens_q = {int(n) for c in cs for n in np.diff(c["cuq"])}
    lens_k = {int(n) for c in cs for n in np.diff(c["cuk"])}
    assert {0, 1, 17, 128, 129, 144, 250, 256} <= lens_q and {0, 1, 3, 129, 130, 250, 256} <= lens_k
    assert any(n > 128 and n % 16 for n in lens_q) and any(n > 128 and n % 16 for n in lens_k)
    assert {(n + 15) // 16 for n in lens_k if n > 128} >= {9, 16}        # the first and the last of the key blocks 9 .. 16
    assert any(c["form"] == "vself" and c["Sq"] == 256 for c in cs) and any(c["form"] == "vself" and c["Sq"] == 250 and c["io"] == "bf16" for c in cs)
    vq = [c for c in cs if c["form"] == "vq"]
    assert any(c["pair_given"] and (c["pair"] < 0).any() and c["Sq"] > 128 and c["Sk"] <= 128 for c in vq)
    assert any(not c["pair_given"] and c["n_pairs"] < c["B"] and c["Sk"] > 128 and c["Sq"] <= 128 for c in vq)      # the visual side above 128
    vk = [c for c in cs if c["form"] == "vk"]
    assert any(c["pair_given"] and (c["pair"] < 0).any() and c["Sq"] <= 128 for c in vk) and any(c["Sq"] > 128 and c["Sk"] > 128 for c in vk)
    assert any(c["form"] == "vk" and any(c["cuk"][j + 1] == c["cuk"][j] for j in c["pair"] if j >= 0) for c in cs)  # a named, empty key side
    for c in cs + [LR.nan_case()]:                                        # every key side is named by at most one query sequence
        named = c["pair"][c["pair"] >= 0]
        assert len(set(named.tolist())) == len(named), c["name"]
        assert c["B"] >= 3
        kq, kk, _ = R.row_kinds(c)                                       # every row kind has a cap
        for name, kinds in (("out", kq), ("lse", kq), ("dq", kq), ("dk", kk), ("dv", kk)):
            assert set(kinds) <= set(LR.MEASURED[R.path_key(c)][name]), (c["name"], name)
    assert {k for c in cs for k in c["kind_q"]} >= set(R.KINDS) | {"filler"}
    n = LR.nan_case()
    assert n["B"] == 3 and np.diff(n["cuq"])[1] > 128 and all(x % 16 for x in np.diff(n["cuq"])) and n["p"] > 0


def _ratio(c, got, output):
    errs = R.errors(c, got)
    return R.worst_ratio(c, {k: v for k, v in errs.items() if k[0] == output})[output][0]


SWITCHES = [
    ("last key of a partial 16-block lost", dict(lose_last_key=True), "long self 250 bf16io", "out"),
    ("last key of a partial 16-block lost, seen in dk", dict(lose_last_key=True), "long k 70x250 pair p 0.1", "dk"),
    ("mask hashed per key, not per group of four", dict(per_key=True), "long self 256 p 0.1", "out"),
    ("mask hashed per key, seen in dv", dict(per_key=True), "long k 200x256 p 0.5 bf16io", "dv"),
    ("row hash built with Sk in place of Sq", dict(row_sk=True), "long q 250x70 pair p 0.1", "dq"),
    ("row hash built with Sk in place of Sq, packed keys", dict(row_sk=True), "long k 70x250 pair p 0.1", "dv"),
    ("mask row of sample b + 1", dict(mask_next=True), "long q 250x70 pair p 0.1", "out"),
    ("mask row of sample b + 1, 140 keys", dict(mask_next=True), "long q 128x140 fillers behind p 0.1 bf16io", "dk"),
]
LONG = [
    ("keys from 128 on ignored", LR.keys_from_128_ignored, "long self 256 p 0.1", "out"),
    ("keys from 128 on ignored, seen in dk", LR.keys_from_128_ignored, "long k 70x250 pair p 0.1", "dk"),
    ("keys from 128 on ignored, 140 keys", LR.keys_from_128_ignored, "long q 128x140 fillers behind p 0.1 bf16io", "dq"),
    ("query rows from 128 on draw chunk 0's dropout rows", LR.chunk1_draws_chunk0, "long q 250x70 pair p 0.1", "out"),
    ("query rows from 128 on draw chunk 0's dropout rows, seen in dq", LR.chunk1_draws_chunk0, "long self 256 p 0.1", "dq"),
    ("query rows from 128 on draw chunk 0's dropout rows, seen in dv", LR.chunk1_draws_chunk0, "long k 200x256 p 0.5 bf16io", "dv"),
    ("query rows from 128 on take chunk 0's statistics", LR.chunk1_takes_chunk0_statistics, "long self 250 bf16io", "lse"),
    ("query rows from 128 on left unwritten", LR.chunk1_unwritten, "long self 250 bf16io", "out"),
    ("query rows from 128 on left unwritten, seen in lse", LR.chunk1_unwritten, "long q 250x70 pair p 0.1", "lse"),
]


@pytest.mark.parametrize("what,mut,case,output", SWITCHES, ids=[m[0] for m in SWITCHES])
def test_switch_mistake_is_caught(what, mut, case, output):
    c = LR.cases()[case]
    with LR.long_caps():
        clean, wrong = _ratio(c, R.restate(c), output), _ratio(c, R.restate(c, mut), output)
    print(f"[{what}] {case}: {output} at {clean:.3g} x its GPU bound without, {wrong:.3g} x with the mistake")
    assert clean <= 1.0 / R.GPU_MARGIN + 1e-12, (what, case, output, clean)
    assert wrong > R.CAUGHT_FACTOR, (what, case, output, wrong)


@pytest.mark.parametrize("what,wrong_fn,case,output", LONG, ids=[m[0] for m in LONG])
def test_long_sequence_mistake_is_caught(what, wrong_fn, case, output):
    c = LR.cases()[case]
    with LR.long_caps():
        clean, wrong = _ratio(c, R.restate(c), output), _ratio(c, wrong_fn(c), output)
    print(f"[{what}] {case}: {output} at {clean:.3g} x its GPU bound without, {wrong:.3g} x with the mistake")
    assert clean <= 1.0 / R.GPU_MARGIN + 1e-12, (what, case, output, clean)
    assert wrong > R.CAUGHT_FACTOR, (what, case, output, wrong)
