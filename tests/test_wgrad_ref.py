"""CPU: tests/_wgrad_ref.py tells a wrong grouped weight-gradient launch from a right one.  On the problems test_gpu_wgrad.py launches, a
right fp32 computation (every k-tile rounded once, summed in k-tile order) stays inside the bounds, and every seeded mistake moves at
least one element (row, slot) by >= 10 x the bound in every tile class -- 64, 128 and 256 rows -- in which its mechanism exists."""
import numpy as np
import pytest

import _wgrad_ref as R


def test_statement_agrees_with_a_plain_loop():
    for p in (R.prob(3, 5, 64, 64, kv=37, acc=1, db=2, seed=1), R.prob(2, 3, 64, 64, K2=64, kv2=9, db=1, seed=2)):
        dy, x, dy2, x2 = R.values(p)
        _, _, _, _, dw0, db0 = R.operands(p.M, p.N, p.K, p.K2, p.seed)
        dw = [[float(dw0[m, n]) if p.acc else 0.0 for n in range(p.N)] for m in range(p.M)]
        db = [float(db0[m]) if p.db == 2 else 0.0 for m in range(p.M)]
        for a, b, kv in ((dy, x, R.kv_of(p)), (dy2, x2, R.kv2_of(p))):
            for k in range(kv):
                for m in range(p.M):
                    db[m] += float(a[k, m])
                    for n in range(p.N):
                        dw[m][n] += float(a[k, m]) * float(b[k, n])
        W = R.want_and_bounds(p)
        assert np.allclose(W["dw"], np.array(dw), rtol=1e-13, atol=0) and np.allclose(W["db"], np.array(db), rtol=1e-12, atol=1e-12)
        assert np.array_equal(W["dw"], R.wgrad_f64(dy, x, dw0, bool(p.acc), R.kv_of(p), dy2, x2, R.kv2_of(p) if p.K2 else None))
        mag = np.abs(dy[:R.kv_of(p)]).T @ np.abs(x[:R.kv_of(p)]) + (np.abs(dy2[:p.kv2]).T @ np.abs(x2[:p.kv2]) if p.K2 else 0.0) + (np.abs(dw0) if p.acc else 0.0)
        assert np.allclose(W["dw_bound"], R.EPS32 * (R.kv_of(p) + R.kv2_of(p) + 3) * mag, rtol=1e-14, atol=0)


def test_operands_are_bf16_with_positive_products_and_finite_padding():
    p = R.prob(65, 129, 192, 64, kv=159, K2=128, kv2=95, seed=3)
    dyb, xb, dy2b, x2b = R.padded(p, "nan")
    assert dyb.dtype == np.uint16 and dyb.shape == (192, 65) and xb.shape == (192, 129) and dy2b.shape == (128, 65) and x2b.shape == (128, 129)
    assert np.isnan(R.bf16_value(dyb[159:])).all() and np.isnan(R.bf16_value(x2b[95:])).all() and np.isfinite(R.bf16_value(dyb[:159])).all()
    dy, x, dy2, x2 = R.values(p)
    assert all(np.isfinite(a).all() for a in (dy, x, dy2, x2))
    assert (dy[:, :, None] * x[:, None, :3] > 0).all() and (dy2[:, :, None] * x2[:, None, :3] > 0).all()
    heavy = np.abs(dy[:128]).reshape(2, 64, 65).min(axis=1) >= 0.5
    assert heavy.any(axis=1).all()


def test_ss_layout_and_units():
    assert R.ss_layout(65, 129, 64, 128).all() and R.ss_layout(65, 129, 64, 128).shape == (2, 2)
    assert R.ss_layout(314, 384, 128, 128).tolist() == [[True] * 3, [False] * 3, [True] * 3, [False] * 3, [True] * 3]
    assert R.ss_layout(314, 384, 256, 256).tolist() == [[True, False, True], [False] * 3, [False] * 3, [False] * 3, [True, False, True]]
    dw = np.arange(130 * 257, dtype=np.float64).reshape(130, 257)
    for bm in (64, 128, 256):
        ss = R.ss_f64(dw, bm, R.bn_of(bm))
        assert ((ss != 0) == R.ss_layout(130, 257, bm, R.bn_of(bm))).all() and np.isclose(ss.sum(), (dw ** 2).sum(), rtol=1e-14)
    for bm, (M, N) in R.UNIT_SHAPES.items():
        un = R.units(M, N, bm)
        cover = np.zeros((M, N), dtype=int)
        for m_lo, mr, n_lo, nc in un:
            assert m_lo % bm == 0 and n_lo % R.bn_of(bm) == 0 and -(-mr // bm) * -(-nc // R.bn_of(bm)) <= R.UNIT_TILES
            cover[m_lo:m_lo + mr, n_lo:n_lo + nc] += 1
        assert (cover == 1).all() and 1 < len(un) <= -(-M // 64)
        assert len({u[2] for u in un}) > 1, "the unit cases need more than one column unit"
    assert R.units(64, 128, 64) == [(0, 64, 0, 128)] and R.units(257, 255, 256) == [(0, 257, 0, 255)]


def test_case_tables_hold_what_they_are_meant_for():
    for setting, (env, bm) in R.SETTINGS.items():
        cs = dict(R.cases(setting))
        assert all(set(env) <= set(R.ENV_NAMES) for env, _ in R.SETTINGS.values())
        shapes = {(p.M, p.N) for p in cs["edges-a"]}
        assert shapes == set(R.EDGES)
        if setting in ("auto", "auto128"):
            assert list(cs) == ["edges-a"] and {p.rows for p in cs["edges-a"]} == {bm}
            continue
        every = [p for ps in cs.values() for p in ps]
        assert {p.K for p in every} >= ({128, 192, 320} if bm == 256 else {64, 128, 192, 320})
        for K in (128, 192, 320):
            assert {p.kv for p in cs["k-valid"] if p.K == K} == set(R.k_valid_positions(K)) and len(R.k_valid_positions(K)) in (7, 9)
        assert {p.fill for p in cs["k-valid"]} == set(R.FILLS)
        assert {(p.K, p.K2) for p in cs["second-pair"]} == set(R.PAIRS)
        for K, K2 in R.PAIRS:      # K2_valid at the same positions relative to K2, and every row counting
            assert {p.kv2 for p in cs["second-pair"] if (p.K, p.K2) == (K, K2)} == {0} | set(R.k_valid_positions(K2)), (K, K2)
        assert R.k_valid_positions(64) == [63, 33, 32, 31, 1] and R.k_valid_positions(320) == [319, 289, 288, 287, 257, 256, 65, 64, 1]
        assert {(p.acc, bool(p.db)) for p in cs["second-pair"]} == {(0, True), (0, False), (1, True), (1, False)}
        assert any(p.wire and len(R.units(p.M, p.N, bm)) > 1 for p in cs["units"]) and any(p.db == 2 for p in cs["units"])
        assert len(cs["one-tile"]) == 1 and len(R.units(*cs["one-tile"][0][:2], bm)) == 1
        if bm == 256:
            # demotion: keff / keff2 of one k-tile next to neighbours that stay on the 256 class, and a call with both classes
            for cid in ("k-valid", "second-pair", "both-classes"):
                assert {p.rows for p in cs[cid]} == {256, 64}, cid
            assert all(p.rows == (256 if R.takes_256(p) else 64) for p in every)
            assert any(p.K2 and R.keff(R.kv_of(p)) >= 128 and R.keff(R.kv2_of(p)) == 64 for p in cs["second-pair"])
            assert {R.keff(R.kv_of(p)) // 64 for p in cs["p8-nk2-nk3"]} == {2, 3}
        if setting in ("64", "128", "256"):
            assert R.table_entries(cs["long-table"], lambda p: p.rows) > R.WG_MAX


CLASS = {bm: R.class_probs(bm) for bm in (64, 128, 256)}


@pytest.mark.parametrize("bm", [64, 128, 256])
def test_right_sum_is_inside_the_bounds_and_every_mistake_leaves_them(bm):
    probs = CLASS[bm]
    assert len(probs) >= 60
    shown, could, beyond_2_9 = set(), set(), 0
    for p in probs:
        W = R.want_and_bounds(p)
        assert (W["dw_bound"] > 0).all() and (W["db_bound"] > 0).all()
        dw32, db32 = R.restate32(p)
        assert dw32.dtype == np.float32
        assert (np.abs(dw32 - W["dw"]) <= W["dw_bound"]).all() and (np.abs(db32 - W["db"]) <= W["db_bound"]).all()
        ref = {"dw": (W["dw"], W["dw_bound"]), "db": (W["db"], W["db_bound"])}
        if p.wire:
            wire32 = R.bf16_value(R.bf16_bits((np.float32(p.wire) * dw32).astype(np.float32))).astype(np.float64)
            assert (np.abs(wire32 - W["wire"]) <= W["wire_bound"]).all()
            # 2^-9 |wire_scale want| in place of the binade's half-ulp is no bound: correctly rounded values leave it
            beyond_2_9 += int((np.abs(wire32 - W["wire"]) > abs(p.wire) * W["dw_bound"] + 2.0 ** -9 * np.abs(W["wire"])).sum())
            ref["wire"] = (W["wire"], W["wire_bound"])
        if p.ss:
            ss_want = R.ss_f64(W["dw"], bm, R.bn_of(bm))
            ss32 = np.zeros_like(ss_want)
            for m0 in range(0, p.M, bm):          # an fp32 sum in another order than the kernel's: the bound does not depend on the order
                for n0 in range(0, p.N, R.bn_of(bm)):
                    ss32[m0 // 64, n0 // 128] = np.sum(W["dw"][m0:m0 + bm, n0:n0 + R.bn_of(bm)].astype(np.float32) ** 2, dtype=np.float32)
            ss_of32 = R.ss_f64(W["dw"].astype(np.float32), bm, R.bn_of(bm))
            assert (np.abs(ss32 - ss_of32) <= R.ss_bound(ss_of32, bm)).all() and ((ss_want != 0) == R.ss_layout(p.M, p.N, bm, R.bn_of(bm))).all()
            ref["ss"] = (ss_want, R.ss_bound(ss_want, bm))
        for name, q in R.MISTAKES.items():
            got = R.mistaken(name, p, bm)
            if got is None:
                continue
            could.add(name)
            want, bound = ref[q]
            assert got.shape == want.shape, name
            moved = ~(np.abs(got - want) < 10 * bound)      # (a NaN has left the bound)
            assert moved.any(), (name, p, float(np.nanmax(np.abs(got - want) / bound)))
            shown.add(name)
    assert beyond_2_9 > 0
    assert could == set(R.MISTAKES), set(R.MISTAKES) - could
    assert shown == set(R.MISTAKES), set(R.MISTAKES) - shown
