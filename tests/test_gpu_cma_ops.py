"""The sep-CMA-ES kernels (csrc/cmaes.hip) through the diagnostic ops, on caller-supplied state and F, against the float64 mirror of
tests/cma_ref.py.  Bars (cma_ref.check_sample / check_update): a sample within 1 fp32 ulp of the mirror's double rounded to fp32 (device
log / cos) and exactly the bound where the mirror clips; the rank exact; every state element within 1e-12 of the magnitudes of the terms it
is built from (contraction is off: only exp / pow and the summation order of ||p_sigma|| can differ); discrete outcomes exact."""
import os

import numpy as np
import pytest

import cma_ref as CR

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
XL, XU = -10.0, 10.0


def state_for(n, sigma, rng, ps_scale=0.3):
    st = CR.new_state(rng.uniform(-3.0, 3.0, n), rng.uniform(0.25, 4.0, n), sigma)
    st["ps"] = ps_scale * rng.uniform(0.9, 1.1, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)      # (a length that does not depend on luck)
    st["pc"] = 0.2 * rng.standard_normal(n)
    st["ps_norm"] = float(np.sqrt(CR.sum_squares(st["ps"])))
    return st


@pytest.mark.parametrize("lam,n", [(4, 1), (5, 3), (8, 64), (8, 65), (16, 512), (1024, 7), (8, 9216)])
def test_sample(lam, n):
    from clip_glass_amd import ops
    rng = np.random.default_rng(lam * 10007 + n)
    seed, g = 0x1234567890AB, 5
    st = state_for(n, 0.7, rng)
    full = ops.cma_sample(st["m"], st["d"], st["sigma"], lam, XL, XU, seed, g)
    CR.check_sample("sample %dx%d" % (lam, n), full, st, lam, XL, XU, seed, g)
    # a step large enough that the mirror clips at least a quarter of the elements: those are exactly xl or xu
    wide = dict(st, sigma=400.0)
    clipped = CR.check_sample("wide sample %dx%d" % (lam, n), ops.cma_sample(wide["m"], wide["d"], 400.0, lam, XL, XU, seed, g), wide, lam, XL, XU, seed, g)
    assert clipped >= 0.25, clipped
    # the same rows in pieces: bitwise equal, and the rows of the caller's array outside a piece come back untouched
    sentinel = np.float32(-123.25)
    cut = max(1, lam // 3)
    for row0, rows in ((0, cut), (cut, lam - cut)):
        piece = ops.cma_sample(st["m"], st["d"], st["sigma"], lam, XL, XU, seed, g, row0=row0, rows=rows, X=np.full((lam, n), sentinel, np.float32))
        assert np.array_equal(CR.bits(piece[row0:row0 + rows]), CR.bits(full[row0:row0 + rows]))
        outside = np.ones(lam, bool)
        outside[row0:row0 + rows] = False
        assert (piece[outside] == sentinel).all()
    # another generation or seed: other rows
    assert not np.array_equal(full, ops.cma_sample(st["m"], st["d"], st["sigma"], lam, XL, XU, seed, g + 1))


def awkward_F(lam, rng, nonfinite):
    """Few distinct values (ties), both zeros, and `nonfinite` rows of NaN / +inf / -inf."""
    F = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 0.25, 3.0, 1e-30, -1e30], np.float32), size=lam).astype(np.float32)
    bad = rng.choice(lam, size=nonfinite, replace=False)
    F[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=nonfinite)
    return F


@pytest.mark.parametrize("lam", [4, 5, 64, 1000, 1024])
def test_rank(lam):
    from clip_glass_amd import ops
    rng = np.random.default_rng(lam)
    for nonfinite, best in ((0, np.inf), (1, np.inf), (lam // 4, -1.5), (lam - lam // 2 + 1, np.inf), (lam, 0.0)):
        F = awkward_F(lam, rng, nonfinite)
        order, finite = CR.rank(F)
        got = ops.cma_rank(F, best)
        assert np.array_equal(got["order"], order), (lam, nonfinite)
        assert (got["finite"], got["nonfinite"]) == (finite, lam - finite) == (lam - nonfinite, nonfinite)
        updated = finite >= lam // 2
        assert (got["updated"], got["skipped"]) == (int(updated), int(not updated))
        improves = updated and float(F[order[0]]) < best      # strictly smaller: -0.0 does not beat 0.0
        assert got["best_src"] == (int(order[0]) if improves else -1)
        assert got["best_F"] == (float(F[order[0]]) if improves else best)
    # -0.0 against a best of 0.0: a tie, nothing replaced
    F = np.full(lam, 5.0, np.float32)
    F[lam - 1] = -0.0
    got = ops.cma_rank(F, 0.0)
    assert got["order"][0] == lam - 1 and got["best_src"] == -1 and got["best_F"] == 0.0


def as_op_state(st):
    return {k: st[k] for k in ("m", "d", "ps", "pc", "sigma", "ps_norm", "h", "finite", "updated", "skipped", "updates", "best_X", "best_F")}


def generation_rows(st, lam, rng, seed=9, g=4):
    X = CR.sample(st, lam, XL, XU, seed, g)
    F = rng.choice(np.linspace(-2.0, 2.0, max(lam // 2, 3)).astype(np.float32), size=lam).astype(np.float32)      # ties
    return X, F


@pytest.mark.parametrize("lam", [4, 5, 64])
@pytest.mark.parametrize("n", [1, 255, 257, 9216])
def test_update(n, lam):
    from clip_glass_amd import ops
    rng = np.random.default_rng(n * 131 + lam)
    seen = set()
    for want_h, ps_scale, g in ((1, 1e-3, 1000), (0, 30.0, 0)):      # a path far below and far above the threshold on ||p_sigma||
        st = state_for(n, 1.3, rng, ps_scale)
        st["best_F"], st["best_X"] = 0.5, rng.standard_normal(n).astype(np.float32)
        X, F = generation_rows(st, lam, rng, g=g)
        ref, mag = CR.update(st, X, F, lam, XL, XU, g)
        assert abs(ref["threshold_ratio"] - 1.0) > 1e-6 and ref["h"] == want_h, (ref["threshold_ratio"], ref["h"])
        got = ops.cma_update(X, F, as_op_state(st), XL, XU, g)
        CR.check_update("update n=%d lam=%d h=%d" % (n, lam, want_h), got, ref, mag)
        assert got["best_src"] == ref["best_src"]
        seen.add(got["h"])
        again = ops.cma_update(X, F, as_op_state(st), XL, XU, g)      # the same call twice: identical bits
        for k in ("m", "d", "ps", "pc", "best_X", "order"):
            assert np.array_equal(CR.bits(got[k]), CR.bits(again[k])), k
        assert (got["sigma"], got["ps_norm"], got["best_F"]) == (again["sigma"], again["ps_norm"], again["best_F"])
    assert seen == {0, 1}


def test_update_hits_both_sigma_clamps():
    from clip_glass_amd import ops
    n, lam = 257, 5
    rng = np.random.default_rng(77)
    for sigma, ps_scale, clamp in ((1.001e-10, 1e-3, 1e-10), (19.5, 30.0, XU - XL)):
        st = state_for(n, sigma, rng, ps_scale)
        if clamp == 1e-10:      # a mean that is exact in fp32 and far from 0: at this step every row rounds to it, y = 0 and the step shrinks
            st["m"] = (np.where(st["m"] < 0, -1.0, 1.0) * (0.5 + np.abs(st["m"]))).astype(np.float32).astype(float)
        X, F = generation_rows(st, lam, rng)
        ref, mag = CR.update(st, X, F, lam, XL, XU, 4)
        assert ref["sigma"] == clamp and ref["sigma_free"] != clamp, (ref["sigma_free"], clamp)
        got = ops.cma_update(X, F, as_op_state(st), XL, XU, 4)
        assert got["sigma"] == clamp
        CR.check_update("clamp %g" % clamp, got, ref, mag)


@pytest.mark.parametrize("n,lam", [(257, 5), (9216, 64)])
def test_update_without_mu_finite_rows_moves_nothing(n, lam):
    from clip_glass_amd import ops
    rng = np.random.default_rng(5)
    st = state_for(n, 0.9, rng)
    st["best_F"], st["best_X"], st["skipped"], st["updates"], st["h"] = 0.5, rng.standard_normal(n).astype(np.float32), 3, 7, 1
    X, F = generation_rows(st, lam, rng)
    F[rng.choice(lam, size=lam - lam // 2 + 1, replace=False)] = np.nan      # mu - 1 finite rows
    got = ops.cma_update(X, F, as_op_state(st), XL, XU, 4)
    ref, mag = CR.update(st, X, F, lam, XL, XU, 4)
    CR.check_update("skipped", got, ref, mag)
    for k in ("m", "d", "ps", "pc", "best_X"):
        assert np.array_equal(CR.bits(got[k]), CR.bits(st[k])), k
    assert (got["sigma"], got["ps_norm"], got["best_F"], got["h"]) == (st["sigma"], st["ps_norm"], st["best_F"], 1)
    assert (got["skipped"], got["updates"], got["updated"], got["finite"], got["best_src"]) == (4, 7, 0, lam // 2 - 1, -1)
