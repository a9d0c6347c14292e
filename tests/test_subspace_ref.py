"""tests/subspace_ref.py against itself, and subspace.pca_basis: the error bar admits a numpy fp32 emulation of the kernel's FMA chain and
rejects every planted fault; the PCA recovers a planted subspace.  No GPU, no built library."""
import numpy as np
import pytest

import subspace_ref as S
from clip_glass_amd import subspace

SHAPES = [(32, 8, 3), (32, 8, 32), (64, 10, 1), (64, 10, 17)]      # (L, n_lat, K)


@pytest.mark.parametrize("L,n_lat,K", SHAPES)
@pytest.mark.parametrize("groups", ["one", "per_layer", "two_frozen_ends", "split_frozen_middle"])
def test_bar_passes_the_fp32_chain(L, n_lat, K, groups):
    lg = S.layer_groups(n_lat)[groups]
    c, B, base = S.case(5, L, n_lat, K, lg, 5)
    ref, bar = S.expand(c, lg, B, base)
    got = S.expand_f32(c, lg, B, base)
    ok, worst, n_bad = S.within(got, ref, bar)
    print("[subspace_ref] L%d n_lat%d K%d %s: worst err / bar %.3f" % (L, n_lat, K, groups, worst))
    assert ok, "%d elements outside the bar (worst ratio %.3f)" % (n_bad, worst)
    frozen = lg < 0
    assert not bar[:, frozen].any() and (bar[:, ~frozen] > 0).all()
    np.testing.assert_array_equal(got[:, frozen], np.broadcast_to(base[frozen], got[:, frozen].shape))


@pytest.mark.parametrize("psi,cutoff", [(0.5, 3), (0.3, None), (0.7, 5)])
def test_bar_passes_the_fp32_chain_under_truncation(psi, cutoff):
    """The lerp of dlatent_expand_kernel emulated in fp32 on top of the fp32 chain stays inside bar_psi; an untouched layer keeps bar."""
    L, n_lat, K = 32, 8, 9
    lg = S.layer_groups(n_lat)["two_frozen_ends"]
    c, B, base = S.case(6, L, n_lat, K, lg, 4)
    avg = np.random.RandomState(1).normal(size=L).astype(np.float32)
    ref, bar = S.expand(c, lg, B, base, psi=psi, cutoff=cutoff, avg=avg)
    ref1, bar1 = S.expand(c, lg, B, base)
    b = S.expand_f32(c, lg, B, base)
    w = S.layer_psi(n_lat, psi, cutoff).astype(np.float32)
    got = np.empty_like(b)
    for l in range(n_lat):
        d = (b[:, l] - avg).astype(np.float32)
        lo = w[l] < 0.5
        v = S._fma32(np.full_like(d, w[l] if lo else w[l] - np.float32(1)), d, np.broadcast_to(avg, d.shape) if lo else b[:, l])
        got[:, l] = b[:, l] if w[l] == 1 else v
    ok, worst, n_bad = S.within(got, ref, bar)
    assert ok, "%d elements outside the bar (worst ratio %.3f)" % (n_bad, worst)
    keep = w == 1
    np.testing.assert_array_equal(ref[:, keep], ref1[:, keep])
    np.testing.assert_array_equal(bar[:, keep], bar1[:, keep])
    assert (bar[:, ~keep] > 0).all()         # a truncated layer is never a copy, frozen or not


@pytest.mark.parametrize("fault", S.FAULTS)
def test_bar_fails_on_a_planted_fault(fault):
    L, n_lat, K = 32, 8, 5
    lg = S.layer_groups(n_lat)["two_frozen_ends"]
    c, B, base = S.case(7, L, n_lat, K, lg, 5)
    ref, bar = S.expand(c, lg, B, base)
    assert S.within(S.expand_f32(c, lg, B, base), ref, bar)[0]
    ok, worst, n_bad = S.within(S.expand_f32(c, lg, B, base, fault=fault), ref, bar)
    assert not ok and n_bad > L, "the bar did not notice %s (worst ratio %.3f)" % (fault, worst)


def test_a_zero_row_is_the_base_and_rows_are_independent():
    L, n_lat, K = 32, 8, 4
    lg = S.layer_groups(n_lat)["split_frozen_middle"]
    c, B, base = S.case(8, L, n_lat, K, lg, 3)
    c[1] = 0
    out = S.expand_f32(c, lg, B, base)
    np.testing.assert_array_equal(out[1], base)
    np.testing.assert_array_equal(S.expand_f32(c[2:], lg, B, base)[0], out[2])
    ref, bar = S.expand(c, lg, B, base)
    np.testing.assert_array_equal(ref[1], base.astype(np.float64))


# ---- pca_basis ------------------------------------------------------------------------------------------------------
def _planted(seed=3, N=256, L=32, r=5):
    rng = np.random.RandomState(seed)
    Q = np.linalg.qr(rng.normal(size=(L, r)))[0]                       # orthonormal columns: the planted span
    coef = rng.normal(size=(N, r)) * np.array([5.0, 4.0, 3.0, 2.0, 1.0])
    return coef @ Q.T + rng.normal(size=L), Q


def test_pca_recovers_a_planted_rank_5_subspace():
    x, Q = _planted()
    mean, comp, std = subspace.pca_basis(x, 5)
    assert mean.dtype == comp.dtype == std.dtype == np.float64 and comp.shape == (5, 32) and std.shape == (5,)
    assert np.linalg.norm(comp.T @ comp - Q @ Q.T) < 1e-9              # the projectors agree (Frobenius)
    np.testing.assert_allclose(mean, x.mean(axis=0), rtol=0, atol=1e-12)
    proj = (x - mean) @ comp.T
    np.testing.assert_allclose(std, proj.std(axis=0, ddof=1), rtol=0, atol=1e-9)
    assert (np.diff(std) <= 0).all()
    assert np.abs(comp @ comp.T - np.eye(5)).max() < 1e-12
    big = np.argmax(np.abs(comp), axis=1)
    assert (comp[np.arange(5), big] > 0).all()
    again = subspace.pca_basis(x.copy(), 5)
    for a, b in zip((mean, comp, std), again):
        assert a.tobytes() == b.tobytes()


def test_pca_refuses_too_many_components():
    x, _ = _planted(N=8)
    with pytest.raises(ValueError, match=r"min\(L, N - 1\) = 7"):
        subspace.pca_basis(x, 8)
    with pytest.raises(ValueError, match=r"K must be in"):
        subspace.pca_basis(x, 0)
    with pytest.raises(ValueError, match=r"\[N >= 2, L\]"):
        subspace.pca_basis(x[0], 1)
    subspace.pca_basis(x, 7)
