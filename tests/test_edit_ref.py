"""tests/edit_ref.py, pinned without a GPU: the float32 twins agree with the float64 forms, x = 0 gives 0, with a zero source and unit-length
features the directional form is prompt_set_ref's plain cosine, the wave-order sum is a sum — and the bars of tests/test_gpu_edit_ops.py bite:
each planted fault moves the result beyond the bar the GPU test uses at the same inputs (as tests/test_vit_block_ref.py shows for its bars).

Planted faults: a missing normalisation of f; the source row of view 0 used for every view; the anchor's mean taken over L instead of
n_lat L; a dropped layer."""
import numpy as np
import pytest

import edit_ref as E
import prompt_set_ref as PR

F32, F64 = np.float32, np.float64
DIR_SHAPES = [(5, 1, 1, 32), (5, 3, 5, 100), (1, 16, 4, 512), (5, 3, 16, 1024)]      # (P, V, T, D): a subset of the GPU test's grid
ANCHOR_SHAPES = [(5, 1, 64), (5, 4, 512), (5, 18, 64), (3, 18, 512)]                 # (P, n_lat, L)


def test_lane_sum_is_a_sum_in_wave_order():
    rng = np.random.default_rng(0)
    for D in (1, 63, 64, 65, 100, 1040):
        a = rng.standard_normal((3, D)).astype(F32)
        got = E.lane_sum(a)
        assert got.dtype == F32 and got.shape == (3,)
        np.testing.assert_allclose(got, a.astype(F64).sum(-1), rtol=0, atol=1e-5 * np.sqrt(D))
    # integers below 2^24 add exactly in any order: the order cannot be seen, the completeness can
    a = rng.integers(-1000, 1000, (4, 777)).astype(F32)
    np.testing.assert_array_equal(E.lane_sum(a), a.sum(-1))
    # the documented order, written out for one row: lane l adds l, l + 64, ...; then the butterfly
    row = rng.standard_normal(200).astype(F32)
    lanes = np.zeros(64, F32)
    for i in range(200):
        lanes[i % 64] = F32(lanes[i % 64] + row[i])
    for o in (32, 16, 8, 4, 2, 1):
        lanes = np.array([F32(lanes[l] + lanes[l ^ o]) for l in range(64)], F32)
    assert E.lane_sum(row).view(np.uint32) == lanes[0].view(np.uint32) and len(set(lanes.view(np.uint32).tolist())) == 1


@pytest.mark.parametrize("P,V,T,D", DIR_SHAPES)
def test_float32_twin_agrees_with_float64(P, V, T, D):
    feat, targets, weights, src = E.dir_inputs(P, V, T, D)
    r64, r32 = E.cosine_set_dir(feat, targets, weights, src), E.cosine_set_dir(feat, targets, weights, src, dt=F32)
    for name, a, b in zip(("view_sim", "set_sim", "sim"), r64, r32):
        assert b.dtype == F32 and a.shape == b.shape, name
        # |x| and |g| are of order sqrt(D) and 1: a cosine's float32 error is a few spacings of 1 / sqrt(D) per accumulated term
        np.testing.assert_allclose(b, a, rtol=0, atol=2e-6, err_msg=name)
    assert np.abs(r64[1]).max() > 0.02       # (not a comparison of zeros)


def test_directional_formula_by_hand():
    """One row, D = 3, against the section's formula evaluated term by term."""
    f, s, g = np.array([3.0, 0.0, 4.0]), np.array([0.0, 1.0, 0.0]), np.array([1.0, 2.0, 2.0])
    x = f / 5.0 - s                                       # (0.6, -1, 0.8)
    want = x @ g / (np.sqrt(x @ x) * 3.0)
    vs, ss, sim = E.cosine_set_dir(f.reshape(1, 1, 3), g.reshape(1, 3), [2.0], s.reshape(1, 3))
    np.testing.assert_allclose([vs[0, 0], ss[0, 0], sim[0]], [want] * 3, rtol=1e-15)
    vs, ss, sim = E.cosine_set_dir(f.reshape(1, 1, 3), g.reshape(1, 3), [-2.0], s.reshape(1, 3), dt=F32)
    np.testing.assert_allclose([vs[0, 0], ss[0, 0], -sim[0]], [want] * 3, rtol=3e-7)


@pytest.mark.parametrize("dt", [F64, F32])
def test_x_zero_gives_exactly_zero(dt):
    src = E.dyadic_unit_rows(3, 100)
    feat = np.stack([src * F32(2.0 ** k) for k in (-3, 0, 5)])                # [P = 3, V = 3, D]: exact positive multiples of the source rows
    _, targets, weights, _ = E.dir_inputs(3, 3, 5, 100)
    vs, ss, sim = E.cosine_set_dir(feat, targets, weights, src, dt=dt)
    assert not vs.any() and not ss.any() and not sim.any()
    # a source row made from a feature by unit_rows, in the twin's own arithmetic: the feature itself and its power-of-two multiples give 0
    raw = np.random.default_rng(2).standard_normal((3, 100)).astype(F32)
    src = E.unit_rows(raw, F32)
    feat = np.stack([raw, raw * F32(4.0), raw * F32(0.125)])
    vs, ss, sim = E.cosine_set_dir(feat, targets, weights, src, dt=F32)
    assert not vs.any() and not ss.any() and not sim.any()


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("V", [1, 3])
def test_zero_source_and_unit_features_give_the_plain_cosine(dt, V):
    feat = np.stack([E.dyadic_unit_rows(V, 100, seed=s) for s in range(5)])   # |f| = 1 exactly: f / |f| = f, and x = f - 0 = f
    _, targets, weights, _ = E.dir_inputs(5, V, 4, 100)
    got = E.cosine_set_dir(feat, targets, weights, np.zeros((V, 100), F32), dt=dt)
    want = PR.cosine_set(feat, targets, weights, dt=dt)
    for name, a, b in zip(("view_sim", "set_sim", "sim"), got, want):
        # the same quantity; the twins sum in different orders (a wave's against one term after the other)
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-15 if dt == F64 else 3e-7, err_msg=name)


@pytest.mark.parametrize("P,n_lat,L", ANCHOR_SHAPES)
def test_anchor_twin_agrees_and_the_anchor_itself_gives_zero(P, n_lat, L):
    w, a = E.anchor_inputs(P, n_lat, L)
    d64, d32 = E.latent_anchor(w, a), E.latent_anchor(w, a, dt=F32)
    assert d32.dtype == F32
    np.testing.assert_allclose(d32, d64, rtol=2e-6)
    np.testing.assert_allclose(d64, ((w.astype(F64) - a) ** 2).mean(axis=(1, 2)), rtol=1e-14)
    for dt in (F64, F32):
        assert not E.latent_anchor(np.broadcast_to(a, (3,) + a.shape), a, dt=dt).any()
    w1, a1 = E.anchor_inputs(P, n_lat, L, layered=False)                      # one row for every layer
    np.testing.assert_array_equal(E.latent_anchor(w1, a1, dt=F32), E.latent_anchor(np.repeat(w1[:, None], n_lat, 1), a1, dt=F32))


def test_assemble_F_edit_layouts():
    sim, d, dis, lp = np.array([0.25, -0.5]), np.array([0.5, 2.0]), np.array([0.5, 1.5]), np.array([0.125, 0.25])
    np.testing.assert_array_equal(E.assemble_F_edit(sim, d), [[-0.25, 0.5], [0.5, 2.0]])
    np.testing.assert_array_equal(E.assemble_F_edit(sim, d, anchor_lambda=2.0), [[0.75], [4.5]])
    np.testing.assert_array_equal(E.assemble_F_edit(sim, d, dis=dis, lp=lp), [[-0.25, 0.5, 0.125, 0.5], [0.5, 0.0, 0.25, 2.0]])
    np.testing.assert_array_equal(E.assemble_F_edit(sim, d, anchor_lambda=2.0, dis=dis, lp=lp, lp_lambda=4.0), [[1.25, 0.5], [5.5, 0.0]])
    c, w = np.array([[0.5, -0.25], [-0.125, -1.0]]), np.array([2.0, -1.0])
    np.testing.assert_array_equal(E.assemble_F_edit(None, d, set_sim=c, weights=w, dis=dis), [[-0.5, -0.25, 0.5, 0.5], [0.125, -1.0, 0.0, 2.0]])


# ---- the bars bite ----
def _beyond(name, faulty, ref64, ref32):
    tol = E.bar(ref64, ref32)
    err = float(np.abs(np.asarray(faulty, F64) - ref64).max())
    assert err > 10 * tol, "%s: a planted fault moves the result by %.3e, the bar is %.3e — the GPU test would not see it" % (name, err, tol)


@pytest.mark.parametrize("P,V,T,D", DIR_SHAPES)
def test_bar_catches_a_missing_normalisation_of_f(P, V, T, D):
    feat, targets, weights, src = E.dir_inputs(P, V, T, D)
    r64, r32 = E.cosine_set_dir(feat, targets, weights, src), E.cosine_set_dir(feat, targets, weights, src, dt=F32)
    f = feat.astype(F64)
    x = f - src[None]                                     # f, not f / |f|
    c = np.einsum("pvd,td->pvt", x, targets.astype(F64)) / (np.linalg.norm(x, axis=-1)[..., None] * np.linalg.norm(targets.astype(F64), axis=-1))
    _beyond("set_sim", c.mean(1), r64[1], r32[1])
    _beyond("view_sim", c[:, :, 0], r64[0], r32[0])


@pytest.mark.parametrize("P,V,T,D", [s for s in DIR_SHAPES if s[1] > 1])
def test_bar_catches_view_zeros_source_used_for_every_view(P, V, T, D):
    feat, targets, weights, src = E.dir_inputs(P, V, T, D)
    r64, r32 = E.cosine_set_dir(feat, targets, weights, src), E.cosine_set_dir(feat, targets, weights, src, dt=F32)
    bad = E.cosine_set_dir(feat, targets, weights, np.repeat(src[:1], V, 0))
    _beyond("set_sim", bad[1], r64[1], r32[1])
    _beyond("view_sim", bad[0][:, 1:], r64[0][:, 1:], r32[0][:, 1:])
    np.testing.assert_array_equal(bad[0][:, 0], r64[0][:, 0])      # (view 0 itself is right: the fault shows in the others only)


@pytest.mark.parametrize("P,n_lat,L", [s for s in ANCHOR_SHAPES if s[1] > 1])
def test_bar_catches_the_mean_over_L_and_a_dropped_layer(P, n_lat, L):
    w, a = E.anchor_inputs(P, n_lat, L)
    d64, d32 = E.latent_anchor(w, a), E.latent_anchor(w, a, dt=F32)
    sq = (w.astype(F64) - a) ** 2
    _beyond("mean over L", sq.sum(axis=(1, 2)) / L, d64, d32)
    _beyond("last layer dropped", sq[:, :-1].sum(axis=(1, 2)) / (n_lat * L), d64, d32)
    _beyond("first layer dropped", sq[:, 1:].sum(axis=(1, 2)) / (n_lat * L), d64, d32)
