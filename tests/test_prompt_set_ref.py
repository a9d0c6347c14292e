"""tests/prompt_set_ref.py (the float64 references of the prompt-set GPU tests) pinned on the CPU: its per-entry columns are
torch.cosine_similarity, one entry of weight 1 is small_ops_ref.cosine_views, the float32 twins compute the same thing, and the sign rule and
the normalisation by sum |w| give hand-computed answers.  Bars: tests/test_small_ops_ref.py's — 1e-12 * max|ref| against torch in float64 (its
cosine bar), 1e-4 * max|ref| for a twin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prompt_set_ref as PR
import small_ops_ref as R

F32 = np.float32


def _close(name, got, ref, rel):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= rel * float(np.abs(ref).max()), "%s: max err %.3e vs max|ref| %.3e" % (name, err, np.abs(ref).max())


def _inputs(P, V, T, D, seed=5):
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((P, V, D)).astype(F32)
    targets = rng.standard_normal((T, D)).astype(F32)
    weights = (rng.uniform(0.25, 2.0, T) * np.where(np.arange(T) % 3 == 1, -1.0, 1.0)).astype(F32)
    return feat, targets, weights


@pytest.mark.parametrize("V", [1, 3])
def test_columns_are_torch_cosine_similarity(V):
    P, T, D = 5, 4, 100
    feat, targets, weights = _inputs(P, V, T, D)
    feat[3] = 0                                            # a zero row: cosine 0, not nan
    view0, set_sim, sim = PR.cosine_set(feat, targets, weights)
    f64 = torch.from_numpy(feat.astype(np.float64)).reshape(P * V, D)
    ref = np.stack([F.cosine_similarity(f64, torch.from_numpy(targets[t].astype(np.float64)).view(1, -1), dim=1, eps=1e-8).numpy().reshape(P, V)
                    for t in range(T)], axis=2)            # [P, V, T]
    _close("per-entry columns", set_sim, ref.mean(axis=1), 1e-12)
    _close("entry 0 per view", view0, ref[:, :, 0], 1e-12)
    assert (set_sim[3] == 0).all() and sim[3] == 0
    want = (ref.mean(axis=1) * weights.astype(np.float64)).sum(axis=1) / np.abs(weights.astype(np.float64)).sum()
    _close("combination", sim, want, 1e-12)
    v32, s32, m32 = PR.cosine_set(feat, targets, weights, dt=F32)
    assert s32.dtype == F32 and m32.dtype == F32
    _close("columns float32 twin", s32, set_sim, 1e-4)
    _close("views float32 twin", v32, view0, 1e-4)
    _close("combination float32 twin", m32, sim, 1e-4)


@pytest.mark.parametrize("dt", [np.float64, F32])
@pytest.mark.parametrize("V", [1, 4])
def test_one_entry_of_weight_one_is_cosine_views_exactly(V, dt):
    feat, targets, _ = _inputs(6, V, 1, 64)
    view0, set_sim, sim = PR.cosine_set(feat, targets, [1.0], dt=dt)
    vs, mean = R.cosine_views(feat, targets[0], dt)
    np.testing.assert_array_equal(view0, vs)
    np.testing.assert_array_equal(set_sim[:, 0], mean)
    np.testing.assert_array_equal(sim, mean)


def test_known_answers_sign_rule_and_normalisation():
    # two candidates, three entries: exact binary fractions, so float32 and float64 agree to the bit
    c = np.array([[0.5, 0.25, -0.75], [-0.125, 1.0, 0.5]])
    w = np.array([2.0, -1.0, 0.5])
    for dt in (np.float64, F32):
        assert PR.weight_sum(w, dt) == 3.5
        # (2 * 0.5 - 0.25 - 0.375) / 3.5 and (-0.25 - 1 + 0.25) / 3.5
        np.testing.assert_array_equal(PR.combine(c, w, dt), np.array([0.375, -1.0], dt) / dt(3.5))
        # the sign of a weight flips the column back: a prompt to stay away from is minimised as +sim
        np.testing.assert_array_equal(PR.assemble_F_set(c, w, dt=dt), [[-0.5, 0.25, 0.75], [0.125, 1.0, -0.5]])
        Fv = PR.assemble_F_set(c[:, :2], w[:2], dis=[0.5, 1.5], lp=[0.125, 0.25], dt=dt)
        np.testing.assert_array_equal(Fv, [[-0.5, 0.25, 0.5, 0.125], [0.125, 1.0, 0.0, 0.25]])
        np.testing.assert_array_equal(PR.assemble_F_set(c[:, :2], w[:2], lp=[0.125, 0.25], dt=dt)[:, 2], [0.125, 0.25])
    # the magnitude of a weight has no meaning on a front; in the sum it has
    np.testing.assert_array_equal(PR.assemble_F_set(c, w * 7), PR.assemble_F_set(c, w))
    assert PR.combine(c, [1.0, 1.0, 1.0])[0] == 0.0 and PR.combine(c, [1.0, -1.0, 1.0])[0] == pytest.approx(-0.5 / 3)
    # an all-negative set: W stays positive, the best candidate is the one farthest away
    np.testing.assert_array_equal(PR.combine(c[:, :1], [-4.0]), [-0.5, 0.125])


def test_float32_twin_rounds_product_and_sum_separately():
    """The rule of include/glass.h: acc + w * c with two roundings.  A fused multiply-add would give another float32 here."""
    c = np.array([[F32(1) + F32(2.0 ** -12), F32(1)]], F32)
    w = np.array([F32(1) + F32(2.0 ** -12), F32(-1)], F32)
    prod = F32(w[0] * c[0, 0])                                        # rounded: 1 + 2^-11 (the 2^-24 term is lost)
    assert prod == F32(1) + F32(2.0 ** -11)
    want = F32(F32(F32(0) + prod) + F32(w[1] * c[0, 1])) / PR.weight_sum(w, F32)
    np.testing.assert_array_equal(PR.combine(c, w, F32), [want])
    exact = (float(w[0]) * float(c[0, 0]) - 1.0) / float(PR.weight_sum(w, np.float64))
    assert float(want) != exact                                        # the separate rounding is visible
