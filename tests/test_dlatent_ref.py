"""Pins tests/dlatent_ref.py — the oracle's composition of the latent spaces and the truncation trick — to what the reference's own
Generator computed (tests/golden/dlatent_modules.npz, written by tests/golden/make_dlatent_golden.py), and, where the reference is present,
to the imported reference directly.  Tolerances: those of tests/test_oracle_vs_reference.py for the generator."""
import numpy as np
import pytest
import torch

import dlatent_ref as R
import ref_harness as rh
from oracle import stylegan2_ref as sg


def _t(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(R.FIXTURE))


@pytest.fixture(scope="module")
def inputs():
    sd, z, avg, planes = R.fixture_inputs()
    return _t(sd), z, avg, [torch.tensor(p) for p in planes]


def _close(got, ref):
    got = got.numpy() if hasattr(got, "numpy") else np.asarray(got)
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-4 * float(np.abs(ref).max()))


def _helper_outputs(inputs, w_plus):
    tsd, z, avg, planes = inputs
    nf = lambda i: planes
    with torch.no_grad():
        out = {"w": sg.g_mapping(tsd, torch.tensor(z)).numpy()}
        for name, (psi, cutoff) in R.MODES.items():
            out["img_z_" + name] = R.synthesize(tsd, z, 4, nf, space="z", psi=psi, cutoff=cutoff, avg=avg).numpy()
        out["img_w"] = R.synthesize(tsd, out["w"], 4, nf, space="w").numpy()
        out["img_w_plus"] = R.synthesize(tsd, w_plus.reshape(4, -1), 4, nf, space="w+").numpy()
        out["img_w_plus_psi05_cut3"] = R.synthesize(tsd, w_plus.reshape(4, -1), 4, nf, space="w+", psi=0.5, cutoff=3, avg=avg).numpy()
    return out


def test_fixture_inputs_are_the_helpers(fx):
    sd, z, avg, planes = R.fixture_inputs()
    np.testing.assert_array_equal(fx["z"], z)
    np.testing.assert_array_equal(fx["dlatent_avg"], avg)
    assert np.abs(avg).min() > 0
    for i, p in enumerate(planes):
        np.testing.assert_array_equal(fx["noise_%d" % i], p)
    np.testing.assert_array_equal(fx["w_plus"], R.fixture_w_plus(fx["w"]))
    assert fx["w_plus"].shape == (4, 8, 32)
    rows = fx["w_plus"][0]
    assert all(not np.array_equal(rows[i], rows[j]) for i in range(8) for j in range(i))     # eight differing rows


@pytest.mark.parametrize("key", ["w", "img_z_psi07", "img_z_psi05_cut3", "img_w", "img_w_plus", "img_w_plus_psi05_cut3"])
def test_helper_matches_the_reference_fixture(fx, inputs, key):
    _close(_helper_outputs(inputs, fx["w_plus"])[key], fx[key])


def test_modes_differ(fx):
    """The pins would hold trivially if truncation or the per-layer rows changed nothing."""
    keys = ["img_z_psi07", "img_z_psi05_cut3", "img_w", "img_w_plus", "img_w_plus_psi05_cut3"]
    for i, a in enumerate(keys):
        for b in keys[:i]:
            assert np.abs(fx[a] - fx[b]).max() > 1e-2, (a, b)


def test_layer_psi_table():
    assert R.layer_psi(8, 1.0, None) is None and R.layer_psi(8, 0.7, 0) is None
    np.testing.assert_array_equal(R.layer_psi(8, 0.5, 3), np.array([.5, .5, .5, 1, 1, 1, 1, 1], np.float32))
    np.testing.assert_array_equal(R.layer_psi(8, 0.7, None), np.full(8, 0.7, np.float32))


@pytest.mark.reference
@pytest.mark.skipif(not rh.available(), reason="the reference is not on this machine")
def test_helper_matches_the_imported_reference(fx, inputs):
    import make_dlatent_golden as G
    ref = G.reference_outputs()
    got = _helper_outputs(inputs, ref["w_plus"])
    for key, v in got.items():
        _close(v, ref[key])
        _close(ref[key], fx[key])                                # the committed fixture is what the reference gives today
