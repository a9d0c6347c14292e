"""tests/lpips_ref.py against the reference's own LPIPS_VGG16 (tests/golden/lpips_modules.npz, written by golden/make_lpips_golden.py), and
the properties the engine's tests lean on.  CPU only."""
import numpy as np

import lpips_ref as R
from clip_glass_amd import synth


def _fixture():
    fx = np.load(R.FIXTURE)
    sd = synth.lpips_state(int(fx["seed"]))
    return fx, sd, [fx[k].astype(np.float32) for k in ("x32", "t32", "x64")]


def test_float64_reference_matches_the_reference_module():
    """The reference runs fp32: 1e-5 relative, the bar of the other *_ref pins."""
    fx, sd, (x32, t32, x64) = _fixture()
    assert "restated" in str(fx["layout_source"])
    for got, key in ((R.lpips(sd, x32, t32), "d_32"), (R.lpips(sd, x32, t32[:1]), "d_32_shared"), (R.lpips(sd, R.area(x64, 32), t32), "d_64")):
        want = fx[key].astype(np.float64)
        assert want.shape == (3,) and (want > 0).all()
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), key
    # Projector._scale_for_lpips (F.interpolate(mode="area")) of a 64 px image to 32 is the 2 x 2 box mean
    np.testing.assert_allclose(R.area(x64, 32)[0].numpy(), fx["area_64_0"], rtol=0, atol=1e-6)


def test_identical_images_give_zero_and_d_is_symmetric():
    _, sd, (x32, t32, _) = _fixture()
    assert (R.lpips(sd, x32, x32) == 0).all()
    assert (R.lpips(sd, x32, x32, storage16=True) == 0).all()
    a, b = R.lpips(sd, x32, t32), R.lpips(sd, t32, x32)
    np.testing.assert_allclose(a, b, rtol=1e-13, atol=0)


def test_all_zero_feature_rows_take_the_eps_path():
    f = np.zeros((2, 64, 1, 1))
    g = np.ones((2, 64, 1, 1))
    lin = np.full((64,), 1.0 / 64)
    assert (R.head_term(f, f, lin).numpy() == 0).all()
    np.testing.assert_allclose(R.head_term(f, g, lin).numpy(), 1.0 / 64, rtol=1e-9)      # |g_hat|^2 = 1, spread over 64 channels, weight 1 / 64 each


def test_synthetic_weights_keep_fp16_activations_in_range():
    """He-scaled convolutions: through 13 layers the largest activation stays far below fp16's 65504."""
    _, sd, (x32, _, _) = _fixture()
    assert set(sd) == {"lpips.features.%d.%s" % (i, s) for i, _, _ in synth.VGG16_CONVS for s in ("weight", "bias")} | {
        "lpips.lin.%d.weight" % k for k in range(5)}
    for k, c in enumerate(synth.LPIPS_SLICE_CHANNELS):
        lin = sd["lpips.lin.%d.weight" % k]
        assert lin.shape == (c,) and (lin >= 0).all() and (lin < 1.0 / c).all()
    extreme = np.concatenate([x32, np.ones((1, 3, 32, 32), np.float32), -np.ones((1, 3, 32, 32), np.float32)])
    assert R.max_activation(sd, extreme) < 1e4
    assert R.max_activation(synth.lpips_state(0), R.images(3, 2, 16)) < 1e4


def test_fp16_storage_costs_what_the_gpu_bar_assumes():
    """The storage-format emulation differs from float64 by a few 1e-5 relative on the GPU tests' inputs: the measured values those tests
    name (test_gpu_lpips.py) are reproduced here, so a change of inputs or weights cannot silently detach the bar from them."""
    import test_gpu_lpips as G
    for (x0, x1, sd), want in ((G.inputs_s32(), G.FP16_STORAGE_REL_S32), (G.inputs_s16(), G.FP16_STORAGE_REL_S16)):
        d64, d16 = R.lpips(sd, x0, x1), R.lpips(sd, x0, x1, storage16=True)
        rel = (np.abs(d16 - d64) / d64).max()
        assert rel <= want and rel >= 0.98 * want, rel
