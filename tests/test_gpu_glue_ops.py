"""The StyleGAN2 glue kernels (csrc/kernels_misc.hip: toRGB + skip, the two FIR blurs, fromRGB, the noise planes), one at a time through the
diagnostic ABI (clip_glass_amd.ops) against the float64 references of tests/glue_ops_ref.py under their derived elementwise bars —
tests/test_glue_ops_ref.py pins the references to the oracle and shows on these very inputs that a FIR tap of 0.374, a clamped border row,
swapped upsample weights, a wrong sample's smax, a wrong channel group's weights, a missing clamp and a slope of 0.25 all fail the bars.

Kernel instances reached: torgb_pix_kernel<16|32|64>, torgb_kernel<16|32|64> (C = 128, 256, 512), each with and without the skip image;
blur_kernel<2,1,16> pixel-major, in 32-channel planes with groups fastest (C = 32, 128) and re-dealt (C = 256: P = 8; C = 512: P = 4);
blur_kernel<1,2,8>; fromrgb_kernel with 8 .. 128 output channels (128: 71 680 bytes of dynamic LDS); noise_kernel.

The ops stage their outputs poisoned (every byte 0xFF: NaN) with guard elements behind them, so an element no thread stores fails
check_bound's finiteness assertion and a store behind the output fails the op.

Not covered: the second iteration of toRGB's grid-stride loop.  It needs hw > 2048 x the pixels of a workgroup-iteration, at least a
512 x 512 map at C = 128 (130 MB of features), and no shipped model reaches it.  Non-square maps: the ops and every caller are square.

Measured on an MI355X (the worst |err| / tol of each kernel over all its cases; a margin under a derived bar, not a bar):
  toRGB     0.086 (C = 16, H = 20, with skip; 0.01 .. 0.09 over the 25 runs)
  blur      0.993 pad 2 (H = 33, C = 512; the plane form returns the same bits), 0.987 pad 1 + ::2 (H = 16, C = 512)
  fromRGB   0.995 (Cout = 128, R = 16)
The fp16 outputs sit just under 1 by construction: the bar's leading term is the half ulp of the store, which some element of a large
tensor comes arbitrarily close to; what is left above it (32 resp. 16 sqrt 2 float32 roundings of A) is the room for the arithmetic.
fromRGB at Cout = 128 launched as it is (no opt-in attribute set) and is right at every element; the noise planes lie within 4.8e-7 of the
numpy mirror."""
import os

import numpy as np
import pytest

import glue_ops_ref as R
from clip_glass_amd import ops, synth
from util import check, check_bound

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]


# ---- toRGB -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("H", R.TORGB_H)
@pytest.mark.parametrize("C", R.TORGB_C)
def test_torgb(C, H, with_skip):
    a = R.torgb_inputs(C, H, with_skip)
    assert len(set(a[4].tolist())) == 3                       # smax differs per sample
    ref, A = R.torgb(*a)
    check_bound("torgb C%d H%d skip%d" % (C, H, with_skip), ops.torgb(*a), ref, R.tol_torgb(C, A))


def test_torgb_refuses_a_width_without_instance():
    x, wrgb, bias, sn, smax, yprev = R.torgb_inputs(16, 4, True)
    with pytest.raises(RuntimeError, match="toRGB: channel width not instantiated"):
        ops.torgb(np.concatenate([x, x[..., :8]], axis=-1), np.concatenate([wrgb, wrgb[:, :8]], axis=1), bias,
                  np.concatenate([sn, sn[:, :8]], axis=1), smax, yprev)                                       # C = 24
    ref, A = R.torgb(x, wrgb, bias, sn, smax, yprev)                   # and the device is as it was: the next launch computes
    check_bound("torgb C16 H4 after the refusal", ops.torgb(x, wrgb, bias, sn, smax, yprev), ref, R.tol_torgb(16, A))


# ---- blur ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", R.BLUR_PAD2)
def test_blur_pad2(H, C):
    x = R.blur_inputs(H, C)
    ref, A = R.blur(x, 2, 1)
    check_bound("blur pad2 H%d C%d" % (H, C), ops.blur(x, 0), ref, R.tol_blur(ref, A))


@pytest.mark.parametrize("H", R.BLUR_PLANAR_H)
@pytest.mark.parametrize("C", R.BLUR_PLANAR_C)
def test_blur_pad2_planar32(C, H):
    x = R.blur_inputs(H, C)
    ref, A = R.blur(x, 2, 1)
    got = ops.blur(x, 2)                                     # (un-permuted from [B,C/32,H+1,H+1,32] by the wrapper)
    check_bound("blur pad2 planar32 H%d C%d" % (H, C), got, ref, R.tol_blur(ref, A))
    np.testing.assert_array_equal(got, ops.blur(x, 0))


@pytest.mark.parametrize("H,C", R.BLUR_DOWN)
def test_blur_down(H, C):
    x = R.blur_inputs(H, C)
    ref, A = R.blur(x, 1, 2)
    check_bound("blur down H%d C%d" % (H, C), ops.blur(x, 1), ref, R.tol_blur(ref, A))


# ---- fromRGB ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_", R.FROMRGB_R)
@pytest.mark.parametrize("Cout", R.FROMRGB_COUT)
def test_fromrgb(Cout, R_):
    y, w, bias = R.fromrgb_inputs(Cout, R_)
    assert all((y == v).any() for v in (-1.0, 1.0, 1.5, -1.5, 0.0))
    ref, A = R.fromrgb(y, w, bias)
    check_bound("fromrgb Cout%d R%d" % (Cout, R_), ops.fromrgb(y, w, bias), ref, R.tol_fromrgb(ref, A))


# ---- noise -----------------------------------------------------------------------------------------------------------------------------
SEED, GEN, LAYER, MB0 = 0x1234567890, 7, 5, 2


def _mirror(side, n_mb, seed=SEED, gen=GEN, layer=LAYER, mb0=MB0):
    return np.stack([synth.noise_plane(seed, gen, mb0 + m, layer, side, side).reshape(-1) for m in range(n_mb)])


@pytest.mark.parametrize("side", [4, 5, 128])            # one thread (the first layer); hw = 25: the q * 4 + j < hw guard; 64 workgroups
def test_noise_matches_numpy_mirror(side):
    got = ops.noise(3, side * side, layer=LAYER, mb0=MB0, generation=GEN, seed=SEED)
    check("philox noise vs numpy %dx%d" % (side, side), got, _mirror(side, 3), 0, atol=2e-5)
    if side == 128:                                      # (the mirror's planes pass the same check: confirmed on the CPU for this seed)
        for m in range(3):
            assert abs(got[m].mean()) < 0.03 and abs(got[m].std() - 1) < 0.03, (m, got[m].mean(), got[m].std())


def test_noise_plane_addressing():
    hw = 128 * 128
    got = ops.noise(3, hw, layer=LAYER, mb0=MB0, generation=GEN, seed=SEED)
    for m in range(3):                                   # plane mb0 + m of a launch is the one-plane launch at mb0 + m
        np.testing.assert_array_equal(got[m], ops.noise(1, hw, layer=LAYER, mb0=MB0 + m, generation=GEN, seed=SEED)[0])
    base = got[0]
    for name, kw in (("layer", dict(layer=LAYER + 1)), ("generation", dict(generation=GEN + 1)), ("seed, low word", dict(seed=SEED + 1)),
                     ("seed, high word", dict(seed=SEED + (1 << 32)))):
        args = dict(layer=LAYER, mb0=MB0, generation=GEN, seed=SEED)
        args.update(kw)
        other = ops.noise(1, hw, **args)[0]
        assert np.isfinite(other).all() and (other != base).mean() > 0.99, "the plane does not depend on the %s" % name
        ref = synth.noise_plane(args["seed"], args["generation"], MB0, args["layer"], 128, 128).reshape(-1)
        check("philox noise, other %s" % name, other, ref, 0, atol=2e-5)
