"""tests/tower_ops_ref.py on the CPU: the float64 references agree with clip_resnet_ref and lpips_ref, the per-element bound admits an fp32
emulation of a faithful kernel at EVERY case the GPU file runs (no case, no element excluded), the lattice premise holds and the emulation
returns the lattice bits, every case with a ReLU has both of its sides populated, and each planted defect — applied to the emulation — leaves
the bound or the lattice bits at the case named next to it.  Which of the defects the old bar (4e-3 of max|ref|) let through is asserted too.
No GPU."""
import numpy as np
import pytest
import torch

import clip_resnet_ref
import lpips_ref
import tower_ops_ref as R
from clip_glass_amd import synth
from fir_ops_ref import bound_ratio
from util import check_bound

f32, f64 = np.float32, np.float64


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- the references against the project's other float64 statements of the same ops ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x1 M98 K256 N192 res1 relu1", "1x1 M12 K64 N64 res1 relu0", "gather rn 5x9", "stem3x3<1> 16-32", "stem1 S64 C8"])
def test_reference_matches_clip_resnet_ref(name):
    inp = R.make_inputs(name)
    x, w, stride, _ = R.conv_geometry(inp)
    ref, tol = R.reference(inp)
    want = clip_resnet_ref.conv_bn(x, w, inp["a"], inp["s"], stride=stride, res=inp.get("res"), relu=inp["relu"])
    assert ref.shape == want.shape and (tol > 0).all() and _rel(ref, want) < 1e-12


def test_pool_and_token_references_match_clip_resnet_ref():
    for name in ("avgpool 6x6 C64", "avgpool 2x2 C8"):
        inp = R.make_inputs(name)
        assert _rel(R.reference(inp)[0], clip_resnet_ref.avgpool2(inp["x"])) < 1e-12
    for name in ("tokens HW1 C128", "tokens HW9 C264"):
        inp = R.make_inputs(name)
        assert _rel(R.reference(inp)[0], clip_resnet_ref.attnpool_tokens(inp["x"], inp["pos"])) < 1e-12


def test_vgg_reference_matches_lpips_ref():
    """lpips_ref.slices on a state whose conv weights are fp16 values already: features.0 (the scalar first conv) from the scaled input, and
    features.2 (a gather conv, 64 -> 64) from features.0's output — each against the reference here on the same operands, 1e-12 relative."""
    sd = dict(synth.lpips_state(lpips_ref.FIXTURE_SEED))
    for idx in (0, 2):
        sd["lpips.features.%d.weight" % idx] = R.h16(sd["lpips.features.%d.weight" % idx])
    xin = lpips_ref.scale_input(lpips_ref.images(3, 2, 16))
    tr = []
    lpips_ref.slices(sd, xin, trace=tr)
    nhwc = lambda t: np.ascontiguousarray(t.numpy().transpose(0, 2, 3, 1))
    for idx, src, dst in ((0, xin, tr[0]), (2, tr[0], tr[1])):
        w, b = sd["lpips.features.%d.weight" % idx], sd["lpips.features.%d.bias" % idx]
        ref, tol = R.conv_bn_ref(nhwc(src), w, np.ones(w.shape[0]), b, mfma=idx > 0)
        assert (tol > 0).all() and _rel(ref, nhwc(dst)) < 1e-12


# ---- a faithful kernel is inside every bound; both sides of the ReLU ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_bound_admits_a_faithful_kernel(name):
    inp = R.make_inputs(name)
    ref, tol = R.reference(inp)
    check_bound("emulation in bound: " + name, R.fp32_emulation(inp), ref, tol, log=False)
    if inp.get("relu"):
        pos, zero = R.relu_sides(ref)
        assert pos > 0.2 and zero > 0.2, "%s: %.2f of the reference above 0, %.2f at 0" % (name, pos, zero)


@pytest.mark.parametrize("name", R.LATTICE_CASES)
def test_lattice_premise_and_bits(name):
    inp = R.make_inputs(name)
    bits = R.lattice_premise(name, inp)
    assert R.fp32_emulation(inp).tobytes() == bits.tobytes()
    assert np.array_equal(bits, R.h16(R.reference(inp)[0]))
    if CASE_NEG == name:
        v = R.reference(dict(inp, relu=False))[0]
        assert ((inp["res"] > 0) & (v < 0)).mean() > 0.2      # the sum is negative where the residual alone is positive


CASE_NEG = "lattice 1x1 negative sum"


def test_k4608_lattice_stays_exact():
    for name in ("lattice gather <64> 512-512 2x2", "lattice gather <64> 512-512 1x1"):
        inp = R.make_inputs(name)
        x, w, _, _ = R.conv_geometry(inp)
        A = R._conv(np.abs(x).astype(f64), np.abs(w).astype(f64), 1, torch.float64)
        assert w.shape[1] * 9 == 4608 and A.max() <= 2304 and 2304 * 16 < 2 ** 24 and np.abs(R.lattice_premise(name, inp)).max() < 65504


# ---- planted defects ---------------------------------------------------------------------------------------------------------------------------------
def _splice_rows(inp, hook, rows, cols=np.s_[:]):
    """The emulation with `hook` in the rows / columns of the [M][N] output matrix given, the faithful emulation elsewhere."""
    clean, bad = R.fp32_emulation(inp), R.fp32_emulation(inp, hook)
    out = clean.copy()
    N = clean.shape[-1]
    out.reshape(-1, N)[rows, cols] = bad.reshape(-1, N)[rows, cols]
    return out


def _w_step(inp, factor, tap=(1, 1), c0=0):
    """The weights with one 64-deep K step (64 input channels of one tap) scaled by `factor` (0: dropped, 2: run twice)."""
    w = inp["w"].copy()
    w[:, c0:c0 + 64, tap[0] % w.shape[2], tap[1] % w.shape[3]] *= factor
    return w


def _d_res_after_relu(inp):
    return R.fp32_emulation(inp, dict(epilogue=lambda acc, a, s, r, relu: np.maximum(acc * a + s, f32(0)) + r))


def _d_tap_dropped(inp):
    w = inp["w"].copy()
    w[:, :, 0, 1] = 0
    M = int(np.prod(inp["x"].shape[:3]))
    return _splice_rows(inp, dict(w=w), np.s_[M - 9:M])           # the last image row(s) only


def _d_kstep_dropped(inp):
    return _splice_rows(inp, dict(w=_w_step(inp, 0)), np.s_[:], np.s_[0:64])      # one n tile


def _d_kstep_twice(inp):
    return _splice_rows(inp, dict(w=_w_step(inp, 2)), np.s_[:], np.s_[0:64])


def _d_pad_clamped(inp):
    return R.fp32_emulation(inp, dict(pad="clamp"))


def _d_acc_fp16(inp):
    return R.fp32_emulation(inp, dict(acc=R.h16))


def _d_shift_before_scale(inp):
    def epi(acc, a, s, r, relu):
        v = (acc + s) * a
        v = v + r if r is not None else v
        return np.maximum(v, f32(0)) if relu else v
    return R.fp32_emulation(inp, dict(epilogue=epi))


def _other_weights(inp):
    return dict(inp, w=R.h16(np.random.default_rng(5).permutation(inp["w"].reshape(-1)).reshape(inp["w"].shape)))


def _d_stale_tile(inp):
    """Rows 0..127, columns 0..63 hold what the launch before left there: the same layer run with other weights."""
    return _splice_rows(inp, dict(w=_other_weights(inp)["w"]), np.s_[0:128], np.s_[0:64])


def _d_tail_leak(inp):
    """Row M - 1 computed from row M of x: in the engine the previous layer's values (random here), in the op the NaN poison."""
    x = inp["x"].copy()
    x.reshape(-1, x.shape[-1])[-1] = R.h16(np.random.default_rng(6).standard_normal(x.shape[-1]))
    M = int(np.prod(x.shape[:3]))
    return _splice_rows(inp, dict(x=x), np.s_[M - 1:M])


# defect -> (plant, the case that catches it, whether the old bar — 4e-3 of max|ref| over the whole output — lets it through there)
DEFECTS = {
    "residual added after the ReLU": (_d_res_after_relu, "1x1 M98 K64 N64 res1 relu1", False),
    "one tap dropped": (_d_tap_dropped, "gather rn 5x9", False),
    "one 64-deep K step dropped": (_d_kstep_dropped, "vgg 512-512 2x2", False),
    "one 64-deep K step run twice": (_d_kstep_twice, "vgg 512-512 2x2", False),
    "edge padding clamped": (_d_pad_clamped, "stem3x3<2> 32-64 5x9", False),
    "accumulator rounded to fp16 before BN": (_d_acc_fp16, "1x1 M98 K256 N192 res1 relu1", True),
    "BN shift before the scale": (_d_shift_before_scale, "gather rn 7x7", False),
    "stale tile of other weights": (_d_stale_tile, "1x1 128-wide 17x17", False),
    "rows M..63 of x leak into row M-1": (_d_tail_leak, "1x1 M12 K256 N64 res0 relu1", False),
}
# the same defects on lattice inputs: the bits change
LATTICE_DEFECTS = {
    "one tap dropped": (_d_tap_dropped, "lattice gather <64> rn 5x9"),
    "one 64-deep K step dropped": (_d_kstep_dropped, "lattice gather <64> 512-512 2x2"),
    "one 64-deep K step run twice": (_d_kstep_twice, "lattice gather <64> 512-512 2x2"),
    "residual added after the ReLU": (_d_res_after_relu, CASE_NEG),
    "edge padding clamped": (_d_pad_clamped, "lattice stem3x3<2>"),
}


def _old_bar_passes(got, ref):
    return bool(np.isfinite(got).all() and np.abs(got - ref).max() <= 4e-3 * np.abs(ref).max())


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_bound_has_teeth(defect):
    plant, name, old_passes = DEFECTS[defect]
    inp = R.make_inputs(name)
    ref, tol = R.reference(inp)
    got = plant(inp)
    ratio, old = bound_ratio(got, ref, tol), _old_bar_passes(got, ref)
    print("[teeth] %-42s caught at %-34s worst err/tol %8.1f; old bar (4e-3 max|ref|): %s" % (defect, name, ratio, "PASS" if old else "FAIL"))
    assert ratio > 1, "defect '%s' stays inside the bound at %s (worst err/tol %.3f)" % (defect, name, ratio)
    with pytest.raises(AssertionError):
        check_bound("teeth: " + defect, got, ref, tol, log=False)
    assert old == old_passes, "the old bar's verdict on '%s' at %s is %s" % (defect, name, "PASS" if old else "FAIL")


@pytest.mark.parametrize("defect", sorted(LATTICE_DEFECTS))
def test_lattice_bits_have_teeth(defect):
    plant, name = LATTICE_DEFECTS[defect]
    inp = R.make_inputs(name)
    bits = R.lattice_premise(name, inp)
    got = plant(inp)
    print("[teeth] %-42s changes %d of %d lattice values at %s" % (defect, int((got != bits).sum()), bits.size, name))
    assert got.tobytes() != bits.tobytes()


def test_stale_tile_under_the_old_bar_and_the_new():
    """The tile a kernel never stored, as the suite saw it while the ops staged their outputs raw: the allocation came back holding the PARENT
    run's values — the same test's launch a moment before, the same inputs — so the tile equals the reference's own values and the old bar passes
    (with any bar: the defect is invisible).  With poisoned staging the tile is NaN: check_bound fails.  A tile from any other launch is outside
    the bound (test_bound_has_teeth)."""
    name = "1x1 128-wide 17x17"
    inp = R.make_inputs(name)
    ref, tol = R.reference(inp)
    parent = R.fp32_emulation(inp)                       # what the parent run left in the allocation
    stale = parent.copy()                                # the kernel under test stores everything but the tile
    assert _old_bar_passes(stale, ref)
    poisoned = parent.copy()
    poisoned.reshape(-1, 256)[0:128, 0:64] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check_bound("poisoned tile", poisoned, ref, tol, log=False)
    assert not _old_bar_passes(poisoned, ref)


def test_poisoned_tail_shows_a_leak():
    """Row M of x is NaN in the op: a row M - 1 that reads it is NaN, whatever the engine's buffer would have held there."""
    inp = R.make_inputs("1x1 M12 K256 N64 res0 relu1")
    ref, tol = R.reference(inp)
    x = inp["x"].copy()
    x.reshape(-1, x.shape[-1])[-1, 5] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check_bound("leak of the poisoned tail", R.fp32_emulation(inp, dict(x=x)), ref, tol, log=False)
