"""tests/fir_ops_ref.py on the CPU: the vectorised mirrors equal the index-level emulators bit for bit, the references agree with the oracle, an
fp32 emulation of a faithful kernel lies inside every bound at every case the GPU file runs (and equals the mirror on lattice inputs), the bound
tells the two contraction forms of fir4 apart, and every planted defect fails the new checks — with the verdict of the old bars next to it.  No
GPU; the built library's host code packs the weights."""
import math

import numpy as np
import pytest
import torch

import emu_down64
import emu_ops
import fir_ops_ref as R
from oracle import stylegan2_ref as sg
from util import check, check_bound, nchw, nhwc

f16, f32, f64 = np.float16, np.float32, np.float64


def blur_down64(x):
    """FIR pad 1 + [::2] in float64, rounded to fp16: a faithful launch_blur_down for the CPU tests (the GPU tests take the device's own)."""
    f = np.array([1, 3, 3, 1], dtype=f64) / 8
    B, H, W, _ = x.shape
    xp = np.pad(np.asarray(x, f64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    return R.h16(sum(f[a] * f[b] * xp[:, a:a + H:2, b:b + W:2] for a in range(4) for b in range(4)))


def _unpack(w):
    """The packed weights back in reference layout: what emu_down64 takes (it rounds its arguments to fp16 and applies no coefficient)."""
    return np.ascontiguousarray(R._pack(w).reshape(w.shape[2], w.shape[3], w.shape[0], w.shape[1]).transpose(2, 3, 0, 1))


_cache = {}


def down_case(kernel, B, R_, Cin, Cout, lattice=False):
    key = (kernel, B, R_, Cin, Cout, lattice)
    if key not in _cache:
        if kernel in ("conv_down", "conv_down64"):
            inp = R.lattice_down(B, R_, Cin, Cout) if lattice else R.down_inputs(B, R_, Cin, Cout)
            inp["xs"] = blur_down64(inp["x"])
        else:
            inp = R.s2_inputs(B, R_, Cin, Cout)
            if B > 3:
                inp = R.take_down(inp, R.three(B))
        _cache[key] = (inp,) + R.down_ref(kernel, inp)
    return _cache[key]


# ---- 1. mirrors against the index-level emulators ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", [True, False])
def test_down_mirror_equals_emulator(lattice):
    """conv_down at its smallest geometry (R = 64, one tile column), conv_down64 at R = 16 on three workgroups (priming mid-column)."""
    inp = down_case("conv_down", 1, 64, 32, 64, lattice)[0]
    emu = emu_ops.dblock_down(inp["h"], inp["x"], inp["w1"], inp["ws"], inp["b1"])
    # (emu_ops.dblock_down makes its own skip input with emu_ops.blur)
    np.testing.assert_array_equal(R.down_mirror("conv_down", dict(inp, xs=emu_ops.blur(inp["x"], 1))), emu)
    inp = down_case("conv_down64", 1, 16, 64, 128, lattice)[0]
    emu, count = emu_down64.dblock_down64(inp["h"], inp["xs"], _unpack(inp["w1"]), _unpack(inp["ws"]), inp["b1"], n_cus=3)
    assert (count == 1).all()
    np.testing.assert_array_equal(R.down_mirror("conv_down64", inp), emu)


def test_dblock0_mirror_equals_emulator():
    inp = R.lattice_dblock0(1, 64)
    np.testing.assert_array_equal(R.dblock0_mirror(inp), emu_ops.dblock0(*R.dblock0_args(inp), n_wg=3))


@pytest.mark.parametrize("lattice", [True, False])
def test_upfir_mirror_equals_emulator(lattice):
    """A 3 x 2 virtual grid of 8 x 8 images with two empty slots, two-step segments (S = 2: the FIR window carried across a step boundary)."""
    B, H, Cin, Cout, bs = 4, 8, 32, 32, 2
    inp = R.lattice_up(B, H, Cin, Cout, bs, post_scale=True) if lattice else R.up_inputs(3, B, H, Cin, Cout, bs, post_scale=True)
    geo = emu_ops.upfir2_geometry(B, H, H, Cout, S=2)
    assert geo["NXI"] * geo["NYI"] > B and geo["n_seg"] >= 2
    emu = emu_ops.upfir2(inp["x"], inp["w"], sn=inp["sn"], dscale=inp["dscale"], noise=inp["noise"], noise_strength=inp["noise_strength"],
                         batch_size=bs, bias=inp["bias"], act=True, post_scale=inp["post_scale"], geo=geo)
    np.testing.assert_array_equal(R.upfir_mirror(inp, lean=False), emu)


# ---- 2. references against the oracle ---------------------------------------------------------------------------------------------------------------
def _oracle_down(h, x, w1, ws, b1):
    ht, xt = torch.tensor(nchw(h)), torch.tensor(nchw(x))
    h1 = sg._bias_act(sg._conv(sg._filter(ht, sg._fir(), 2, 2), torch.tensor(w1), stride=2), torch.tensor(b1))
    xs = sg._filter(xt, sg._fir(), 1, 1)[:, :, ::2, ::2]
    return nhwc(((h1 + sg._conv(xs, torch.tensor(ws))) / math.sqrt(2)).numpy())


@pytest.mark.parametrize("kernel,B,R_,Cin,Cout", [("conv_down", 1, 64, 32, 64), ("conv_down64", 1, 16, 64, 128)])
def test_down_ref_matches_the_oracle(kernel, B, R_, Cin, Cout):
    """4e-4 max|ref| is what a float64 conv on the device's rounded WEIGHTS leaves against the oracle's fp32 ones (test_conv_ops_ref.py).  Here the
    operand carries the two fp16 FIR passes as well, which the mirror reproduces on purpose: on N(0, 1) maps they alone leave an rms of 1.3e-4
    and a largest deviation of 0.9 .. 1.03 times that bar (measured on this CPU: (1, 64, 32, 64) 7.4e-4 of 7.9e-4, (1, 128, 32, 64) 7.9e-4 of 8.0e-4,
    (2, 64, 64, 128) 8.2e-4 of 9.2e-4; at (2, 64, 32, 64) ONE of 131072 elements reaches 8.5e-4 against 8.2e-4).  So the random maps are asserted at
    the smallest geometry of each kernel (the ones the emulators run above), and the larger geometries on maps whose FIR is exact (multiples of 1/4:
    lattice_down's) with the same random weights — there the bar means what it meant in test_conv_ops_ref.py."""
    inp, ref, tol = down_case(kernel, B, R_, Cin, Cout)
    assert (tol > 0).all() and np.isfinite(ref).all()
    check("down_ref[%s] vs oracle" % kernel, ref, _oracle_down(inp["h"], inp["x"], inp["w1"], inp["ws"], inp["b1"]), 4e-4)
    B, R_ = (2, 64) if kernel == "conv_down" else (1, 36)
    inp = dict(R.down_inputs(B, R_, Cin, Cout), h=R.lattice_down(B, R_, Cin, Cout)["h"])
    inp["xs"] = blur_down64(inp["x"])
    for form in R.FORMS:
        check("down_ref[%s, %s] vs oracle, exact FIR" % (kernel, form), R.down_ref(kernel, inp, form)[0],
              _oracle_down(inp["h"], inp["x"], inp["w1"], inp["ws"], inp["b1"]), 4e-4)


@pytest.mark.parametrize("kernel", ["conv_s2", "conv_tiled_skip"])
def test_s2_ref_matches_the_oracle(kernel):
    inp, ref, tol = down_case(kernel, 2, 64, 32, 64)
    h1 = sg._bias_act(sg._conv(torch.tensor(nchw(inp["hb"])), torch.tensor(inp["w1"]), stride=2), torch.tensor(inp["b1"]))
    want = nhwc(((h1 + sg._conv(torch.tensor(nchw(inp["xs"])), torch.tensor(inp["ws"]))) * inp["out_scale"]).numpy())
    check("down_ref[%s] vs oracle" % kernel, ref, want, 4e-4)


def test_dblock0_ref_matches_the_oracle():
    """The back half (FIR, stride-2 conv, skip branch) against the oracle's ops at 4e-4 max|ref| on maps whose FIR is exact, in both FIR orders and
    forms; the front (fromRGB, conv0) against the oracle's within its counted roundings; and, printed only, the whole chain on a lattice front: the
    front's mirrored roundings (x and h stored as fp16, 0.2h = 0.2 (1 - 2.4e-4), k1 = h(sqrt2) = sqrt2 (1 - 1.1e-4)) leave 1.0e-3 against the oracle
    where 4e-4 max|ref| is 7.0e-4 (117 of 41472 elements above it, measured on this CPU) — not a figure that bar was made for."""
    inp = R.lattice_dblock0(2, 36, seed=1)
    y, fw, fb = torch.tensor(inp["y"]), torch.tensor(inp["frgb_w"]), torch.tensor(inp["frgb_b"])
    img = ((y + 1) / 2).clip(0, 1) * 2 - 1
    xo = sg._bias_act(torch.einsum("bchw,oc->bohw", img, fw), fb)        # (frgb_w is passed scaled: test_gpu_ops._dblock0_case)
    ho = sg._bias_act(sg._conv(xo, torch.tensor(inp["w0"]), padding=1), torch.tensor(inp["b0"]))
    xo, ho = nhwc(xo.numpy()).astype(f64), nhwc(ho.numpy()).astype(f64)
    x, h = (a.astype(f64) for a in R.dblock0_front(inp))
    # x: fp16(z) is exact on the lattice; a negative value is h(z * 0.2h): the constant and the product round (2 U16), the oracle's fp32 does the rest
    ex = 2 * R.U16 * np.abs(xo) + 8 * R.U32 * np.abs(xo) + 2.0 ** -24
    assert (np.abs(x - xo) <= ex).all()
    # h: conv0 of x (error ex through |w0| and the gain sqrt2), then h(acc), the constant k1 / k2, the product: 3 U16 (k2 = h(0.2f sqrt2f): two)
    w0 = np.abs(R._pack(inp["w0"]))
    eh = math.sqrt(2) * R._conv(ex, w0, 1, 1, torch.float64) + 4 * R.U16 * np.abs(ho) + (2 * 289 + 8) * R.U32 * math.sqrt(2) * R._conv(np.abs(x), w0, 1, 1, torch.float64) + 2.0 ** -24
    assert (np.abs(h - ho) <= eh).all() and (eh <= 6e-3 * np.abs(ho).max()).all()
    for variant in ("fused", "stream"):
        ref, tol = R.dblock0_ref(inp, variant=variant)
        full = _oracle_down(ho.astype(f32), xo.astype(f32), inp["w1"], inp["ws"], inp["b1"])
        print("[dblock0_ref %s] whole chain vs oracle: max err %.3e, 4e-4 max|ref| = %.3e" % (variant, np.abs(ref - full).max(), 4e-4 * np.abs(full).max()))
        lat = R.lattice_down(2, 36, 32, 64)
        maps = (R.h16(np.random.default_rng(3).integers(-4, 5, lat["h"].shape) / 4.0), lat["h"])
        for form in R.FORMS:
            ref, tol = R.dblock0_ref(inp, form, variant, front=maps)
            check("dblock0_ref[%s, %s] back half vs oracle, exact FIR" % (variant, form), ref, _oracle_down(maps[1], maps[0], inp["w1"], inp["ws"], inp["b1"]), 4e-4)


def _oracle_up(inp):
    x = torch.tensor(nchw(inp["x"]))
    Cin = x.shape[1]
    y = sg._mod_conv(x, torch.tensor(inp["sn"]), torch.tensor(inp["w"]), torch.eye(Cin) * math.sqrt(Cin), torch.zeros(Cin), demod=False, up=True)
    y = y * torch.tensor(inp["dscale"])[:, :, None, None]
    y = y + inp["noise_strength"] * torch.tensor(inp["noise"]).repeat_interleave(inp["batch_size"], dim=0)[:, None]
    y = sg._bias_act(y, torch.tensor(inp["bias"]))
    if inp.get("post_scale") is not None:
        y = y * torch.tensor(inp["post_scale"])[:, :, None, None]
    return nhwc(y.numpy())


@pytest.mark.parametrize("lean", [False, True])
def test_upfir_ref_matches_the_oracle(lean):
    inp = R.up_inputs(3, 3, 12, 32, 64, batch_size=1, post_scale=True)
    ref, tol = R.upfir_ref(inp, lean)
    assert (tol > 0).all() and np.isfinite(ref).all()
    # (post_scale reaches the kernel as fp16: 2^-11 relative on top of conv_ops_ref's 4e-4 is inside it)
    check("upfir_ref lean=%d vs oracle" % lean, ref, _oracle_up(inp), 4e-4)


# ---- 3. an fp32 emulation of a faithful kernel lies inside every bound, at every case of the GPU file ------------------------------------------------------
@pytest.mark.parametrize("case", R.DOWN_CASES + R.S2_CASES, ids=lambda c: "%s-%d-%d-%d-%d" % c)
def test_bound_admits_a_faithful_down_kernel(case):
    kernel = case[0]
    inp, ref, tol = down_case(*case)
    check_bound("emulation in bound: %s %s" % (kernel, case[1:]), R.down_mirror(kernel, inp, dtype=torch.float32), ref, tol, log=False)


@pytest.mark.parametrize("B,R_", R.D0_CASES + [R.D0_TWO_KERNEL_CASE])
def test_bound_admits_a_faithful_dblock0(B, R_):
    inp = R.lattice_dblock0(B, R_)
    for variant in (("fused",) if (B, R_) != R.D0_TWO_KERNEL_CASE else ("fused", "stream")):
        ref, tol = R.dblock0_ref(inp, variant=variant)
        check_bound("emulation in bound: dblock0 %s B%d R%d" % (variant, B, R_), R.dblock0_mirror(inp, variant=variant, dtype=torch.float32), ref, tol, log=False)


def _up_case(B, H, Cin, Cout, bs, ps, lean):
    inp = R.up_inputs(51 if lean else 3, B, H, Cin, Cout, bs, post_scale=ps)
    return R.take_up(inp, R.three(B)) if B > 8 else inp


@pytest.mark.parametrize("lean,case", [(False, c) for c in R.UP_GRID_CASES] + [(True, c) for c in R.UP_LEAN_CASES], ids=lambda c: str(c).replace(" ", ""))
def test_bound_admits_a_faithful_upconv(lean, case):
    inp = _up_case(*case, lean)
    ref, tol = R.upfir_ref(inp, lean)
    for form in R.UP_FORMS:         # whichever way a compiler contracts the FIR, a faithful kernel is inside the counted bound
        check_bound("emulation in bound: up-conv lean=%d %s %s" % (lean, case, form), R.upfir_mirror(inp, lean, form, torch.float32), ref, tol, log=False)


@pytest.mark.parametrize("case", R.DOWN_LATTICE_CASES[::2], ids=lambda c: "%s-%d-%d-%d-%d" % c)
def test_lattice_down_emulation_is_the_mirror(case):
    """On lattice inputs the fp32 sums ARE the float64 sums, in every form and FIR order: the device has one answer."""
    kernel = case[0]
    inp = down_case(*case, lattice=True)[0]
    want = R.down_mirror(kernel, inp)
    assert np.isfinite(want).all() and np.abs(want).max() > 1 and len(np.unique(want)) > 500
    for form in R.FORMS:
        np.testing.assert_array_equal(R.down_mirror(kernel, inp, form, torch.float32), want)


@pytest.mark.parametrize("lean", [False, True])
def test_lattice_upconv_emulation_is_the_mirror(lean):
    inp = R.lattice_up(9, 32, 32, 32, 3, post_scale=True)
    outs = {form: R.upfir_mirror(inp, lean, form) for form in R.UP_FORMS}
    for form in R.UP_FORMS:
        np.testing.assert_array_equal(R.upfir_mirror(inp, lean, form, torch.float32), outs[form])
    # the lattice tells all four combinations of contraction forms apart: a device result equals at most one of them
    for fa in R.UP_FORMS:
        for fb in R.UP_FORMS:
            assert fa == fb or not np.array_equal(outs[fa], outs[fb]), "forms %s and %s give the same bits" % (fa, fb)


# ---- 4. the bound sees the contraction form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [R.DOWN_CASES[0], R.DOWN_CASES[3]], ids=lambda c: c[0])
def test_bound_sees_the_contraction_form(case):
    kernel = case[0]
    inp, ref, tol = down_case(*case)
    a_fma, a_sep = (R.blur_operand(inp["h"], "vh", form) for form in R.FORMS)
    sep = R.down_mirror(kernel, inp, "sep", torch.float32)
    ratio = np.abs(sep - ref) / tol
    print("[form] %s: operand elements that differ %.1f %%, outputs of the uncontracted form outside the as-built bound %.1f %% (worst err/tol %.2f), "
          "median bound %.2e, old bar %.2e" % (kernel, 100 * (a_fma != a_sep).mean(), 100 * (ratio > 1).mean(), ratio.max(), np.median(tol), 6e-3 * np.abs(ref).max()))
    assert ratio.max() > 1
    ref_s, tol_s = R.down_ref(kernel, inp, "sep")       # and each form is inside its own bound
    check_bound("sep in its own bound", sep, ref_s, tol_s, log=False)
    assert R.bound_ratio(R.down_mirror(kernel, inp, "fma", torch.float32), ref_s, tol_s) > 1


# ---- 5. planted defects ---------------------------------------------------------------------------------------------------------------------------------------
BORDERS = (np.s_[:, :2], np.s_[:, -2:], np.s_[:, :, :2], np.s_[:, :, -2:])
VERDICTS = {}        # defect -> family -> (old bars pass?, worst err / tol under the new check)


def _old_bar(got, ref, whole, border=None):
    """The bars these kernels had: `whole` * max|ref| everywhere and `border` * max|ref[slice]| on the four two-pixel border slices (util.check)."""
    ok = np.abs(got - ref).max() <= whole * np.abs(ref).max()
    if border is not None:
        ok = ok and all(np.abs(got[sl] - ref[sl]).max() <= border * np.abs(ref[sl]).max() for sl in BORDERS)
    return bool(ok)


def _record(defect, family, old_pass, new_ratio):
    VERDICTS.setdefault(defect, {})[family] = (old_pass, new_ratio)
    print("[defect] %-46s %-16s old bars: %s   new check: worst err/tol %.2f -> %s" % (defect, family, "PASS" if old_pass else "FAIL", new_ratio,
                                                                                       "FAIL" if new_ratio > 1 else "pass"))
    assert new_ratio > 1, "%s on %s stays inside the new check under some contraction form" % (defect, family)


def _down_refs(kernel, inp):
    return {form: R.down_ref(kernel, inp, form) for form in R.FORMS}


UNCONTRACTED = "uncontracted fir4 (against the as-built form)"


def _worst_over_forms(got, refs, defect=None):
    """A device result passes when ONE form's bound holds everywhere: a defect has to leave every form's.  The exception is the uncontracted fir4
    itself: a build that contracts nothing is another legitimate kernel and holds "sep" everywhere by construction, so that defect is measured
    against the form these kernels are built with and match on the device ("fma": DESIGN.md) — what a change of form inside that build leaves."""
    if defect == UNCONTRACTED:
        return R.bound_ratio(got, *refs["fma"])
    return min(R.bound_ratio(got, ref, tol) for ref, tol in refs.values())


def _pad_unmasked(h, b, ch):
    """The zero-padded map with ONE 1/8-weight tap left unmasked: the second pad column right of sample b's image holds the clamped load (the last
    image column) for the 8-channel group `ch`."""
    v = np.pad(np.asarray(h).astype(f16), ((0, 0), (2, 2), (2, 2), (0, 0)))
    v[b, 2:-2, -1, ch:ch + 8] = v[b, 2:-2, -3, ch:ch + 8]
    return v


def _planted_down(kernel):
    case = R.DOWN_CASES[0] if kernel == "conv_down" else R.DOWN_CASES[3]
    inp, ref, tol = down_case(*case)
    refs = _down_refs(kernel, inp)
    clean = R.down_mirror(kernel, inp, dtype=torch.float32)
    assert _worst_over_forms(clean, refs) <= 1 and _old_bar(clean, ref, 6e-3, 8e-3)
    a, w1, wk = R.down_operands(kernel, inp)
    run = lambda **kw: R.down_mirror(kernel, inp, dtype=torch.float32, **kw)
    defects = {
        "FIR pass order swapped": run(a=R.blur_operand(inp["h"], "hv").astype(f32)),
        UNCONTRACTED: run(a=R.blur_operand(inp["h"], "vh", "sep").astype(f32)),
        "one 1/8 tap unmasked at the right border": run(a=R._fir_pass(R._fir_pass(_pad_unmasked(inp["h"], 0, 8), 1, "fma"), 2, "fma").astype(f32)),
        "skip weights scaled by 1/sqrt2 before their rounding": run(wk=R.h16(np.asarray(inp["ws"], f32).reshape(wk.shape) * f32(1 / math.sqrt(wk.shape[1])) * R.SKIP_SCALE)),
    }
    # the skip rows are also pinned bit for bit by the skip-branch lattice run: where the bound alone does not see their rounding, that run does
    lat = R.lattice_down_skip(*case[1:])
    lat_bad = R.down_mirror(kernel, lat, wk=R.h16(np.asarray(lat["ws"], f32).reshape(wk.shape) * f32(1 / math.sqrt(wk.shape[1])) * R.SKIP_SCALE))
    skip_seen_on_lattice = not np.array_equal(lat_bad, R.down_mirror(kernel, lat))
    for name, got in defects.items():
        assert not np.array_equal(got, clean)
        ratio = _worst_over_forms(got, refs, name)
        if name.startswith("skip weights"):
            print("         (skip weights, %s: the bound alone gives worst err/tol %.2f; the skip-branch lattice run differs: %s)" % (kernel, ratio, skip_seen_on_lattice))
            ratio = ratio if ratio > 1 or not skip_seen_on_lattice else float("inf")
        _record(name, kernel, _old_bar(got, ref, 6e-3, 8e-3), ratio)


def _planted_dblock0():
    inp = R.lattice_dblock0(1, 64)
    refs = {form: R.dblock0_ref(inp, form) for form in R.FORMS}
    ref = refs["fma"][0]
    clean = R.dblock0_mirror(inp, dtype=torch.float32)
    assert _worst_over_forms(clean, refs) <= 1 and _old_bar(clean, ref, 6e-3, 8e-3)
    x, h = R.dblock0_front(inp, check=False)
    wk = R.dblock0_operands(inp)[3]
    run = lambda **kw: R.dblock0_mirror(inp, dtype=torch.float32, **kw)
    defects = {
        "FIR pass order swapped": run(a=R.blur_operand(h, "vh").astype(f32)),
        UNCONTRACTED: run(a=R.blur_operand(h, "hv", "sep").astype(f32)),
        "one 1/8 tap unmasked at the right border": run(a=R._fir_pass(R._fir_pass(_pad_unmasked(h, 0, 8), 2, "fma"), 1, "fma").astype(f32)),
        "skip weights scaled by 1/sqrt2 before their rounding": run(wk=R.h16(np.asarray(inp["ws"], f32).reshape(wk.shape) * f32(1 / math.sqrt(32)) * R.SKIP_SCALE)),
    }
    lat = R.lattice_dblock0_skip(1, 64)
    lat_bad = R.dblock0_mirror(lat, wk=R.h16(np.asarray(lat["ws"], f32).reshape(wk.shape) * f32(1 / math.sqrt(32)) * R.SKIP_SCALE))
    skip_seen_on_lattice = not np.array_equal(lat_bad, R.dblock0_mirror(lat))
    for name, got in defects.items():
        assert not np.array_equal(got, clean)
        ratio = _worst_over_forms(got, refs, name)
        if name.startswith("skip weights"):
            print("         (skip weights, dblock0: the bound alone gives worst err/tol %.2f; the skip-branch lattice run differs: %s)" % (ratio, skip_seen_on_lattice))
            ratio = ratio if ratio > 1 or not skip_seen_on_lattice else float("inf")
        _record(name, "dblock0", _old_bar(got, ref, 6e-3, 8e-3), ratio)


def _planted_upconv(lean):
    """The new check of an up-conv is the lattice run (bit equality under one of the four forms) AND the counted bound on random inputs; a defect
    fails when either does.  The figure recorded is the counted bound's worst err / tol where the lattice run does not already differ, else inf."""
    family = "upfir2<%s>" % ("false" if lean else "true")
    B, H, Cin, Cout, bs = 6, 16, 32, 32, 2          # a 6 x 1 grid: noise planes shared by pairs, every image with its own tables
    lat = R.lattice_up(B, H, Cin, Cout, bs, post_scale=True)
    rnd = R.up_inputs(3, B, H, Cin, Cout, bs, post_scale=True)
    ref, tol = R.upfir_ref(rnd, lean)
    lat_forms = [R.upfir_mirror(lat, lean, form) for form in R.UP_FORMS]
    clean = R.upfir_mirror(rnd, lean, dtype=torch.float32)
    assert R.bound_ratio(clean, ref, tol) <= 1 and _old_bar(clean, ref, 5e-3)
    defects = {"a stale hs window row across a step boundary": ("stale_hs", 1, 1 + 2 + 16 + 13),       # T row 13 of the second step keeps the first step's
               "the noise plane of the neighbouring minibatch": ("noise_plane", 2, 0)}
    if not lean:        # (the lean instance has one image per grid: no second image row, no table rows of other candidates)
        defects["kpsa where kpsb applies"] = ("kps_row", 3, 2)
        defects["another candidate's dscale on one 8-channel group"] = ("dscale_group", 1, 4, 8)
    for name, d in defects.items():
        got = R.upfir_mirror(rnd, lean, dtype=torch.float32, defect=d)
        got_lat = R.upfir_mirror(lat, lean, defect=d)
        lattice_differs = all(not np.array_equal(got_lat, m) for m in lat_forms)
        ratio = R.bound_ratio(got, ref, tol)
        assert lattice_differs, "%s: the lattice run does not see it" % name
        _record(name, family, _old_bar(got, ref, 5e-3), ratio if ratio > 1 else float("inf"))
        print("         (counted bound alone: worst err/tol %.2f)" % ratio)


def test_planted_defects():
    """Every planted defect fails the new check of every family it applies to (asserted in _record), and at least three of them were invisible
    to the bars these kernels had."""
    VERDICTS.clear()
    _planted_down("conv_down")
    _planted_down("conv_down64")
    _planted_dblock0()
    _planted_upconv(False)
    _planted_upconv(True)
    assert len(VERDICTS) == 8
    invisible = sorted(d for d, fams in VERDICTS.items() if any(old and new > 1 for old, new in fams.values()))
    print("[defect] pass the old bars, fail the new checks: %s" % invisible)
    assert len(invisible) >= 3, invisible
