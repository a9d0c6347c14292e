"""The BigGAN path's per-element bounds on the CPU (tests/conv_ops_ref.py's BigGAN fields, tests/biggan_ops_ref.py's bg_tail and batched-GEMM
bounds): the references agree with biggan_ops_ref.conv / tail — which tests/test_biggan_ops_ref.py pins to oracle/biggan_ref.py — an fp32
emulation of a faithful kernel sits inside every bound under every form and equals every lattice mirror bit for bit, the new per-element bound is
nowhere above the bar it replaces, and every planted defect leaves every form's bound or differs from the lattice mirror.  Each defect test
prints whether the OLD bar would have passed it ("BigGAN path: what the tests pin", holds the table).  No GPU; the built library's
host code packs the weights."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import biggan_ops_ref as B
import conv_ops_ref as R
from util import check

f32, f64 = np.float32, np.float64
GEMM_CASES = [(256, 64, 64, 3), (192, 64, 64, 3), (256, 128, 64, 0), (512, 128, 64, 0), (256, 64, 32, 3), (128, 64, 256, 0), (128, 128, 1024, 0), (192, 64, 256, 0)]
GEMM_OLD = {3: 3e-3, 0: 4e-3}          # x max|ref|
TAIL_OLD = 4e-3                        # absolute, images in (-1, 1)
TAIL_SHAPES = [(1, 32), (3, 64)]


def _family(inp):
    return R.FAMILY_OF_IMPL[inp["impl"]]


def _forms(inp):
    return R.PRE_FORMS if inp.get("pre_shift") is not None else ("fma",)


def _report(what, new_caught, old_passed):
    print("[planted] %-64s new bar: %-7s old bar: %s" % (what, "CAUGHT" if new_caught else "passed", "passed" if old_passed else "caught"))


# ---- the rounding helpers ------------------------------------------------------------------------------------------------------------------------
def _nearest(fr, dtype):
    """The `dtype` value nearest to the Fraction fr, ties to even — by exact comparison with the neighbours of a first guess."""
    c = dtype(float(fr))
    cands = sorted({float(np.nextafter(c, dtype(-np.inf))), float(c), float(np.nextafter(c, dtype(np.inf)))})
    best = min(cands, key=lambda v: (abs(Fraction(v) - fr), int(np.array(v, dtype).view({2: np.uint16, 4: np.uint32}[np.dtype(dtype).itemsize])) & 1))
    return best


def test_fma_mirrors_round_once_without_assuming_an_exact_float64_sum():
    """fma32 / fma16 against exact rational arithmetic, on operands whose float64 sum is NOT exact (products far below the addend) as well as on
    ordinary ones; sum_odd reports how many sums were inexact, so the premise is counted rather than assumed."""
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(400) * 10.0 ** rng.uniform(-6, 2, 400)).astype(f32)
    b = rng.standard_normal(400).astype(f32)
    c = (rng.standard_normal(400) * 10.0 ** rng.uniform(-3, 3, 400)).astype(f32)
    assert B.sum_odd(a.astype(f64) * b.astype(f64), c)[1] > 50
    got = B.fma32(a, b, c, "fma")
    for i in range(400):
        assert got[i] == _nearest(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])), np.float32), i
    sep = B.fma32(a, b, c, "sep")
    assert np.array_equal(sep, (a * b + c).astype(f64))                      # numpy float32 arithmetic IS the separate form
    h = lambda v: np.asarray(v, f64).astype(np.float16).astype(f64)
    x, s, t = h(rng.standard_normal(400)), h(rng.standard_normal(400) * 10.0 ** rng.uniform(-3, 1, 400)), h(rng.standard_normal(400))
    got = B.fma16(x, s, t, "fma")
    for i in range(400):
        assert got[i] == _nearest(Fraction(x[i]) * Fraction(s[i]) + Fraction(t[i]), np.float16), i
    assert np.array_equal(B.fma16(x, s, t, "sep"), h(h(x * s) + t))


# ---- the extended conv reference against biggan_ops_ref.conv ------------------------------------------------------------------------------------
def _plain(inp, rounded_w):
    """biggan_ops_ref.conv of the same launch with no mirrored rounding of the input affine; weights as packed (rounded_w) or in float64."""
    w = inp["w"].astype(f64) / np.sqrt(float(np.prod(inp["w"].shape[1:])))
    if rounded_w:
        KS = inp["w"].shape[2]
        w = R._pack(inp["w"]).astype(f64).reshape(KS, KS, w.shape[0], w.shape[1]).transpose(2, 3, 0, 1)
    pre = (inp["sn"], inp["pre_shift"]) if inp.get("pre_shift") is not None else None
    y = B.conv(inp["x"], w, pre=pre, in_up=bool(inp.get("in_up")), dscale=inp.get("dscale"), bias=inp.get("bias"), shift=inp.get("shift"),
               relu=inp["act"] == 2, res=inp.get("res"), res_up=bool(inp.get("res_up")))
    return np.tanh(y[..., :3]).transpose(0, 3, 1, 2) if inp.get("rgb_tanh") else y


@pytest.mark.parametrize("name", sorted(R.BG_CASES))
def test_conv_ref_agrees_with_biggan_ops_ref(name):
    """Within the weights' fp16 rounding, 4e-4 max|ref| (test_conv_ops_ref.py's bar).  The forms with the input affine mirror a SECOND rounding,
    relu(x A + S) to fp16 — 2^-11 of every operand, ~3e-4 of max|ref| through K = 128 .. 1152 products, which the 4e-4 bar cannot hold on a random
    map (the FIR-chain suite met the same): there the bar is asserted on the lattice map, where the mirror is exact and so is the agreement, and
    the random map is held to the float64 model with the same declared rounding (biggan_ops_ref.pre_bn_relu), to 1e-9."""
    inp = R.bg_case(name)
    ref = R.conv_ref(inp, _family(inp))[0]
    if inp.get("pre_shift") is None:
        check("conv_ref %s vs biggan_ops_ref.conv" % name, ref, _plain(inp, False), 4e-4)
        return
    lat, _ = R.bg_lattice(**{**R.BG_CASES[name][0], **({"H": 64, "W": 288} if R.BG_CASES[name][0]["H"] == 0 else {})})
    check("conv_ref %s (lattice) vs biggan_ops_ref.conv" % name, R.conv_ref(lat, _family(lat))[0], _plain(lat, False), 4e-4)
    rounding = "f16" if R.KERNELS[_family(inp)][1] == "sn16" else "f32"
    w = R._pack(inp["w"]).astype(f64).reshape(inp["w"].shape[2], inp["w"].shape[3], inp["w"].shape[0], inp["w"].shape[1]).transpose(2, 3, 0, 1)
    y = B.conv(inp["x"], w, pre=(inp["sn"], inp["pre_shift"]), dscale=inp.get("dscale"), bias=inp.get("bias"), shift=inp.get("shift"),
               relu=inp["act"] == 2, pre_rounding=rounding)
    y = np.tanh(y[..., :3]).transpose(0, 3, 1, 2) if inp.get("rgb_tanh") else y
    if rounding == "f16":                    # pre_bn_relu("f16") rounds the exact x A16 + S16 once: the "fma" form
        assert np.abs(ref - y).max() <= 1e-9 * np.abs(y).max()
    else:                                    # ("f32" rounds the float64 affine to fp16 directly, not through fp32: equal but for double roundings)
        check("conv_ref %s vs biggan_ops_ref.conv(pre_rounding=f32)" % name, ref, y, 4e-4)


@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_ref_agrees_with_biggan_ops_ref(shape):
    """On the lattice the mirrored operands are exact, and tail_ref is biggan_ops_ref.tail.  On the random map the mirror rounds Ca, the
    fragments w3 Ca and Cc to fp16; the distance to the unrounded restatement is bounded per element by those three roundings carried through
    |W_rgb| (tanh is 1-Lipschitz) — computed here, not fitted."""
    inp, s = B.tail_lattice(*shape)
    assert np.abs(np.tanh(s) - B.tail(*inp)).max() <= 1e-12
    assert np.abs(B.tail_ref(*inp)[2] - s).max() == 0
    inp = B.tail_inputs(*shape)
    h, x0, w3, b3, A, S, rgb_w, rgb_b = (np.asarray(a, f64) for a in inp)
    ref = B.tail_ref(*inp)[0]
    dist = np.abs(ref - B.tail(*inp))
    bound = np.empty_like(dist)
    for b in range(h.shape[0]):       # |Ca - a| <= U16 |a|; |W3s - w3 a| <= 2 U16 |w3 a| (Ca's rounding and the product's); |Cc - (b3 a + s)| <= (U16 + 2 U32) |.|
        dz = 2 * B.U16 * (np.abs(h[b]) @ np.abs(w3 * A[:, None]).T) + B.U16 * np.abs(B.up2(x0[b:b + 1])[0] * A) + (B.U16 + 2 * B.U32) * (np.abs(b3 * A) + np.abs(S))
        bound[b] = B._conv3(dz * (1 + 2.0 ** -9), np.abs(rgb_w))
    print("tail_ref vs biggan_ops_ref.tail %s: max distance %.3e, worst distance / bound %.3f" % (shape, dist.max(), (dist / bound).max()))
    assert (dist <= bound).all()


def test_gemm_ref_is_the_float64_product():
    a, w = B.gemm_inputs(192, 64, 256)
    ref, tol = B.gemm_ref(a, w, 0)
    assert np.array_equal(ref, np.stack([a[z].astype(f64) @ w[z].astype(f64).T for z in range(3)])) or np.allclose(ref, np.stack([a[z].astype(f64) @ w[z].astype(f64).T for z in range(3)]), rtol=0, atol=1e-12)
    assert (tol > 0).all()


# ---- a faithful kernel sits inside every bound and equals every lattice mirror ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.BG_CASES))
def test_conv_bound_admits_a_faithful_kernel_and_is_not_above_the_old_bar(name):
    inp = R.bg_case(name)
    old = R.OLD_BAR * np.abs(_plain(inp, True)).max()          # the old assertion: 5e-3 max|ref| of the unmirrored float64 reference
    for pf in _forms(inp):
        ref, tol = R.conv_ref(inp, _family(inp), pf)
        got = R.Emulation(inp, _family(inp), pf).finish()
        ratio = (np.abs(got - ref) / tol).max()
        print("%-32s %s: emulation worst err/tol %.3f, max tol / old bar %.3f" % (name, pf, ratio, tol.max() / old))
        assert np.isfinite(got).all() and ratio <= 1.0
        assert tol.max() <= old, "%s: the per-element bound reaches %.3e, above the old bar %.3e" % (name, tol.max(), old)


@pytest.mark.parametrize("name", R.BG_LATTICE)
def test_conv_lattice_mirror_is_bit_equal(name):
    inp, want = R.bg_case(name, lattice=True)
    for pf in R.PRE_FORMS:
        got = R.Emulation(inp, _family(inp), pf).finish()
        if inp.get("rgb_tanh"):
            assert np.abs(got - np.tanh(want)).max() <= B.tanh_term(want)
        else:
            assert np.array_equal(got, want)
    assert (want != 0).mean() > 0.25                             # (the ReLU leaves enough of the map alive)


@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_bound_admits_a_faithful_kernel(shape):
    """Under every form.  The counted bound is a WORST CASE over the 9 x 128 fp16 roundings of z that reach a pixel and comes out at 1.5e-2 ..
    2.5e-2 — above the 4e-3 this kernel was held to.  So it replaces nothing: test_gpu_biggan_ops.py::test_tail asserts both, and the sharp
    check of bg_tail is its lattice run.  Asserted here: the emulation is inside both, and the figures are printed."""
    inp = B.tail_inputs(*shape)
    for cc, tf in B.TAIL_FORMS:
        ref, tol, _ = B.tail_ref(*inp, cc_form=cc, t_form=tf)
        err = np.abs(B.tail_emulation(inp, cc, tf) - ref)
        print("tail %s %s/%s: emulation worst err/tol %.3f, max err %.3e; tol max %.3e median %.3e (old bar %.1e)" % (shape, cc, tf, (err / tol).max(), err.max(), tol.max(), np.median(tol), TAIL_OLD))
        assert (err <= tol).all() and err.max() <= TAIL_OLD


@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_lattice_mirror(shape):
    inp, s = B.tail_lattice(*shape)
    term = B.tanh_term(s)
    for cc, tf in B.TAIL_FORMS:
        assert np.abs(B.tail_emulation(inp, cc, tf) - np.tanh(s)).max() <= term
    assert (s != B.h16(s)).mean() >= 0.25                        # (a pre-tanh value rounded to fp16 would show)


@pytest.mark.parametrize("M,N,K,mode", GEMM_CASES)
def test_gemm_bound_lattice_and_old_bar(M, N, K, mode):
    a, w = B.gemm_inputs(M, N, K)
    ref, tol = B.gemm_ref(a, w, mode)
    err = np.abs(B.gemm_emulation(a, w, mode) - ref)
    old = GEMM_OLD[mode] * np.abs(ref).max()
    print("gemm %s mode %d: emulation worst err/tol %.3f, max tol / old bar %.3f" % ((M, N, K), mode, (err / tol).max(), tol.max() / old))
    assert (err <= tol).all() and tol.max() <= old
    la, lw, want = B.gemm_lattice(M, N, K, mode)
    assert np.array_equal(B.gemm_emulation(la, lw, mode), want)


# ---- planted defects ----------------------------------------------------------------------------------------------------------------------------------
def _conv_defect(what, name, plant, forms=None, lattice_name=None):
    """plant(em, inp) -> the defective output.  New bar: beyond the bound of EVERY form on the random map, or different from the lattice mirror.
    Old bar: 5e-3 max|ref| on the random map."""
    inp = R.bg_case(name)
    fam = _family(inp)
    got = plant(R.Emulation(inp, fam), inp)
    beyond = []
    for pf in forms or _forms(inp):
        ref, tol = R.conv_ref(inp, fam, pf)
        beyond.append(int((np.abs(got - ref) > tol).sum()))
    plain = _plain(inp, True)
    old_passed = np.abs(got - plain).max() <= R.OLD_BAR * np.abs(plain).max()
    lat, want = R.bg_case(lattice_name or name, lattice=True)
    lgot = plant(R.Emulation(lat, _family(lat)), lat)
    differs = bool((np.abs(lgot - np.tanh(want)) > B.tanh_term(want)).any()) if lat.get("rgb_tanh") else not np.array_equal(lgot, want)
    caught = min(beyond) > 0 or differs
    _report("%s [%s]: beyond the bound %s, lattice %s" % (what, name, beyond, "differs" if differs else "equal"), caught, old_passed)
    assert caught
    return min(beyond) > 0, differs, old_passed


def test_planted_accumulator_rounded_to_fp16():
    """Caught by the bound at K = 64 .. 288.  At K = 1152 (conv_glds at 128 channels) it is NOT: 2^-11 |acc| lies inside (2 K + 8) 2^-24 sum |a b|
    there, the price of an order-free summation bound — printed, not asserted; the lattice accumulators fit fp16 and cannot see it either."""
    plant = lambda em, inp: em.finish(acc=R.h16(em.acc))
    for name in ("conv0 tiled 24x64", "conv3 tiled res_cs 128 up1", "conv2 tiled"):
        assert _conv_defect("accumulator rounded to fp16 before dscale / shift", name, plant)[0]
    inp = R.bg_case("conv2 glds<16>")
    ref, tol = R.conv_ref(inp, "conv_glds")
    got = plant(R.Emulation(inp, "conv_glds"), inp)
    _report("accumulator rounded to fp16 before dscale / shift [conv2 glds<16>, K = 1152]: beyond the bound %d" % int((np.abs(got - ref) > tol).sum()),
            bool((np.abs(got - ref) > tol).any()), True)


def test_planted_tanh_of_the_fp16_value():
    on_random, on_lattice, _ = _conv_defect("tanh of the fp16-rounded v (fused rgb_tanh)", "final tanh 8x32", lambda em, inp: em.finish(tanh_of_fp16=True))
    assert on_lattice            # (the bias of 14 fractional bits is there for this)


def test_planted_wrong_tables():
    _conv_defect("fp32 tables where conv_tiled takes the fp16 ones", "conv0 tiled 24x64", lambda em, inp: R.Emulation(inp, em.family, table="sn").finish())
    _conv_defect("fp16 tables where conv_direct takes the fp32 ones", "conv0 direct 8x8", lambda em, inp: R.Emulation(inp, em.family, table="sn16").finish())


def test_planted_separate_rounding_where_the_build_contracts():
    """Measured against the as-built form alone ("fma"): on the lattice both forms are the same bits by construction, so only the bound can see it."""
    _conv_defect("mul + add where the build has an fma (input affine)", "conv0 tiled 24x64", lambda em, inp: R.Emulation(inp, em.family, "sep").finish(), forms=("fma",))


def _affine_on_padding(em, inp):
    """The input affine applied to the padding pixels of the right border column: relu(S) instead of 0."""
    a = np.pad(em.a, ((0, 0), (1, 1), (1, 1), (0, 0)))
    zero = np.zeros_like(inp["x"][:, :1, :1])
    a[:, 1:-1, -1, :] = R.pre_affine(zero, inp["sn"], inp["pre_shift"], em.table, "fma")[:, 0]
    return em.finish(acc=R._conv(a, em.b, em.KS, 1, 0, torch.float32))


def test_planted_affine_on_padding_pixels():
    _conv_defect("input affine applied to one padding column", "final tanh 8x32", _affine_on_padding)


def test_planted_relu_before_the_shift():
    _conv_defect("ReLU taken before the shift is added", "conv2 tiled", lambda em, inp: em.finish(relu_before_shift=True))


def _in_up_row(em, inp):
    """(iy + 1) >> 1 on the last row where it stays inside the stored map: iy = H - 3 (at iy = H - 1 the index leaves the map)."""
    a = em.a.copy()
    H = a.shape[1]
    a[:, H - 3] = a[:, H - 2]
    return em.finish(acc=em.accumulate(a, em.b))


def test_planted_in_up_row():
    _conv_defect("in_up reads row (iy + 1) >> 1 at iy = H - 3", "conv1 tiled up 32", _in_up_row)


def _res_stride(em, inp):
    r = np.asarray(inp["res"])
    B_, h, w, rcs = r.shape
    Cout = inp["w"].shape[0]
    flat = r.reshape(B_, -1)
    rr = np.stack([flat[:, p * Cout:(p + 1) * Cout] for p in range(h * w)], axis=1).reshape(B_, h, w, Cout)
    return em.finish(res=R.up2(rr) if inp.get("res_up") else rr)


def test_planted_residual_stride():
    _conv_defect("residual read with stride Cout where res_cs applies", "conv3 tiled res_cs 128 up1", _res_stride)


def _res_neighbour(em, inp):
    """Output row 0 of candidate b >= 1 reads the residual row of candidate b - 1's last row."""
    r = R.residual(inp).copy()
    r[1:, 0] = r[:-1, -1]
    return em.finish(res=r)


def test_planted_residual_row_of_the_neighbouring_candidate():
    _conv_defect("residual row of the neighbouring candidate at a batch boundary", "conv3 gemm res_cs 128 up1", _res_neighbour)


def test_planted_residual_before_the_relu():
    """conv_3 has no activation, so the defect is planted on its inputs with act = 2 (no engine layer has both; the bound does not care)."""
    def plant(em, inp):
        inp2 = dict(inp, act=2)
        return R.Emulation(inp2, em.family).finish(res_before_act=True)
    inp = dict(R.bg_case("conv3 direct res_cs 128 up1"), act=2)
    ref, tol = R.conv_ref(inp, "conv_direct")
    got = plant(R.Emulation(inp, "conv_direct"), inp)
    beyond = int((np.abs(got - ref) > tol).sum())
    lat, _ = R.bg_case("conv3 direct res_cs 128 up1", lattice=True)
    lat = dict(lat, act=2)
    differs = not np.array_equal(plant(R.Emulation(lat, "conv_direct"), lat), R.Emulation(lat, "conv_direct").finish())
    _report("residual added before the ReLU [conv3 inputs, act 2]: beyond %d, lattice %s" % (beyond, "differs" if differs else "equal"),
            beyond > 0 or differs, np.abs(got - ref).max() <= R.OLD_BAR * np.abs(ref).max())
    assert beyond > 0 and differs


@pytest.mark.parametrize("defect", B.TAIL_DEFECTS)
def test_planted_tail_defects(defect):
    """(3, 64) on a grid of 40 workgroups, so that tiles 40 .. 47 take the cross-tile prefetch path as (9, 128) does on the device's 512."""
    shape, grid = (3, 64), 40
    inp = B.tail_inputs(*shape)
    got = B.tail_emulation(inp, defect=defect, grid=grid)
    beyond = []
    for cc, tf in B.TAIL_FORMS:
        ref, tol, _ = B.tail_ref(*inp, cc_form=cc, t_form=tf)
        beyond.append(int((np.abs(got - ref) > tol).sum()))
    old_passed = np.abs(got - B.tail(*inp)).max() <= TAIL_OLD
    lat, s = B.tail_lattice(*shape)
    differs = bool((np.abs(B.tail_emulation(lat, defect=defect, grid=grid) - np.tanh(s)) > B.tanh_term(s)).any())
    _report("bg_tail %s: beyond the bound %s, lattice %s" % (defect, beyond, "differs" if differs else "equal"), min(beyond) > 0 or differs, old_passed)
    assert min(beyond) > 0 and differs


def test_planted_tail_pre_tanh_value_rounded_to_fp16():
    """One fp16 rounding too many, the defect class the old bar cannot see: 2^-11 |s| is ~2e-4, the bar 4e-3.  Only the lattice run catches it."""
    inp, s = B.tail_lattice(1, 32)
    got = np.tanh(B.h16(s).astype(f32))
    differs = bool((np.abs(got - np.tanh(s)) > B.tanh_term(s)).any())
    rnd = B.tail_inputs(1, 32)
    ref, tol, sr = B.tail_ref(*rnd)
    bad = np.tanh(B.h16(sr).astype(f32))
    _report("bg_tail pre-tanh value rounded to fp16: beyond the counted bound %d, lattice %s" % (int((np.abs(bad - ref) > tol).sum()), "differs" if differs else "equal"),
            differs, np.abs(bad - ref).max() <= TAIL_OLD)
    assert differs


@pytest.mark.parametrize("defect,shape", [("neighbour_w", (128, 64, 256, 0)), ("k_step", (128, 128, 1024, 0))])
def test_planted_gemm_defects(defect, shape):
    M, N, K, mode = shape
    a, w = B.gemm_inputs(M, N, K)
    ref, tol = B.gemm_ref(a, w, mode)
    got = B.gemm_emulation(a, w, mode, defect)
    beyond = int((np.abs(got - ref) > tol).sum())
    la, lw, want = B.gemm_lattice(M, N, K, mode)
    differs = not np.array_equal(B.gemm_emulation(la, lw, mode, defect), want)
    _report("batched gemm %s %s: beyond the bound %d, lattice %s" % (defect, shape, beyond, "differs" if differs else "equal"), beyond > 0 or differs,
            np.abs(got - ref).max() <= GEMM_OLD[mode] * np.abs(ref).max())
    assert beyond > 0 and differs
