"""The kernels whose operands or outputs go through a packed-fp16 FIR chain — upfir2_kernel<true> / <false>, conv_down_kernel, conv_down64_kernel,
dblock0_kernel, conv_stream_kernel<fromrgb> + conv_down_kernel — and the stride-2 kernels with the fused skip branch (conv_s2_kernel,
conv_tiled<3,2,4,N,skip>) against tests/fir_ops_ref.py:

  bit for bit   on LATTICE inputs, where every MFMA accumulator is exact in any summation order and the rest of the kernel is a deterministic sequence of
                fp32 / packed-fp16 operations that numpy reproduces (np.testing.assert_array_equal against the mirror);
  per element   on RANDOM inputs, against a float64 reference of bit-exact fp16 operands (FIR included) with the bound (2 K + 8) U32 P + one fp16 store
                + 2^-24 — or, for the up-conv, whose FIR follows the MFMA, a bound counted rounding by rounding (fir_ops_ref.upfir_ref).

The op stages every output poisoned and guarded (csrc/ops.hip): an element no thread stores is NaN, a store outside the output is an error.  Every case
asserts the kernel symbol it ran, finiteness and the WHOLE output, then the four two-pixel border slices again so that a failure says where it is.
Where a packed a * b + c may compile to one rounding or two (fir_ops_ref's CONTRACTION FORMS) a case passes when ONE form — for the up-conv one of
the four combinations of its two sites — holds for the whole output; which one held is logged (util.diag) and recorded in DESIGN.md.

SHAPES: the up-conv grid shapes are test_conv_up_virtual_grid's (three images per virtual row at 8 x 8, empty slots, two grids, three n
tiles, three chunks), the lean ones test_lean_upconv_matches_oracle's; conv_down / conv_down64 / dblock0 run test_d_block_down_fused's,
test_d_block_down64's and test_dblock0_fused's first three (one tile column with both borders in every window; two columns; interior tiles, odd
counts, two-step ranges).  A launch whose float64 reference over all candidates would take more than a few seconds is referenced at three candidates
(first, middle, last) and checked for finiteness everywhere.  conv_tiled<3,2,4,128,skip,..> cannot be reached through the op on a 256-CU part: at
N = 128 conv_s2 takes every shape conv_tiled's skip form takes (64 (W / 32)(H / 8) >= 256 from 32 x 32 outputs on), so (2, 64, 64, 128)
at impl 2 asserts conv_s2_kernel; the 64-wide instance runs at (3, 64, 32, 64).

MEASURED on the MI355X: DESIGN.md, "FIR-chain kernels: what the tests pin"."""
import os

import numpy as np
import pytest

import fir_ops_ref as R
from util import check_bound, diag

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
ops = None


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global ops
    from clip_glass_amd import ops as _ops
    ops = _ops
    yield


BORDERS = (("top", np.s_[:, :2]), ("bottom", np.s_[:, -2:]), ("left", np.s_[:, :, :2]), ("right", np.s_[:, :, -2:]))


def ran(symbol):
    assert ops.last_kernel() == symbol, "the launch ran %r, this case is about %r" % (ops.last_kernel(), symbol)


def finite(name, got):
    assert np.isfinite(got).all(), "%s: %d non-finite values (an element no thread stored is NaN)" % (name, int((~np.isfinite(got)).sum()))


def in_bound(name, got, refs):
    """got is inside the per-element bound of ONE contraction form everywhere (and then on the border slices); refs(form) -> (ref, tol)."""
    tried = []
    for form in R.FORMS:
        ref, tol = refs(form)
        ratio = R.bound_ratio(got, ref, tol)
        tried.append("%s %.4f" % (form, ratio))
        if ratio <= 1:
            diag("[fir form] %-44s holds under %-4s (worst err/tol: %s)" % (name, form, ", ".join(tried)))
            check_bound(name, got, ref, tol)
            for side, sl in BORDERS:
                check_bound("%s border %s" % (name, side), got[sl], ref[sl], tol[sl], log=False)
            return form
    diag("[fir form] %-44s holds under NO form (worst err/tol: %s)" % (name, ", ".join(tried)))
    ref, tol = refs(R.FORMS[0])
    check_bound(name, got, ref, tol)        # fails, with the place
    raise AssertionError(name)


def bit_equal(name, got, mirrors):
    """got equals the mirror of ONE form (combination) bit for bit; mirrors: form -> array."""
    held = [form for form, m in mirrors.items() if np.array_equal(got, m)]
    diff = {form: int((got != m).sum()) for form, m in mirrors.items()}
    diag("[fir bits] %-44s equal under %s (elements that differ per form: %s)" % (name, held if held else "NO form", diff))
    if not held:
        best = min(diff, key=diff.get)
        np.testing.assert_array_equal(got, mirrors[best], err_msg="%s: closest form %s" % (name, best))
    return held


# ---- the up-conv ------------------------------------------------------------------------------------------------------------------------------------------
def _up_mirrors(inp, lean):
    T = R.up_T(inp, lean)
    return {form: R.up_chain(T, inp, form) for form in R.UP_FORMS}


@pytest.mark.parametrize("B,H,Cin,Cout,bs,ps", R.UP_GRID_CASES)
def test_upfir_grid_lattice_bit_exact(B, H, Cin, Cout, bs, ps):
    inp = R.lattice_up(B, H, Cin, Cout, bs, post_scale=ps)
    got = ops.conv(inp["x"], inp["w"], **R.up_kwargs(inp))
    ran("upfir2_kernel<true>")
    name = "upfir2<true> lattice B%d H%d %d->%d bs%d ps%d" % (B, H, Cin, Cout, bs, ps)
    finite(name, got)
    bit_equal(name, got, _up_mirrors(inp, False))


@pytest.mark.parametrize("B,H,Cin,Cout,bs,ps", R.UP_LEAN_CASES)
def test_upfir_lean_lattice_bit_exact(B, H, Cin, Cout, bs, ps):
    inp = R.lattice_up(B, H, Cin, Cout, bs, post_scale=ps)
    got = ops.conv(inp["x"], inp["w"], **R.up_kwargs(inp, premod=True))
    ran("upfir2_kernel<false>")
    name = "upfir2<false> lattice B%d H%d %d->%d bs%d ps%d" % (B, H, Cin, Cout, bs, ps)
    finite(name, got)
    bit_equal(name, got, _up_mirrors(inp, True))
    if (B, H, ps) == (2, 16, False):        # the chunk-planar store: the same bits (asserted at every shape in test_gpu_conv_engine_forms.py)
        np.testing.assert_array_equal(ops.conv(inp["x"], inp["w"], planar_y=True, **R.up_kwargs(inp, premod=True)), got)


def _up_counted(lean, seed, B, H, Cin, Cout, bs, ps):
    inp = R.up_inputs(seed, B, H, Cin, Cout, bs, post_scale=ps)
    got = ops.conv(inp["x"], inp["w"], **R.up_kwargs(inp, premod=lean))
    ran("upfir2_kernel<%s>" % ("false" if lean else "true"))
    name = "upfir2<%s> B%d H%d %d->%d bs%d ps%d" % ("false" if lean else "true", B, H, Cin, Cout, bs, ps)
    finite(name, got)
    idx = R.three(B) if B > 8 else list(range(B))
    ref, tol = R.upfir_ref(R.take_up(inp, idx), lean)
    check_bound(name, got[idx], ref, tol)
    for side, sl in BORDERS:
        check_bound("%s border %s" % (name, side), got[idx][sl], ref[sl], tol[sl], log=False)


@pytest.mark.parametrize("B,H,Cin,Cout,bs,ps", R.UP_GRID_CASES)
def test_upfir_grid_counted_bound(B, H, Cin, Cout, bs, ps):
    """test_gpu_ops._modconv_case's inputs (seed 3)."""
    _up_counted(False, 3, B, H, Cin, Cout, bs, ps)


@pytest.mark.parametrize("B,H,Cin,Cout,bs,ps", R.UP_LEAN_CASES)
def test_upfir_lean_counted_bound(B, H, Cin, Cout, bs, ps):
    """test_gpu_conv_engine_forms._layer's inputs (seed 51)."""
    _up_counted(True, 51, B, H, Cin, Cout, bs, ps)


# ---- conv_down, conv_down64 ---------------------------------------------------------------------------------------------------------------------------------
SYMBOL = {"conv_down": "conv_down_kernel", "conv_down64": "conv_down64_kernel"}


def _dblock_down(inp):
    return ops.dblock_down(inp["h"], inp["x"], inp["w1"], inp["ws"], inp["b1"])


@pytest.mark.parametrize("kernel,B,R_,Cin,Cout", R.DOWN_LATTICE_CASES)
def test_down_lattice_bit_exact(kernel, B, R_, Cin, Cout):
    """Lattice h, wskip = 0: both FIR passes are exact, so taps, masks, windows and tile walks are pinned to the last bit."""
    inp = R.lattice_down(B, R_, Cin, Cout)
    got = _dblock_down(inp)
    ran(SYMBOL[kernel])
    name = "%s lattice B%d R%d" % (kernel, B, R_)
    finite(name, got)
    inp["xs"] = ops.blur(inp["x"], 1)
    bit_equal(name, got, {form: R.down_mirror(kernel, inp, form) for form in R.FORMS})


@pytest.mark.parametrize("kernel,B,R_,Cin,Cout", R.DOWN_LATTICE_CASES[::2])
def test_down_skip_lattice_bit_exact(kernel, B, R_, Cin, Cout):
    """The skip branch on its own lattice (h = 0, b1 >= 0, x in {-1, 0, 1}, full-mantissa skip weights of one binade): launch_blur_down returns the
    exact skip input, and the skip rows' rounding h(ws16 * 0.70710678f) and the skip MFMAs' addressing are pinned to the last bit."""
    inp = R.lattice_down_skip(B, R_, Cin, Cout)
    np.testing.assert_array_equal(ops.blur(inp["x"], 1), inp["xs"])
    got = _dblock_down(inp)
    ran(SYMBOL[kernel])
    name = "%s skip lattice B%d R%d" % (kernel, B, R_)
    finite(name, got)
    bit_equal(name, got, {"any": R.down_mirror(kernel, inp)})


@pytest.mark.parametrize("kernel,B,R_,Cin,Cout", R.DOWN_CASES)
def test_down_in_bound(kernel, B, R_, Cin, Cout):
    """Random inputs; the skip input is ops.blur(x, 1): the same launch_blur_down the op runs (bounded by the glue tests)."""
    inp = R.down_inputs(B, R_, Cin, Cout)
    got = _dblock_down(inp)
    ran(SYMBOL[kernel])
    inp["xs"] = ops.blur(inp["x"], 1)
    in_bound("%s B%d R%d" % (kernel, B, R_), got, lambda form: R.down_ref(kernel, inp, form))


# ---- conv_s2, conv_tiled<3,2,4,N,skip> -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,B,R_,Cin,Cout", R.S2_CASES)
def test_stride2_skip_in_bound(kernel, B, R_, Cin, Cout):
    inp = R.s2_inputs(B, R_, Cin, Cout)
    kw = dict(stride=2, pad=0, bias=inp["b1"], act=True, out_scale=inp["out_scale"], skip=(inp["xs"], inp["ws"]))
    got = ops.conv(inp["hb"], inp["w1"], impl=5 if kernel == "conv_s2" else 2, **kw)
    if kernel == "conv_tiled_skip" and Cout % 128 == 0:
        kernel = "conv_s2"                   # (see the module docstring: conv_s2 takes this shape at impl 2 as well)
        ran("conv_s2_kernel")
    else:
        ran("conv_s2_kernel" if kernel == "conv_s2" else "conv_tiled_kernel<3,2,4,64,skip>")
    name = "%s B%d R%d %d->%d" % (kernel, B, R_, Cin, Cout)
    finite(name, got)
    idx = R.three(B) if B > 3 else list(range(B))
    ref, tol = R.down_ref(kernel, R.take_down(inp, idx))
    check_bound(name, got[idx], ref, tol)
    for side, sl in BORDERS:
        check_bound("%s border %s" % (name, side), got[idx][sl], ref[sl], tol[sl], log=False)
    if kernel == "conv_s2" and B <= 3:       # the blurred input in 32-channel planes: the same bits
        np.testing.assert_array_equal(got, ops.conv(inp["hb"], inp["w1"], impl=5, planar32_x=True, **kw))


# ---- dblock0 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R_", R.D0_CASES)
def test_dblock0_in_bound(B, R_):
    """A lattice front (y, fromRGB, w0, b0: x and h are exact, asserted by the builder) with random w1 / wskip: the operands of the LAST MFMAs are
    mirrored bit for bit — FIR pad 2 of h, horizontal pass first, and the skip input FIR pad 1 [::2] of x."""
    inp = R.lattice_dblock0(B, R_)
    args = R.dblock0_args(inp)
    got = ops.dblock0(*args)
    ran("dblock0_kernel")
    in_bound("dblock0 B%d R%d" % (B, R_), got, lambda form: R.dblock0_ref(inp, form))
    np.testing.assert_array_equal(got, ops.dblock0(*args, impl=2))          # the chunk-planar output: the same bits


def test_dblock0_two_kernel_form_in_bound():
    """conv_stream<fromrgb> + conv_down on the same lattice front: its own front mirror (the packed-fp16 fromRGB chain, exact here: the builder
    asserts that both forms' x and h are the same bits) and conv_down's FIR order."""
    B, R_ = R.D0_TWO_KERNEL_CASE
    inp = R.lattice_dblock0(B, R_)
    got = ops.dblock0(*R.dblock0_args(inp), impl=1)
    ran("conv_stream_kernel<fromrgb> + conv_down_kernel")
    in_bound("dblock0 two-kernel form B%d R%d" % (B, R_), got, lambda form: R.dblock0_ref(inp, form, "stream"))


@pytest.mark.parametrize("B,R_", R.D0_CASES[:2])
def test_dblock0_skip_lattice_bit_exact(B, R_):
    """The skip branch on its own lattice (h = 0, b1 >= 0, a never-negative fromRGB map of multiples of 1/2): P2's patch walk, the XS ring and the skip
    MFMAs are pinned to the last bit, at one step per workgroup (R = 64) and on the ragged 17-step columns of R = 68."""
    inp = R.lattice_dblock0_skip(B, R_)
    args = R.dblock0_args(inp)
    got = ops.dblock0(*args)
    ran("dblock0_kernel")
    name = "dblock0 skip lattice B%d R%d" % (B, R_)
    finite(name, got)
    bit_equal(name, got, {"any": R.dblock0_mirror(inp)})
    np.testing.assert_array_equal(got, ops.dblock0(*args, impl=2))
