"""The stride-1 3x3 / 1x1 convolution kernels behind glass_op_conv, one instance at a time, against the float64 reference and the PER-ELEMENT
bound of tests/conv_ops_ref.py (operand roundings mirrored exactly, everything after them exact; the bound is derived from each kernel's code
there, nothing is fitted).  The op stages every output poisoned and guarded (csrc/ops.hip): an element no thread stores is NaN, a store
outside the output is an error.  Every case asserts the kernel symbol it ran (ops.last_kernel()), the bound everywhere, and the bound again
on the four two-pixel border slices, so that a failure says where it is.

SHAPES (B, H, W, Cin, Cout) are the smallest each instance admits on a 256-CU part, as read from the choosers; the symbol assertion fails
where a part with another CU count chooses otherwise.
  conv_direct (choose_conv_direct, at the nominal population of 64): Neff <= 32 -> <1>; Neff in (32, 64] or too few blocks -> <2>;
      Neff > 64 and ceil(64 Hc Wc / 32) ceil(Neff / 128) >= 512 -> <4> (16 x 16: 512 exactly); ceil(64 Hc Wc / 128) ceil(Neff / 128) >= 256
      -> <4,rows> (16 x 32: 256 exactly).  Odd 5 x 7 images: the last 32-row tile is partial, rows of a tile cross samples.
  conv_tiled (choose_conv_tiled): TILED_PLAIN(3, 1, 8) by Neff % 128 / 64 / 32; W = 32, H = 8 is one tile per sample; Cin = 96 is three chunks;
      (1, 16, 64, 64, 128) is 2 x 2 tiles; <1,1,8,64> is the 1 x 1 form, pad 0.
  conv_glds (choose_conv_glds / glds_inst): W % 32 != 0 -> <16> (a whole 16 x 16 image per workgroup); Cin = 160 is an odd chunk count (Cin & 63),
      which the persistent ring does not take -> conv_glds_kernel<32>.  Persistent conv_gldsp: 64 (W / 32)(H / 16)(N / 128) >= 2 * 256, i.e.
      (W / 32)(H / 16)(N / 128) >= 8: 32 x 64, N = 256.  B = 33 gives 264 items over 256 workgroups: eight run on into a second item.  The
      fused-toRGB instance needs N = 128 (one n tile), so its smallest persistent geometry is 64 x 64 (2 * 4 * 1 = 8), again B = 33; the
      partial-sum form (N = 256, square images: 64 x 64, 16 items a sample) runs at B = 17 (272 items).
  conv_wreg (choose_conv_wreg): 64 (W / 32)(H / 8) >= 16 * 256, i.e. (W / 32)(H / 8) >= 64: 128 x 128.  B = 5 is 320 tiles; launch_wreg deals
      ceil(320 / 256) = 2 tiles to each of 160 workgroups (every range is a ring of two tiles, the last tile of a sample and the first of
      the next are neighbours in the walk).
  conv_stream (choose_conv_stream): 64 (W / 32)(H / 8) >= 6 * 768, i.e. (W / 32)(H / 8) >= 72: 200 x 96 is 75.  B = 31 is 2325 tiles over 768
      slots: ceil = 4 tiles per workgroup in 582 workgroups, the last with one; 75 tiles a sample is odd, so ranges cross samples.
  conv_gemm (launch_conv_gemm): the shapes of test_gpu_ops.py::test_conv_gemm_matches_direct — a style materialises the patch matrix (im2col),
      none lets the GEMM gather it, the plain 1 x 1 is one gemm_tiled launch.

MEASURED on the MI355X (worst err / tol per case, from the log util.diag writes; the table with shapes and symbols is in DESIGN.md, "Conv ops: what
the tests pin"):
  direct <1> 0.784, <2> full 0.926, <4> 0.860, <4,rows> 0.898, stride 2 + res 0.680, 1x1 0.964, broadcast 0.725
  tiled <3,1,8,32> 0.763, <3,1,8,64> 0.552, <3,1,8,128> 0.668, <1,1,8,64> 0.967
  glds <16> 0.476, <32> 0.368; gldsp <f,f,f> 0.510, <f,f,t> 0.531; gldsp<torgb> map 0.454 image 0.017, partial sums map 0.446 image 0.005
  wreg plain 0.609, full 0.625 (planar x, <xs> and <torgb> maps: the same bits), premod 0.686; wreg<torgb> image 0.031 / 0.035
  stream 0.693; stream<torgb> 0.059 / 0.067
  gemm conv8 0.413, const4 0.465, plain8 0.324, plain4 0.348, skip1x1 0.886
Every case sits below 1.  The bound's leading term is the fp16 store's half ulp, which some element of any output attains; the ratios near
0.9 are outputs just above a power of two, where 2^-11 |out| IS that half ulp.

The up-conv, the stride-2 and skip kernels, conv_down, conv_down64 and conv_d0 — whose packed-fp16 FIR chains need a rounding model of their own —
are in tests/test_gpu_fir_ops.py, against tests/fir_ops_ref.py."""
import os

import numpy as np
import pytest

import conv_ops_ref as R
from util import check, check_bound, diag

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
ops = None


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global ops
    from clip_glass_amd import ops as _ops
    ops = _ops
    yield


NHWC_BORDERS = (("top", np.s_[:, :2]), ("bottom", np.s_[:, -2:]), ("left", np.s_[:, :, :2]), ("right", np.s_[:, :, -2:]))
NCHW_BORDERS = (("top", np.s_[:, :, :2]), ("bottom", np.s_[:, :, -2:]), ("left", np.s_[:, :, :, :2]), ("right", np.s_[:, :, :, -2:]))


def bound_with_borders(name, got, ref, tol, borders=NHWC_BORDERS):
    check_bound(name, got, ref, tol)
    for side, sl in borders:
        check_bound("%s border %s" % (name, side), got[sl], ref[sl], tol[sl], log=False)


def ran(symbol):
    assert ops.last_kernel() == symbol, "the launch ran %r, this case is about %r" % (ops.last_kernel(), symbol)


def run_case(name):
    """Launch CASES[name], assert the symbol and the bound; returns (inp, ref, tol, got)."""
    family, impl, symbol, args = R.CASES[name]
    inp = R.make_inputs(**args)
    ref, tol = R.conv_ref(inp, family)
    got = ops.conv(inp["x"], inp["w"], impl=impl, **R.op_kwargs(inp))
    ran(symbol)
    bound_with_borders(name, got, ref, tol)
    return inp, ref, tol, got


PLAIN = [n for n in sorted(R.CASES) if n not in ("wreg full", "stream full", "gldsp<f,f,f>")]


@pytest.mark.parametrize("name", PLAIN)
def test_conv_instance_in_bound(name):
    run_case(name)


def _blur_down_ref(x):
    f = np.array([1, 3, 3, 1], dtype=np.float64) / 8
    B, H, W, _ = x.shape
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    return sum(f[a] * f[b] * xp[:, a:a + H:2, b:b + W:2] for a in range(4) for b in range(4))


def test_conv_gldsp_plain_and_blurdown_byproduct():
    """conv_gldsp_kernel<false,false,false> in bound; <false,true,false> (the blur-down by-product) stores the same map bit for bit, and its
    by-product at the bar test_gpu_ops.py has for it (the packed-fp16 FIR chain is outside this file's bounds)."""
    inp, ref, tol, got = run_case("gldsp<f,f,f>")
    xs = np.full((inp["B"], 16, 32, 128), np.nan, dtype=np.float32)
    y = ops.conv(inp["x"], inp["w"], impl=5, xs_out=xs, **R.op_kwargs(inp))
    ran("conv_gldsp_kernel<false,true,false>")
    np.testing.assert_array_equal(y, got)
    check("conv_gldsp blur-down by-product", xs, _blur_down_ref(inp["x"]), 2e-3)


def _fused_torgb(name, feat, got_rgb, t, C, partial=False):
    assert np.isfinite(feat).all(), "%s: the stored map holds non-finite values" % name
    ref, tol = R.torgb_ref(feat, t, C, partial)
    bound_with_borders(name, got_rgb, ref, tol, NCHW_BORDERS)


@pytest.mark.parametrize("form", ["torgb", "partial"])
def test_conv_gldsp_fused_torgb(form):
    """conv_gldsp_kernel<true,false,true>: toRGB from the tile in registers (one n tile) and as partial sums per n tile + trgb_finish_kernel.
    The stored map of three candidates (first, one in the middle of a workgroup's run, last) against the float64 bound; the image against the
    float64 toRGB of the kernel's own stored map."""
    B, C, Cout = (33, 128, 128) if form == "torgb" else (17, 128, 256)
    inp = R.make_inputs(B, 64, 64, C, Cout, **R.FULL)
    inp["out_scale"] = 1.0
    t = R.torgb_inputs(B, 64, 64, Cout, with_skip=True)
    rgb, feat = ops.conv(inp["x"], inp["w"], impl=5, torgb=t, both=True, trgb_partial=(form == "partial"), **R.op_kwargs(inp))
    ran("conv_gldsp_kernel<true,false,true>")
    idx = [0, B // 2, B - 1]
    ref, tol = R.conv_ref(R.take(inp, idx), "conv_glds")
    bound_with_borders("conv_gldsp<torgb> %s map" % form, feat[idx], ref, tol)
    _fused_torgb("conv_gldsp<torgb> %s image" % form, feat, rgb, t, Cout, partial=(form == "partial"))


def test_conv_wreg_forms():
    """conv_wreg at one geometry: the full epilogue; the chunk-planar input (the same bits); the blur-down by-product instance; the fused toRGB
    instance with and without the previous image."""
    inp, ref, tol, got = run_case("wreg full")
    kw = R.op_kwargs(inp)
    got_p = ops.conv(inp["x"], inp["w"], impl=5, planar_x=True, **kw)
    ran("conv_wreg_kernel<false,false>")
    bound_with_borders("wreg full planar_x", got_p, ref, tol)
    np.testing.assert_array_equal(got_p, got)
    xs = np.full((inp["B"], 64, 64, 64), np.nan, dtype=np.float32)
    y = ops.conv(inp["x"], inp["w"], impl=5, xs_out=xs, **kw)
    ran("conv_wreg_kernel<false,true>")
    bound_with_borders("wreg<xs> map", y, ref, tol)
    check("conv_wreg blur-down by-product", xs, _blur_down_ref(inp["x"]), 2e-3)
    for with_skip in (True, False):
        t = R.torgb_inputs(inp["B"], 128, 128, 64, with_skip)
        rgb, feat = ops.conv(inp["x"], inp["w"], impl=5, torgb=t, both=True, **kw)
        ran("conv_wreg_kernel<true,false>")
        bound_with_borders("wreg<torgb> map skip%d" % with_skip, feat, ref, tol)
        _fused_torgb("wreg<torgb> image skip%d" % with_skip, feat, rgb, t, 64)


def test_conv_stream_map_and_torgb():
    """conv_stream_kernel (the map) in bound, and conv_stream_kernel<torgb> — which never stores the map — against the float64 toRGB of the map
    form's stored output, with and without the previous image."""
    inp, ref, tol, feat = run_case("stream full")
    del ref, tol
    kw = R.op_kwargs(inp)
    for with_skip in (True, False):
        t = R.torgb_inputs(inp["B"], 200, 96, 32, with_skip)
        rgb = ops.conv(inp["x"], inp["w"], impl=4, torgb=t, **kw)
        ran("conv_stream_kernel<torgb>")
        _fused_torgb("conv_stream<torgb> skip%d" % with_skip, feat, rgb, t, 32)
    diag("[conv ops] poisoned + guarded staging, per-element float64 bounds: done")
