"""The conv forms only the StyleGAN2 host builds (csrc/stylegan2.cpp g_conv_params / up_link / torgb_conv_params), one kernel at a time
against oracle.stylegan2_ref through the diagnostic ABI (include/glass_ops.h: premod, post_scale, y_planar8, trgb_partial):

  * per-sample pre-modulated weights (w_bstride != 0): modulate_weights_kernel, the lean up-conv instance upfir2_kernel<false>, the weight
    reloads of conv_wreg / conv_stream and the per-candidate weight pointers of conv_tiled / conv_glds;
  * the up-conv -> conv link: the consumer's style on the up-conv's output (post_scale16) and the chunk-planar store (y_planar8);
  * the toRGB partial sums of the blocks wider than 128 channels (trgb_part + trgb_finish_kernel).

Bars.  Oracle parity: 5e-3 * max|ref|, the bar test_gpu_ops.py::test_conv_modulated_* apply to the same layers in their activation-side
form (a float64 conv with the device's twice-rounded weights lies within 4e-4 * max|ref| of the oracle; the device adds its fp16 stores).
Fused toRGB: 2e-5 * max|ref|, the bar of test_conv_epilogue_fused_torgb (hi / lo fp16 tables, fp32 accumulation; the partial form adds
at most four fp32 additions).  Styles come from style_tables on random latents: sn changes sign and differs by O(1) between candidates,
so a kernel that reads another candidate's weights is wrong by O(1)."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clip_glass_amd import synth
from oracle import stylegan2_ref as sg
from util import _torgb_ref, check, nchw, nhwc, style_tables

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
ops = None


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global ops
    from clip_glass_amd import ops as _ops
    ops = _ops
    yield


def h16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def _layer(seed, B, H, Cin, Cout, up=False, batch_size=1, W=None, L=24):
    """One modulated 3x3 layer as _modconv_case (test_gpu_ops.py) builds it: fp16-rounded x (NCHW), style affine on random latents."""
    W = H if W is None else W
    r = lambda name, shape, std=1.0: synth.normal(seed, name, shape, std)
    c = SimpleNamespace(B=B, H=H, W=W, Cin=Cin, Cout=Cout, up=up, batch_size=batch_size, strength=0.37)
    c.x = h16(r("x", (B, Cin, H, W)))
    c.w = r("w", (Cout, Cin, 3, 3)); c.lat = r("lat", (B, L)); c.A = r("A", (Cin, L)); c.Ab = r("Ab", (Cin,), 0.2) + 1
    c.bias = r("b", (Cout,), 0.3)
    c.Ho, c.Wo = (2 * H, 2 * W) if up else (H, W)
    c.noise = r("noise", (B // batch_size, c.Ho, c.Wo))
    c.sn, c.smax, c.dscale = style_tables(c.lat, c.A, c.Ab, c.w, demod=True)
    return c


def _kw(c):
    return dict(up=c.up, sn=c.sn, dscale=c.dscale, noise=c.noise, noise_strength=c.strength, batch_size=c.batch_size, bias=c.bias, act=True)


def _oracle(c, lo=0, hi=None):
    """sg._mod_conv + noise + sg._bias_act of candidates [lo, hi), NCHW."""
    hi = c.B if hi is None else hi
    ref = sg._mod_conv(torch.tensor(c.x[lo:hi]), torch.tensor(c.lat[lo:hi]), torch.tensor(c.w), torch.tensor(c.A), torch.tensor(c.Ab),
                       demod=True, up=c.up)
    nz = torch.tensor(c.noise).repeat_interleave(c.batch_size, dim=0)[lo:hi, None]
    return sg._bias_act(ref + c.strength * nz, torch.tensor(c.bias)).numpy()


_cases = {}


def _up_case(B, H, Cin, Cout, bs):
    """An up-conv layer, its oracle output and the lean instance's (upfir2_kernel<false>) pixel-major output: computed once, shared."""
    key = (B, H, Cin, Cout, bs)
    if key not in _cases:
        c = _layer(51, B, H, Cin, Cout, up=True, batch_size=bs)
        c.ref = _oracle(c)
        c.lean = ops.conv(nhwc(c.x), c.w, impl=3, premod=True, **_kw(c))
        _cases[key] = c
    return _cases[key]


def _rgb(seed, B, C, Ho, Wo, with_skip):
    rng = np.random.default_rng(seed)
    t = dict(w=(rng.standard_normal((3, C)) / math.sqrt(C)).astype(np.float32), b=(rng.standard_normal(3) * 0.1).astype(np.float32),
             sn=rng.uniform(-1.0, 1.0, (B, C)).astype(np.float32), smax=rng.uniform(0.5, 3.0, B).astype(np.float32))
    t["yprev"] = rng.standard_normal((B, 3, Ho // 2, Wo // 2)).astype(np.float32) if with_skip else None
    return t


def _rgb_ref(feat, t):
    return _torgb_ref(feat, t["w"], t["b"], t["sn"], t["smax"], t["yprev"])


# ---- (a) the lean up-conv instance against the oracle ---------------------------------------------------------------------------
UP_SHAPES = [(2, 16, 32, 32, 2),       # one tile
             (3, 40, 32, 96, 1),       # three n tiles, ragged last tile and segment
             (4, 64, 64, 64, 2),
             (2, 128, 128, 64, 1)]     # the r256 -> r512 geometry


@pytest.mark.parametrize("B,H,Cin,Cout,bs", UP_SHAPES)
def test_lean_upconv_matches_oracle(B, H, Cin, Cout, bs):
    """upfir2_kernel<false> (per-sample weights from modulate_weights_kernel, one candidate per grid) against sg._mod_conv(up=True)."""
    c = _up_case(B, H, Cin, Cout, bs)
    check("lean up-conv B%d H%d %d->%d" % (B, H, Cin, Cout), nchw(c.lean), c.ref, 5e-3)


def test_lean_upconv_rolling_segments():
    """The launcher's own rule reaches S >= 2 (segments of several 16-row steps, the FIR window carried from step to step) only from 2048
    workgroups on: 6 candidates x 9 tiles x 19 segments x 2 n tiles = 2052 at S = 2 (upfir.hip launch_upfir2, TR = 16: 28 rows per
    segment, 514 virtual rows).  Compared candidate by candidate (one candidate's oracle map at a time)."""
    B, H, Cin, Cout = 6, 256, 32, 64
    assert B * ((2 * (H + 1) - 2 + 59) // 60) * ((2 * (H + 1) - 2 + 27) // 28) * (Cout // 32) >= 2048
    c = _layer(52, B, H, Cin, Cout, up=True, batch_size=2)
    got = ops.conv(nhwc(c.x), c.w, impl=3, premod=True, **_kw(c))
    for b in range(B):
        check("lean up-conv S = 2, candidate %d" % b, nchw(got[b:b + 1]), _oracle(c, b, b + 1), 5e-3)


# ---- (b) the chunk-planar store ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,Cin,Cout,bs", UP_SHAPES)
def test_lean_upconv_planar_store(B, H, Cin, Cout, bs):
    """y_planar8: the same values at [B][Cout / 8][Ho][Wo][8] (what conv_wreg reads) — bitwise, for 32, 64 and 96 channels."""
    c = _up_case(B, H, Cin, Cout, bs)
    np.testing.assert_array_equal(ops.conv(nhwc(c.x), c.w, impl=3, premod=True, planar_y=True, **_kw(c)), c.lean)


def test_planar_store_needs_the_lean_instance():
    c = _layer(51, 2, 16, 32, 32, up=True, batch_size=2)
    with pytest.raises(Exception):             # upfir2_kernel<true> does not write the layout: refused, not ignored
        ops.conv(nhwc(c.x), c.w, impl=3, planar_y=True, **_kw(c))


# ---- (c) the consumer's style on the up-conv's output --------------------------------------------------------------------------------
def _consumer(c, Cout2, seed=53):
    """The block's second conv (its input: the up-conv's output), with its own latent."""
    return _layer(seed, c.B, c.Ho, c.Cout, Cout2, up=False, batch_size=c.batch_size)


@pytest.mark.parametrize("premod", [False, True])
@pytest.mark.parametrize("B,H,Cin,Cout,bs,Cout2,impls2", [(2, 16, 32, 32, 2, 64, (2,)),       # consumer on conv_tiled
                                                          (4, 64, 64, 64, 2, 64, (2, 5))])   # and on conv_wreg (128 x 128, 64 -> 64)
def test_upconv_post_scale(premod, B, H, Cin, Cout, bs, Cout2, impls2):
    """post_scale16 on both instances (upfir2_kernel<true> / <false>): the layer's output times the consumer's style; and the consumer run
    without its activation-side style on that map computes what sg._mod_conv computes from the unscaled map (the engine's up_link move)."""
    c = _up_case(B, H, Cin, Cout, bs)
    n = _consumer(c, Cout2)
    plain = c.lean if premod else ops.conv(nhwc(c.x), c.w, impl=3, **_kw(c))
    scaled = ops.conv(nhwc(c.x), c.w, impl=3, premod=premod, post_scale=n.sn, **_kw(c))
    check("up-conv post_scale premod%d H%d" % (premod, H), nchw(scaled), c.ref * n.sn[:, :, None, None], 5e-3)
    kw2 = _kw(n)
    kw2["sn"] = None
    n.x = nchw(plain)                           # the unscaled DEVICE map (fp16 values) under the second layer's latent
    ref2 = _oracle(n)
    for impl2 in impls2:
        got = ops.conv(scaled, n.w, impl=impl2, **kw2)
        check("up-conv -> conv link premod%d impl%d" % (premod, impl2), nchw(got), ref2, 5e-3)
        if impl2 == 5:                          # the engine's pair hands the map over chunk-planar: same values
            np.testing.assert_array_equal(got, ops.conv(scaled, n.w, impl=5, planar_x=True, **kw2))


@pytest.mark.parametrize("impl", [1, 2, 4, 5])
def test_post_scale_refused_where_not_implemented(impl):
    """conv_direct / conv_tiled / conv_stream / conv_glds do not apply post_scale16: they refuse the launch instead of storing the
    unscaled map."""
    if impl in (1, 2):       # the folded up-conv
        c = _layer(54, 2, 32, 32, 32, up=True)
    elif impl == 4:
        c = _layer(54, 1, 256, 32, 32, W=1056)
    else:
        c = _layer(54, 2, 32, 128, 128)
    ops.conv(nhwc(c.x), c.w, impl=impl, **_kw(c))                       # the launcher takes the layer ...
    with pytest.raises(Exception):                                        # ... and refuses the field
        ops.conv(nhwc(c.x), c.w, impl=impl, post_scale=np.ones((c.B, c.Cout), np.float32), **_kw(c))


# ---- (d) pre-modulated stride-1 convs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl,B,H,W,Cin,Cout,bs", [
    (2, 2, 32, 32, 32, 64, 1),          # conv_tiled
    (2, 4, 64, 64, 64, 64, 2),
    (5, 3, 32, 96, 128, 128, 1),        # conv_glds_kernel (6 tiles x 64 nominal candidates < 2 per CU)
    (5, 16, 128, 128, 128, 128, 2),     # conv_gldsp_kernel, the persistent form: 16 x 32 work items
    (4, 3, 256, 1056, 32, 32, 1),       # conv_stream: uneven tile ranges per workgroup, candidate switches inside a range
])
def test_premod_conv_matches_oracle(impl, B, H, W, Cin, Cout, bs):
    c = _layer(55, B, H, Cin, Cout, batch_size=bs, W=W)
    got = ops.conv(nhwc(c.x), c.w, impl=impl, premod=True, **_kw(c))
    check("premod conv impl%d B%d %dx%d %d->%d" % (impl, B, H, W, Cin, Cout), nchw(got), _oracle(c), 5e-3)


def test_premod_conv_wreg_reload_inside_a_range():
    """conv_wreg keeps the whole weight tensor in registers and reloads it where a workgroup's tile range crosses into the next
    candidate (reload = has_next && w_bstride != 0 && nxt.b != b).  64 tiles per candidate at 128 x 128: the range length
    ceil(B * 64 / CUs) must not divide 64, or every range ends where a candidate ends and the reload never runs."""
    from clip_glass_amd.engine import device_info
    cus = device_info(0)["cus"]             # what the launcher divides by (glass_cu_count)
    B = 9
    per_wg = (B * 64 + cus - 1) // cus
    assert per_wg > 1 and 64 % per_wg != 0, "B = %d on %d CUs: ranges of %d tiles never straddle two candidates" % (B, cus, per_wg)
    c = _layer(56, B, 128, 64, 64, batch_size=1)
    got = ops.conv(nhwc(c.x), c.w, impl=5, premod=True, **_kw(c))
    check("premod conv_wreg B%d (ranges of %d tiles)" % (B, per_wg), nchw(got), _oracle(c), 5e-3)


# ---- (e) pre-modulated conv + fused toRGB -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("impl,B,H,W,C", [(2, 3, 32, 96, 64),          # conv_tiled<torgb>
                                          (5, 9, 128, 128, 64),        # conv_wreg<torgb>: 576 tiles, ranges of 3 on 256 CUs cross candidates
                                          (5, 3, 32, 96, 128),         # conv_glds<torgb>
                                          (4, 3, 256, 1056, 32)])      # conv_stream<torgb> (does not store the map)
def test_premod_conv_fused_torgb(impl, B, H, W, C, with_skip):
    c = _layer(57, B, H, C, C, batch_size=1, W=W)
    t = _rgb(58, B, C, H, W, with_skip)
    x = nhwc(c.x)
    if impl == 4:
        got = ops.conv(x, c.w, impl=4, premod=True, torgb=t, **_kw(c))
        feat = ops.conv(x, c.w, impl=4, premod=True, **_kw(c))
    else:
        got, feat = ops.conv(x, c.w, impl=impl, premod=True, torgb=t, both=True, **_kw(c))
        np.testing.assert_array_equal(feat, ops.conv(x, c.w, impl=impl, premod=True, **_kw(c)))
    check("premod fused toRGB impl%d %d ch" % (impl, C), got, _rgb_ref(feat, t), 2e-5)


# ---- (f) toRGB partial sums ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("Cout", [256, 384, 512])
def test_torgb_partial_sums(Cout, with_skip):
    """conv_gldsp_kernel<torgb> with trgb_part (one partial image per 128-wide n tile, at [(n0 >> 7) * B + b]) + trgb_finish_kernel:
    against a float64 toRGB of the stored map and the separate toRGB pass; the stored map is the launch's without toRGB."""
    B, H, Cin = 16, 64, 128                  # 16 x 8 pixel tiles x Cout / 128 n tiles on the persistent form
    c = _layer(59, B, H, Cin, Cout, batch_size=2)
    t = _rgb(60, B, Cout, H, H, with_skip)
    x = nhwc(c.x)
    got, feat = ops.conv(x, c.w, impl=5, torgb=t, trgb_partial=True, both=True, **_kw(c))
    np.testing.assert_array_equal(feat, ops.conv(x, c.w, impl=5, **_kw(c)))
    check("toRGB partial sums %d ch" % Cout, got, _rgb_ref(feat, t), 2e-5)
    if Cout & (Cout - 1) == 0:               # (launch_torgb is instantiated for power-of-two widths)
        check("toRGB partial sums %d ch vs the separate pass" % Cout, got, ops.torgb(feat, t["w"], t["b"], t["sn"], t["smax"], t["yprev"]), 2e-5)


def test_torgb_partial_sums_need_the_persistent_form():
    c = _layer(59, 2, 32, 128, 256)          # 2 x 1 tiles x 2 n tiles x 64 nominal candidates < 2 per CU: conv_glds_kernel, which has no partial store
    t = _rgb(60, 2, 256, 32, 32, False)
    ops.conv(nhwc(c.x), c.w, impl=5, **_kw(c))
    with pytest.raises(Exception):
        ops.conv(nhwc(c.x), c.w, impl=5, torgb=t, trgb_partial=True, both=True, **_kw(c))


# ---- (g) modulate_weights_kernel on its own ---------------------------------------------------------------------------------------
def _premod_model(c):
    """float64 conv of x with the device's own weights h16(h16(w * coef) * sn * dscale) (glass_pack_conv, modulate_weights_kernel); up:
    conv_transpose2d(stride 2), pad 1, [1,3,3,1] x [1,3,3,1] / 16.  No noise, bias or activation.  NCHW."""
    coef = 1.0 / math.sqrt(c.Cin * 9)
    wp = h16(c.w * np.float32(coef)).astype(np.float64)
    wm = h16(wp[None] * c.sn.astype(np.float64)[:, None, :, None, None] * c.dscale.astype(np.float64)[:, :, None, None, None])
    xg = torch.tensor(c.x, dtype=torch.float64).reshape(1, c.B * c.Cin, c.H, c.W)
    wt = torch.tensor(wm, dtype=torch.float64)
    if not c.up:
        y = F.conv2d(xg, wt.reshape(c.B * c.Cout, c.Cin, 3, 3), padding=1, groups=c.B)
    else:
        y = F.conv_transpose2d(xg, wt.transpose(1, 2).reshape(c.B * c.Cin, c.Cout, 3, 3), stride=2, groups=c.B)
        k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64)
        k = (k[:, None] * k[None, :]) / 16
        y = F.conv2d(F.pad(y, [1, 1, 1, 1]), k[None, None].repeat(c.B * c.Cout, 1, 1, 1), groups=c.B * c.Cout)
    return y.reshape(c.B, c.Cout, c.Ho, c.Wo).numpy()


@pytest.mark.parametrize("up", [False, True])
def test_premod_weights_float64_model(up):
    """Separates "weights modulated wrongly" from "conv wrong": the pre-modulated launch, no epilogue terms, against a float64 conv with
    the weights as modulate_weights_kernel must have written them.
    Bars.  Stride 1 (conv_tiled): the result is the fp32 accumulator rounded to fp16 once — half an ulp, 2^-11 relative; 2 x 2^-11 *
    max|ref| leaves the same again for the fp32 accumulation and for a modulated weight whose fp32 product rounds to the other fp16
    neighbour than the float64 product's.  Up (upfir2_kernel<false>): the T tile and the separable FIR are packed fp16 — the same error
    sources the oracle-parity bar of the up-convs (5e-3 * max|ref|) was set for, minus the 4e-4 of the weight rounding that the model
    carries itself: the same bar.  A wrong style or demodulation row is an O(1) error under either."""
    c = _layer(61, 3, 32, 32, 64, up=up)
    got = ops.conv(nhwc(c.x), c.w, up=up, sn=c.sn, dscale=c.dscale, impl=3 if up else 2, premod=True)
    check("premod weights, float64 model, up%d" % up, nchw(got), _premod_model(c), 5e-3 if up else 2 * 2.0 ** -11)
