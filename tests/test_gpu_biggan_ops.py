"""Every kernel the BigGAN-deep path launches (csrc/biggan.cpp), one at a time through the diagnostic ABI (include/glass_ops.h) against the
float64 restatements of tests/biggan_ops_ref.py — which tests/test_biggan_ops_ref.py pins to oracle/biggan_ref.py on the CPU.

Inputs make an indexing bug O(1): the per-candidate tables differ by O(1) between candidates and between channels and change sign, the
input shift S has a positive mean (a kernel that applies the affine to padding or halo pixels writes relu(S) != 0 there), maps are
non-square wherever the launcher takes them, B >= 2 everywhere.  Convolutions are compared on the fp16-rounded operands the op uploads
(x, and the weights as glass_pack_conv rounds them: h16(w / sqrt(Cin KS KS))).

Kernel instances reached (MI355X, 256 CUs; the launchers' own rules, csrc/*.hip):
  conv_tiled_kernel<1,1,8,32> / <1,1,8,64> / <1,1,8,128> / <3,1,8,32> (also with rgb_tanh_out) / <3,1,8,64>, conv_glds_kernel<16> / <32>,
  conv_stream_kernel, conv_gemm (im2col + gemm_tiled + finish: S = 1, 2; gather + gemm_tiled + finish: S = 1, 4), conv_direct_kernel<1> / <2>,
  gemm_tiled_kernel<64> / <128> (batched), gemm_direct_kernel<2> (batched, K = 32),
  bg_attn_split_vec_kernel, bg_attn_split_kernel, bg_softmax_reg_kernel<4>, bg_softmax_reg_kernel<1>, bg_softmax_kernel,
  bg_cond_kernel, dense + bg_bn_tables_kernel + bg_to_half_kernel, bg_rgb_tanh_kernel, bg_tail_kernel (1, 48 and 576 tiles: the last wraps
  the persistent loop of 2 x 256 workgroups).
The issue's conv1 / impl 6 case (8 x 8 from 4 x 4, 64 -> 64) does NOT split K: launch_conv_gemm needs K % (64 S) == 0 and 9 * 64 = 576 is
no multiple of 128.  It runs as the launcher decides (S = 1); 128 -> 128 at 8 x 8 (S = 2) and 256 -> 256 at 4 x 4 (S = 4) are added so
that both split forms — the im2col one and the gather one — run.

Bars.
  * Convolutions with an fp16 store: |err| <= 5e-3 * max|ref|, the project's bar (test_gpu_ops.py::test_conv_modulated_*).
  * conv_tiled with pre_shift16 (fp16 tables, packed fp16 fma while staging), additionally: with d = max |ref_rounded - ref_exact| of two
    float64 references (tables rounded to fp16 and relu(x A + S) rounded to fp16 once, against no rounding at all),
    |got - ref_exact| <= d + 2^-11 |ref_exact| + 2^-16 max|ref|.  The last term is the margin: K <= 1152 fp32 additions of random-sign
    roundings are ~ sqrt(K) 2^-24 ~ 2^-19 of partial sums that stay within a few max|ref|, plus three fp32 epilogue operations; 2^-16
    leaves a factor of eight.
  * Small fp32 kernels: 4 x the largest error of a plain float32 numpy restatement against float64 on the same inputs (+ 2^-11 |ref| where
    the kernel stores fp16).  The float32 restatements of the two kernels that sum many terms (bg_cond over the classes, the table product
    over cond) add them one after the other, as the kernels do.
  * bg_attn_split, bg_to_half, tab16: bit-exact.  cand_batch 0 / 1: bit-identical outputs.
  * bg_tail: max |err| <= 4e-3 on images in (-1, 1), the project's bar for this kernel (test_biggan_fused_last_stage_...); the border
    pixels' max error <= the interior's + the interior rms (the border is 1 / 8 .. 1 / 32 of the pixels, so its max is expected BELOW the
    interior's; one rms covers sampling, a padding bug is O(0.1)).  Weights are scaled as spectrally normalised Gaussian matrices are
    (sigma ~ sqrt(rows) + sqrt(cols)), so the pre-tanh values are O(0.5) and tanh does not hide an error by saturating.
  * The self-attention chain: 1e-2 * max|ref|, the bar of test_biggan_per_block_taps (gamma = 0.7).

Measured on an MI355X (max |err| / max|ref| unless stated; every figure is also logged through util.diag):
  conv0 form        impl 2: 4.5e-4 (8 x 32), 4.2e-4 (24 x 64); derived bar: d = 3.9e-3 / 4.5e-3 absolute at max|ref| 13, device 6.0e-3 / 5.7e-3 from
                    the exact reference and 3.9e-3 (one fp16 ulp of the store) from the rounded model, worst err / tol 0.75 / 0.82;
                    impl 6: 3.1e-4; impl 1: 2.9e-4; rms 4e-5 of max|ref| throughout
  conv1 form        impl 2: 3.2e-4 (32 ch), 2.6e-4 (64 ch); impl 6: 2.4e-4 (64, S = 1), 3.4e-4 (128, S = 2), 3.1e-4 / 2.3e-4 (non-up 64 / 256, S = 4);
                    impl 1: 3.6e-4; rms 2.4e-5 of max|ref|
  conv2 form        impl 5: 3.7e-4 (<16>), 2.9e-4 (<32>); impl 4 and impl 2 (64 x 288): 2.6e-4 both; impl 6: 3.3e-4
  conv3 form        2.4e-4 (res_cs 128, up), 3.7e-4 (res_cs 64), 4.3e-4 (res_cs 128): impl 2, 6 and 1 return the same values
  final form        impl 2 + tanh: 1.2e-3 (8 x 32), 1.6e-3 (24 x 64) absolute on (-1, 1) — all of it the declared roundings: d = 1.2e-3 / 1.6e-3, the device
                    lies 7e-7 from the rounded model (worst err / tol 0.95 / 0.97); two passes: map 4.0e-4, bg_rgb_tanh 7.0e-8 absolute
  softmax           max err 6.8e-5 .. 2.3e-4 absolute (the fp16 store; float32 restatement 2e-8 .. 2e-7), worst err / tol 0.62 .. 0.88
  cond              1.0e-7 .. 1.3e-7 absolute, float32 restatement 9.5e-8 .. 1.3e-7 (worst err / tol 0.31)
  bn tables         4.0e-6 (C = 96), 2.6e-6 (C = 1000) absolute, float32 restatement 2.9e-6 / 4.2e-6; tab16 bit-equal
  rgb_tanh          7.2e-8 absolute, float32 restatement 6.0e-8
  attn_split, to_half (n = 1 .. 4098, overflow, subnormals, halfway cases): bit-exact
  batched gemm      mode 3: 1.1e-7; mode 0: 3.7e-4 / 3.9e-4; K = 32 on gemm_direct: 8e-8; cand_batch 0 / 1 bit-identical (also where it switches
                    gemm_tiled_kernel<64> / <128>)
  tail              (1, 32): max 9.0e-4, border max 8.3e-4 rms 1.9e-4, interior max 9.0e-4 rms 2.1e-4; (3, 64): max 1.2e-3, border 8.4e-4 / 1.7e-4,
                    interior 1.2e-3 / 2.0e-4; (9, 128): max 1.3e-3, border 7.9e-4 / 1.7e-4, interior 1.3e-3 / 1.7e-4 (absolute, images in (-1, 1))
  chain             3.8e-4 (rms 4.2e-5) of max|ref| = 5.7
"""
import math
import os

import numpy as np
import pytest
import torch

import biggan_ops_ref as R
from clip_glass_amd import synth
from oracle import biggan_ref
from util import check, diag, nchw

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
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def weff(w):
    """The weights as the op uploads them (glass_pack_conv): h16(w * coef), coef = 1 / sqrtf(Cin KS KS) in float32."""
    coef = np.float32(1.0) / np.sqrt(np.float32(w.shape[1] * w.shape[2] * w.shape[3]))
    return h16(w.astype(np.float32) * coef).astype(np.float64)


def _rng(seed):
    return np.random.default_rng(seed)


def _tables(rng, B, C):
    """Per-(candidate, channel) scale and shift: O(1) apart between candidates and channels, both signs; the shift has a positive mean."""
    A = (rng.standard_normal((B, C)) + 0.8 * rng.choice([-1.0, 1.0], (B, 1))).astype(np.float32)
    S = (0.6 + 0.8 * rng.standard_normal((B, C))).astype(np.float32)
    return A, S


def _xw(rng, B, H, W, Cin, Cout, ks):
    return h16(rng.standard_normal((B, H, W, Cin))), rng.standard_normal((Cout, Cin, ks, ks)).astype(np.float32)


def check_staged(name, got, ref_exact, ref_rounded):
    """The derived bar of the module docstring for the forms that stage through fp16 tables."""
    got, ref_exact = np.asarray(got, np.float64), np.asarray(ref_exact, np.float64)
    d = float(np.abs(ref_rounded - ref_exact).max())
    scale = float(np.abs(ref_exact).max())
    tol = d + 2.0 ** -11 * np.abs(ref_exact) + 2.0 ** -16 * scale
    err = np.abs(got - ref_exact)
    diag("[bg-ops] %-40s derived bar: d(rounded, exact) %.3e  max err %.3e  vs rounded model %.3e  max|ref| %.3e  worst err / tol %.3f"
         % (name, d, err.max(), np.abs(got - ref_rounded).max(), scale, (err / tol).max()))
    assert (err <= tol).all(), "%s: %d elements beyond the derived bar (max err %.3e, d %.3e)" % (name, int((err > tol).sum()), err.max(), d)


# ---- conv0 form: 1x1, bn + relu of the input while staging, bn + relu in the epilogue -------------------------------------------------
@pytest.mark.parametrize("impl,B,H,W,Cin,Cout", [(2, 3, 8, 32, 128, 32), (2, 2, 24, 64, 128, 32), (6, 3, 4, 4, 256, 64), (1, 3, 8, 8, 128, 32)])
def test_conv0_form(impl, B, H, W, Cin, Cout):
    rng = _rng(100 + impl + H)
    x, w = _xw(rng, B, H, W, Cin, Cout, 1)
    A, S = _tables(rng, B, Cin)
    ds, sh = _tables(rng, B, Cout)
    got = ops.conv(x, w, impl=impl, sn=A, pre_shift=S, dscale=ds, shift=sh, act=2)
    kw = dict(pre=(A, S), dscale=ds, shift=sh, relu=True)
    ref = R.conv(x, weff(w), **kw)
    name = "conv0 impl%d B%d %dx%d %d->%d" % (impl, B, H, W, Cin, Cout)
    check(name, got, ref, 5e-3)
    if impl == 2:
        check_staged(name, got, ref, R.conv(x, weff(w), pre_rounding="f16", **kw))


# ---- conv1 form: 3x3 reading its input through a nearest x2 upsample, bn + relu in the epilogue ---------------------------------------
@pytest.mark.parametrize("impl,B,h,w_,C,up", [(2, 3, 12, 32, 32, True), (2, 3, 12, 32, 64, True),
                                              (6, 3, 4, 4, 64, True), (1, 3, 4, 4, 64, True),        # 9 * 64 = 576: no K split (see the docstring)
                                              (6, 3, 4, 4, 128, True),                                # im2col, S = 2
                                              (6, 3, 4, 4, 64, False),                                # the non-up 4 x 4 case (gather)
                                              (6, 3, 4, 4, 256, False)])                              # gather, S = 4
def test_conv1_form(impl, B, h, w_, C, up):
    rng = _rng(200 + impl + C)
    x, w = _xw(rng, B, h, w_, C, C, 3)
    ds, sh = _tables(rng, B, C)
    got = ops.conv(x, w, impl=impl, in_up=up, dscale=ds, shift=sh, act=2)
    assert got.shape == (B, h << up, w_ << up, C)
    check("conv1 impl%d B%d %dx%d up%d %d->%d" % (impl, B, h, w_, up, C, C), got, R.conv(x, weff(w), in_up=up, dscale=ds, shift=sh, relu=True), 5e-3)


# ---- conv2 form: 3x3, bn + relu in the epilogue ---------------------------------------------------------------------------------------
def _stream_shape():
    """The smallest map choose_conv_stream accepts: 64 nominal candidates x (W / 32) (H / 8) tiles >= 6 per slot, 3 slots per CU."""
    from clip_glass_amd.engine import device_info
    need = -(-device_info(0)["cus"] * 3 * 6 // 64)
    return 64, 32 * -(-need // 8)


@pytest.mark.parametrize("impl,B,H,W,C", [(5, 3, 16, 16, 128), (5, 3, 16, 32, 128), (4, 2, 0, 0, 32), (2, 2, 0, 0, 32), (6, 3, 8, 8, 64)])
def test_conv2_form(impl, B, H, W, C):
    if H == 0:
        H, W = _stream_shape()
    rng = _rng(300 + C)
    x, w = _xw(rng, B, H, W, C, C, 3)
    ds, sh = _tables(rng, B, C)
    got = ops.conv(x, w, impl=impl, dscale=ds, shift=sh, act=2)
    check("conv2 impl%d B%d %dx%d %d->%d" % (impl, B, H, W, C, C), got, R.conv(x, weff(w), dscale=ds, shift=sh, relu=True), 5e-3)


# ---- conv3 form: 1x1 + bias, no activation, the skip as a strided / upsampled residual read ---------------------------------------------
@pytest.mark.parametrize("impl", [2, 6, 1])
@pytest.mark.parametrize("res_mult,res_up", [(2, True), (1, False), (2, False)])
def test_conv3_form(impl, res_mult, res_up):
    B, H, W, Cin, Cout = 3, 8, 32, 64, 64
    rng = _rng(400 + res_mult + res_up)
    x, w = _xw(rng, B, H, W, Cin, Cout, 1)
    bias = rng.standard_normal(Cout).astype(np.float32)
    rcs = res_mult * Cout
    res = h16(rng.standard_normal((B, H >> res_up, W >> res_up, rcs)) + np.arange(B)[:, None, None, None])     # O(1) apart per candidate
    got = ops.conv(x, w, impl=impl, bias=bias, res=res, res_cs=rcs if res_mult > 1 else 0, res_up=res_up)
    check("conv3 impl%d res_cs %d up%d" % (impl, rcs, res_up), got, R.conv(x, weff(w), bias=bias, res=res, res_up=res_up), 5e-3)


# ---- final form: bn + relu while staging, 3x3 128 -> 32 (3 used), tanh from the accumulators --------------------------------------------
def _final_case(seed, B, H, W):
    rng = _rng(seed)
    x, w = _xw(rng, B, H, W, 128, 32, 3)
    A, S = _tables(rng, B, 128)
    bias = (0.2 * rng.standard_normal(32)).astype(np.float32)
    return x, w, A, S, bias


@pytest.mark.parametrize("B,H,W", [(3, 8, 32), (2, 24, 64)])
def test_final_form_fused_tanh(B, H, W):
    x, w, A, S, bias = _final_case(500 + H, B, H, W)
    got = ops.conv(x, w, impl=2, sn=A, pre_shift=S, bias=bias, rgb_tanh=True)
    assert got.shape == (B, 3, H, W)
    f = lambda rounding: np.tanh(R.conv(x, weff(w)[:3], pre=(A, S), bias=bias[:3], pre_rounding=rounding)).transpose(0, 3, 1, 2)
    ref = f(None)
    check("final impl2 B%d %dx%d rgb_tanh" % (B, H, W), got, ref, 5e-3)
    check_staged("final impl2 B%d %dx%d rgb_tanh" % (B, H, W), got, ref, f("f16"))


def test_final_form_two_pass_fallback():
    """A map conv_tiled does not take (16 x 16): the conv on conv_direct storing the 32-channel map, then bg_rgb_tanh_kernel — the engine's
    fallback in glass_biggan_chunk."""
    B, H, W = 3, 16, 16
    x, w, A, S, bias = _final_case(516, B, H, W)
    y = ops.conv(x, w, impl=1, sn=A, pre_shift=S, bias=bias)
    ref = R.conv(x, weff(w), pre=(A, S), bias=bias)
    check("final impl1 16x16 map", y, ref, 5e-3)
    y = y.reshape(B, H * W, 32)                                # the second pass is checked on the map the first one stored
    _f32_bar("final impl1 16x16 + bg_rgb_tanh", ops.bg_rgb_tanh(y), R.rgb_tanh(y), np.tanh(y[..., :3]).transpose(0, 2, 1))


@pytest.mark.parametrize("impl", [1, 5, 6])
def test_rgb_tanh_is_refused_off_conv_tiled(impl):
    x, w, A, S, bias = _final_case(500, 2, 16, 32)
    with pytest.raises(RuntimeError, match="rgb_tanh: conv_tiled only"):
        ops.conv(x, w, impl=impl, sn=A, pre_shift=S, bias=bias, rgb_tanh=True)


# ---- small kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C,kernel", [(16, 16, 256, "bg_attn_split_vec_kernel"), (8, 16, 512, "bg_attn_split_vec_kernel"),
                                          (16, 16, 384, "bg_attn_split_vec_kernel"), (4, 4, 64, "bg_attn_split_kernel"),
                                          (8, 8, 128, "bg_attn_split_kernel"), (16, 16, 192, "bg_attn_split_kernel")])
def test_attn_split_bit_exact(H, W, C, kernel):
    B, c8, c2 = 3, C // 8, C // 2
    T = h16(_rng(600 + C).standard_normal((B, H, W, 2 * c8 + c2)))
    theta, phi, gT, ran = ops.bg_attn_split(T, c8, c2)
    assert ran == kernel
    rt, rp, rg = R.attn_split(T, c8, c2)
    np.testing.assert_array_equal(theta, rt)
    np.testing.assert_array_equal(phi, rp)
    np.testing.assert_array_equal(gT, rg)


def _f32_bar(name, got, ref64, ref32, store16=False):
    """|got - ref64| <= 4 max|ref32 - ref64| (+ 2^-11 |ref64| for an fp16 store)."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    e32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    err = np.abs(got - ref64)
    tol = 4 * e32 + (2.0 ** -11 * np.abs(ref64) if store16 else 0.0)
    diag("[bg-ops] %-40s max err %.3e  float32 restatement's %.3e  worst err / tol %.3f" % (name, err.max(), e32, (err / tol).max()))
    assert np.isfinite(got).all() and (err <= tol).all(), "%s: max err %.3e, float32 restatement %.3e" % (name, err.max(), e32)


def _softmax32(s):
    s = s.astype(np.float32)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e * (np.float32(1) / e.sum(axis=1, keepdims=True, dtype=np.float32))


@pytest.mark.parametrize("rows", [5, 8])
@pytest.mark.parametrize("n", [1024, 256, 64, 100])
def test_softmax(n, rows):
    rng = _rng(700 + n)
    S = (4.0 * rng.standard_normal((rows, n))).astype(np.float32)
    S[0] = 80.0 * rng.choice([-1.0, 1.0], n)          # +-80 logits
    S[1] = 3.25                                         # constant row
    S[2, n // 3] += 40.0                                # one dominant entry
    got = ops.bg_softmax(S)
    ref = R.softmax(S)
    _f32_bar("softmax n%d rows%d" % (n, rows), got, ref, _softmax32(S), store16=True)
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= n * 2.0 ** -12


def _cond32(x, et, zd):
    """bg_cond_kernel in float32 numpy: exp(bits - max), the class sum one term after the other, times 1 / sum."""
    x, et = x.astype(np.float32), et.astype(np.float32)
    bits = x[:, zd:zd + et.shape[0]]
    e = np.exp(bits - bits.max(axis=1, keepdims=True))
    acc = np.zeros((x.shape[0], zd), np.float32)
    for k in range(et.shape[0]):
        acc += e[:, k:k + 1] * et[k]
    return np.concatenate([np.clip(x[:, :zd], -2, 2), acc * (np.float32(1) / e.sum(axis=1, keepdims=True, dtype=np.float32))], axis=1)


@pytest.mark.parametrize("zd,nc", [(128, 1000), (16, 24), (128, 300)])
def test_cond(zd, nc):
    P = 3
    x = synth.biggan_population(800 + nc, P, zd, nc).astype(np.float32)
    x[0, :zd] *= 3.0                                     # z beyond +-2
    x[1, zd:] = np.linspace(-50.0, 50.0, nc)             # class bits up to +-50
    x[2, zd:] += _rng(nc).standard_normal(nc).astype(np.float32)
    emb = _rng(801 + nc).standard_normal((zd, nc)).astype(np.float32)
    et = np.ascontiguousarray(emb.T)
    got = ops.bg_cond(x, et, zd)
    np.testing.assert_array_equal(got[:, :zd], np.clip(x[:, :zd], -2, 2))
    _f32_bar("cond zd%d nc%d" % (zd, nc), got, R.cond(x, emb, zd), _cond32(x, et, zd))


def _tables32(cnd, wt, bias, inv_std, mean, prebias):
    lin = np.tile(bias.astype(np.float32), (cnd.shape[0], 1))
    for k in range(cnd.shape[1]):
        lin += cnd[:, k:k + 1].astype(np.float32) * wt[k].astype(np.float32)
    C = inv_std.shape[0]
    A = lin[:, :C] * inv_std
    return np.concatenate([A, lin[:, C:] + (prebias - mean) * A], axis=1)


@pytest.mark.parametrize("C", [96, 1000])
def test_bn_tables(C):
    P, cd = 3, 256
    rng = _rng(900 + C)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    cnd, wt = f(P, cd), f(cd, 2 * C) / np.float32(math.sqrt(cd))
    bias = np.concatenate([np.ones(C, np.float32), np.zeros(C, np.float32)])
    inv_std, mean, prebias = rng.uniform(0.5, 2.0, C).astype(np.float32), 0.3 * f(C), 0.5 * f(C)
    tab, tab16 = ops.bg_bn_tables(cnd, wt, bias, inv_std, mean, prebias)
    _f32_bar("bn tables C%d" % C, tab, R.bn_tables(cnd, wt, bias, inv_std, mean, prebias), _tables32(cnd, wt, bias, inv_std, mean, prebias))
    np.testing.assert_array_equal(tab16.astype(np.float16).view(np.uint16), tab.astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("n", [1, 3, 4, 7, 1023, 4096 + 2])
def test_to_half_bit_exact(n):
    """Any n: launch_bg_to_half converts the n % 4 tail one element at a time (csrc/kernels.h)."""
    special = np.array([65504.0, 65519.99, 65520.0, 70000.0, -65520.0, 1e30, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -25 * 1.0001,
                        -2.0 ** -26, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 * 1.0001,
                        0.0, -0.0, 0.1, -1.0 / 3], dtype=np.float32)
    x = (_rng(n).standard_normal(n) * 10.0 ** _rng(n + 1).uniform(-9, 5, n)).astype(np.float32)
    k = min(n, special.size)
    x[n - k:] = special[:k]                               # the special values sit in the tail elements too
    got = ops.bg_to_half(x)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    np.testing.assert_array_equal(got.astype(np.float16).view(np.uint16), want.view(np.uint16))


def test_rgb_tanh():
    B, hw, C = 3, 300, 32
    x = h16(1.5 * _rng(1000).standard_normal((B, hw, C)))
    _f32_bar("rgb_tanh", ops.bg_rgb_tanh(x), R.rgb_tanh(x), np.tanh(x[..., :3].astype(np.float32)).transpose(0, 2, 1))


# ---- batched gemm ---------------------------------------------------------------------------------------------------------------------------
def _gemm_case(M, N, K, batch=3):
    rng = _rng(1100 + M + N + K)
    a = h16(rng.standard_normal((batch, M, K)) + np.arange(batch)[:, None, None] - 1.0)      # O(1) apart per batch slice
    w = h16(rng.standard_normal((batch, N, K)) * K ** -0.5 * (1.0 + np.arange(batch)[:, None, None]))
    return a, w, np.einsum("bmk,bnk->bmn", a.astype(np.float64), w.astype(np.float64))


@pytest.mark.parametrize("M,N,K,mode", [(256, 64, 64, 3), (192, 64, 64, 3), (256, 128, 64, 0), (512, 128, 64, 0), (256, 64, 32, 3)])
def test_gemm_batched(M, N, K, mode):
    """The self-attention products.  (512, 128, 64): 4 x 64 nominal candidates fill the chip with 128-wide tiles, 4 x 3 problems do not —
    cand_batch switches the instance there, and the launcher's comment says the instances are bit-identical per output element."""
    a, w, ref = _gemm_case(M, N, K)
    got = ops.gemm_batched(a, w, mode=mode, cand_batch=True)
    check("gemm batched %dx%dx%d mode%d" % (M, N, K, mode), got, ref, 3e-3 if mode == 3 else 4e-3)
    np.testing.assert_array_equal(got, ops.gemm_batched(a, w, mode=mode, cand_batch=False))
    if K % 64 == 0:
        np.testing.assert_array_equal(got, ops.gemm_batched(a, w, mode=mode, impl=2))           # impl 0 took gemm_tiled
    else:
        np.testing.assert_array_equal(got, ops.gemm_batched(a, w, mode=mode, impl=1))           # gemm_tiled refuses K = 32: gemm_direct
        with pytest.raises(RuntimeError, match="tiled gemm: unsupported shape"):
            ops.gemm_batched(a, w, mode=mode, impl=2)


# ---- the fused last stage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R_", [(1, 32), (3, 64), (9, 128)])
def test_tail(B, R_):
    rng = _rng(1200 + R_)
    h = h16(np.maximum(rng.standard_normal((B, R_, R_, 32)), 0.0))                               # relu(bn_3(conv_2))
    x0 = h16(rng.standard_normal((B, R_ // 2, R_ // 2, 128)) + 0.5 * (np.arange(B)[:, None, None, None] % 3 - 1))
    w3 = h16(rng.standard_normal((128, 32)) / (math.sqrt(128) + math.sqrt(32)))
    b3 = (0.2 * rng.standard_normal(128)).astype(np.float32)
    A = (rng.uniform(0.5, 1.5, 128) * rng.choice([-1.0, 1.0], 128)).astype(np.float32)
    S = (0.3 + 0.5 * rng.standard_normal(128)).astype(np.float32)
    rgb_w = h16(rng.standard_normal((3, 128, 3, 3)) / (math.sqrt(128 * 9) + math.sqrt(128)))
    rgb_b = (0.1 * rng.standard_normal(3)).astype(np.float32)
    got = ops.bg_tail(h, x0, w3, b3, A, S, rgb_w, rgb_b)
    ref = R.tail(h, x0, w3, b3, A, S, rgb_w, rgb_b)
    err = np.abs(got.astype(np.float64) - ref)
    border = np.zeros((R_, R_), bool)
    border[[0, -1], :] = True
    border[:, [0, -1]] = True
    eb, ei = err[:, :, border], err[:, :, ~border]
    rms = lambda e: float(np.sqrt((e ** 2).mean()))
    diag("[bg-ops] tail B%d R%d: max err %.3e  border max %.3e rms %.3e  interior max %.3e rms %.3e  max|ref| %.3f"
         % (B, R_, err.max(), eb.max(), rms(eb), ei.max(), rms(ei), np.abs(ref).max()))
    assert np.isfinite(got).all() and err.max() <= 4e-3, "max err %.3e" % err.max()
    assert eb.max() <= ei.max() + rms(ei), "border-only excess: border max %.3e, interior max %.3e" % (eb.max(), ei.max())


# ---- one self-attention block composed from the ops --------------------------------------------------------------------------------------
def test_self_attention_chain():
    """theta | phi | g conv -> split -> logits -> softmax -> values -> o_conv + residual at C = 512, 32 x 32: 256 pooled positions, the
    geometry that reaches bg_softmax_reg_kernel<1>, against biggan_ref.self_attn in float64."""
    B, C, H = 2, 512, 32
    c8, c2 = C // 8, C // 2
    p = "a"
    sd = synth.make_biggan_state([(p + ".snconv1x1_theta.weight_orig", (c8, C, 1, 1), "sn"), (p + ".snconv1x1_phi.weight_orig", (c8, C, 1, 1), "sn"),
                                  (p + ".snconv1x1_g.weight_orig", (c2, C, 1, 1), "sn"), (p + ".snconv1x1_o_conv.weight_orig", (C, c2, 1, 1), "sn"),
                                  (p + ".gamma", (1,), ("gamma", 0.0))], 7)
    sd = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in sd.items()}
    x = h16(_rng(1300).standard_normal((B, H, H, C)))
    with torch.no_grad():
        ref = biggan_ref.self_attn(sd, p, torch.from_numpy(nchw(x).astype(np.float64))).numpy()
        wn = {k: biggan_ref.sn_weight(sd, p + ".snconv1x1_" + k).numpy() for k in ("theta", "phi", "g", "o_conv")}
    unscale = lambda w: (w * math.sqrt(w.shape[1])).astype(np.float32)                            # the op applies 1 / sqrt(Cin) itself
    T = ops.conv(x, unscale(np.concatenate([wn["theta"], wn["phi"], wn["g"]])), impl=2)
    theta, phi, gT, ran = ops.bg_attn_split(T, c8, c2)
    assert ran == "bg_attn_split_vec_kernel"
    logits = ops.gemm_batched(theta, phi, mode=3)
    P = ops.bg_softmax(logits.reshape(B * H * H, H * H // 4))
    O = ops.gemm_batched(P.reshape(B, H * H, H * H // 4), gT, mode=0)
    y = ops.conv(O.reshape(B, H, H, c2), unscale(wn["o_conv"] * float(sd[p + ".gamma"][0])), res=x, impl=2)
    check("self-attention chain C512 32x32", nchw(y), ref, 1e-2)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_biggan_ops_refuse_unsupported_forms_by_name():
    rng = _rng(1400)
    x, w = _xw(rng, 2, 16, 32, 128, 128, 3)
    A, S = _tables(rng, 2, 128)
    with pytest.raises(RuntimeError, match="pre_shift needs sn"):
        ops.conv(x, w, impl=2, pre_shift=S)
    with pytest.raises(RuntimeError, match="in_up: H and W are the upsampled dims"):
        d = ops.ConvDesc()                                 # (the wrapper derives H = 2 h: an odd H only exists at the ABI)
        xs, ws, ys = ops._f32(x[:, :3]), ops._f32(w), np.empty((2, 7, 64, 128), np.float32)
        d.B, d.H, d.W, d.Cin, d.Cout, d.KS, d.stride, d.pad, d.Ho, d.Wo, d.in_up, d.impl = 2, 7, 64, 128, 128, 3, 1, 1, 7, 64, 1, 2
        d.out_scale, d.batch_size = 1.0, 1
        d.x, d.w, d.y = ops._fp(xs), ops._fp(ws), ops._fp(ys)
        lib = ops._lib()
        ops._check(lib, lib.glass_op_conv(0, ops.C.byref(d)))
    ops.conv(x, w, impl=5)                                  # conv_glds takes the plain layer ...
    with pytest.raises(RuntimeError, match="LDS-DMA conv: unsupported shape"):
        ops.conv(x[:, :8, :16], w, impl=5, in_up=True)      # ... and refuses the same map read through the upsample
    with pytest.raises(RuntimeError, match="LDS-DMA conv: unsupported shape"):
        ops.conv(x, w, impl=5, sn=A, pre_shift=S)
    H, W = _stream_shape()
    xs, ws = _xw(rng, 1, H, W, 32, 32, 3)
    with pytest.raises(RuntimeError, match="streaming conv: unsupported shape"):
        ops.conv(xs, ws, impl=4, res=np.zeros((1, H, W, 32), np.float32))
    t = lambda R_, mid: ops.bg_tail(np.zeros((1, R_, R_, mid), np.float32), np.zeros((1, R_ // 2, R_ // 2, 128), np.float32),
                                    np.zeros((128, mid), np.float32), np.zeros(128, np.float32), np.ones(128, np.float32), np.zeros(128, np.float32),
                                    np.zeros((3, 128, 3, 3), np.float32), np.zeros(3, np.float32))
    with pytest.raises(RuntimeError, match="bg_tail: unsupported shape"):
        t(16, 32)
    with pytest.raises(RuntimeError, match="bg_tail: unsupported shape"):
        t(32, 64)
