"""float64 references of the stride-1 3x3 / 1x1 convolution kernels behind glass_op_conv, an error bound PER ELEMENT, an fp32 emulation of a
faithful kernel and the inputs the CPU and the GPU tests share (TEST INFRASTRUCTURE; tests/test_conv_ops_ref.py, tests/test_gpu_conv_ops.py).

Every reference returns (ref, tol), arrays of the output's shape.  Nothing here is measured on the device.

OPERANDS ARE MIRRORED EXACTLY.  The roundings that make the MFMA's fp16 operands are deterministic, so the reference applies them itself and
bounds only what comes after.  Weights: fp16(fp32(w) * coef) — ops.host_pack_conv, the library's own glass_pack_conv.  The style reaches the
product in one of three forms, from the fp32 table `sn` or its fp16 copy `sn16`:

  family (KERNELS key)   form     table   where the staging code does it
  conv_direct            x        sn      conv_direct.hip:88-93    a[j] = (half_t)((float)a[j] * f.s0[j])           fp32 product, then fp16
  conv_gemm              x        sn      conv_gemm.hip:38-41      a[j] = (half_t)((float)a[j] * s[j])              (im2col; "conv_direct's rounding")
  conv_tiled             x        sn16    conv_tiled.hip:128,143,175   *(h8*)a_lds(k) = (... ra[k] ...) * sh        packed fp16 product: one rounding
  conv_stream            x        sn16    conv_stream.hip:201,275-285  *(h8*)(As + ...) = a * sh                    packed fp16 product
  conv_glds / conv_gldsp w        sn16    conv_glds.hip:145,182-185 / 424,561   wf[j] = wf[j] * sv                  packed fp16 product on the weight fragments
  conv_wreg              (none)           conv_wreg.hip:455 WREG_FEATURES has no CF_STYLE: the kernel takes per-sample weights instead
  premod (any family)    premod   sn      kernels_misc.hip:277     r[j] = (half_t)((float)v[j] * s[j] * d)          two fp32 products, then fp16; the
                                                                                                                    conv then runs without sn / dscale
A product of two fp16 values is exact in fp32, so fp16(fp32(a) * fp32(b)) mirrors a packed fp16 product with ONE rounding; the fp32-table forms
are mirrored as the fp32 product rounded to fp16 (two roundings, as the device makes them).

EVERYTHING AFTER THE OPERANDS IS EXACT float64.  With a_k, b_k the mirrored fp16 operands, K = KS^2 Cin products per output element:
  acc = sum a_k b_k,  A = sum |a_k b_k|
  pre = acc d + sigma noise + bias,  P = A |d| + |sigma noise| + |bias|
  out = (act(pre) + res) out_scale,  g = sqrt 2 where act is on, 1 otherwise
and the bound per element is

  tol = out_scale g (2 K + 8) U32 P  +  4 U32 (|res| out_scale + |out|)  +  sum_j U16 |v_j|  +  2^-24

  (2 K + 8) U32 P   the order-free summation bound |fl(sum) - sum| <= K u sum|terms| plus the epilogue's fp32 operations (at most eight: d, sigma,
                    two or three additions, slope, gain, scale), carried through the activation by its largest slope g and the output scale.  The
                    factor 2 on K is a margin for the MFMA's internal accumulation (how v_mfma_f32_32x32x16_f16 rounds between its 16 products
                    is not specified and NOBODY HERE HAS MEASURED IT); the split-K forms (conv_direct's four waves, conv_gemm's up to four slices)
                    add three fp32 additions, inside the same margin.
  4 U32 (...)       the residual's product with out_scale, its addition and the final scale.
  v_j               the values at which the kernel rounds to fp16 between the accumulator and the store (EPILOGUES below):
     fp32 epilogues (conv_direct.hip:149-165, conv_gemm.hip:81-91, conv_tiled.hip:410-423 and 480-521, conv_glds.hip:268-272 / 657-661,
                    conv_wreg.hip:393-396): ONE, the store itself: v = out.
     conv_stream    (conv_stream.hip:345-346, 403-404) THREE: the activation input v = (half_t)(acc d + (nz + bb)) [|pre|, carried to the output by
                    g out_scale]; the constant k1 = (half_t)(sqrt2 out_scale) resp. k2 [relative U16 of the output: |out|]; the packed product
                    v * k [|out|]; the max of the two products is exact.  The kernel has no residual.
  2^-24             half the smallest fp16 subnormal: the rounding unit of outputs below 2^-14.

FUSED toRGB FORMS keep the structure of the suite's existing tests: the kernel's own stored fp16 map goes through the float64 toRGB
(util._torgb_ref), bound glue_ops_ref.tol_torgb plus TRGB_SPLIT = 4 roundings: the kernels hold the modulated toRGB weight as an fp16 pair
hi + lo / 2048 (kernels_misc.hip trgb_table_value; conv_stream.hip:213-217), whose lo half is rounded to fp16: 2^-11 2^-11 |w| = 4 U32 |w|.  The
partial-sum form (trgb_finish_kernel, kernels_misc.hip:507-508) adds TRGB_PARTIAL = 4 more: one fp32 addition per n tile (two tiles at Cout = 256)
and the two roundings of each partial's own closing additions.

No term is fitted to an observed error."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from glue_ops_ref import U16, U32, h16, tol_torgb, torgb
from util import style_tables

SQRT2 = math.sqrt(2.0)
SUBNORMAL = 2.0 ** -24
TRGB_SPLIT, TRGB_PARTIAL = 4, 4

# family -> (form, table, epilogue); form / table as the docstring's table, epilogue "fp32" or "stream"
KERNELS = {
    "conv_direct": ("x", "sn", "fp32"),
    "conv_gemm": ("x", "sn", "fp32"),
    "conv_tiled": ("x", "sn16", "fp32"),
    "conv_stream": ("x", "sn16", "stream"),
    "conv_glds": ("w", "sn16", "fp32"),
    "conv_wreg": ("premod", "sn", "fp32"),      # (its only styled form: per-sample weights from modulate_weights_kernel)
}


def _pack(w):
    """[T = KS^2][Cout][Cin] float32 holding fp16 values: fp16(fp32(w) * 1 / sqrt(Cin KS^2)), the library's own host code."""
    from clip_glass_amd import ops
    return ops.host_pack_conv(np.asarray(w, np.float32))


def operands(inp, form, table):
    """The fp16 operands of the MFMAs as float32 arrays: a [B,H,W,Cin] and b [B or 1][T][Cout][Cin] — and whether dscale still applies."""
    x, sn, B = inp["x"], inp.get("sn"), inp["B"]
    wp = _pack(inp["w"])
    a = np.broadcast_to(x, (B,) + x.shape[1:]) if x.shape[0] != B else x
    b = wp[None]
    demod = inp.get("dscale") is not None
    if sn is None:
        return np.ascontiguousarray(a, np.float32), b, demod
    s = np.asarray(sn, np.float32)
    if table == "sn16":
        s = h16(s)
    if form == "x":         # fp32 product (exact for the fp16 table), one conversion to fp16
        a = h16(a.astype(np.float32) * s[:, None, None, :])
    elif form == "w":
        b = h16(wp[None] * s[:, None, None, :])
    elif form == "premod":  # (w16 * s) * d in fp32, then fp16; the conv runs without dscale
        d = np.asarray(inp["dscale"], np.float32) if demod else np.ones((B, wp.shape[1]), np.float32)
        b = h16((wp[None] * s[:, None, None, :]).astype(np.float32) * d[:, None, :, None])
        demod = False
    else:
        raise ValueError(form)
    return np.ascontiguousarray(a, np.float32), b, demod


def _conv(a, b, KS, stride, pad, dtype):
    """sum_k a_k b_k for NHWC a [B,H,W,Cin] and b [B or 1][T][Cout][Cin] -> [B,Ho,Wo,Cout] in `dtype` (torch CPU; per-sample weights as groups)."""
    B, H, W, Cin = a.shape
    Cout = b.shape[2]
    at = torch.as_tensor(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).to(dtype)
    wt = torch.as_tensor(np.ascontiguousarray(b.reshape(b.shape[0], KS, KS, Cout, Cin).transpose(0, 3, 4, 1, 2))).to(dtype)      # [Bw,Cout,Cin,KS,KS]
    if b.shape[0] == 1:
        y = F.conv2d(at, wt[0], stride=stride, padding=pad)
    else:
        y = F.conv2d(at.reshape(1, B * Cin, H, W), wt.reshape(B * Cout, Cin, KS, KS), stride=stride, padding=pad, groups=B)
        y = y.reshape(B, Cout, y.shape[2], y.shape[3])
    return np.ascontiguousarray(y.numpy().transpose(0, 2, 3, 1))


def _planes(inp, Ho, Wo):
    """sigma * noise per SAMPLE [B,Ho,Wo,1] (float64; zeros without noise)."""
    if inp.get("noise") is None:
        return np.zeros((inp["B"], Ho, Wo, 1))
    nz = np.repeat(np.asarray(inp["noise"], np.float64), inp.get("batch_size", 1), axis=0)
    return (float(np.float32(inp.get("noise_strength", 0.0))) * nz)[..., None]


def conv_ref(inp, family):
    """(ref, tol) of one launch under `family`'s operand form and epilogue roundings; ref and tol [B,Ho,Wo,Cout] float64."""
    form, table, epi = KERNELS[family]
    a, b, demod = operands(inp, form, table)
    KS, stride, pad = inp["w"].shape[2], inp.get("stride", 1), inp.get("pad", inp["w"].shape[2] // 2)
    acc = _conv(a, b, KS, stride, pad, torch.float64)
    B, Ho, Wo, Cout = acc.shape
    K = KS * KS * a.shape[3]
    # (A only scales the bound: summed in float32 and raised by that sum's own worst-case error, it stays an upper bound of sum |a_k b_k|)
    A = _conv(np.abs(a), np.abs(b), KS, stride, pad, torch.float32).astype(np.float64) * (1 + 2 * K * U32)
    d = np.asarray(inp["dscale"], np.float64)[:, None, None, :] if demod else 1.0
    nz = _planes(inp, Ho, Wo)
    bias = np.asarray(inp["bias"], np.float64) if inp.get("bias") is not None else np.zeros(Cout)
    pre = acc * d + nz + bias
    P = A * np.abs(d) + np.abs(nz) + np.abs(bias)
    act = bool(inp.get("act"))
    g = SQRT2 if act else 1.0
    os_ = float(np.float32(inp.get("out_scale", 1.0)))
    res = np.asarray(inp["res"], np.float64) if inp.get("res") is not None else 0.0
    post = np.where(pre > 0, pre, 0.2 * pre) * SQRT2 if act else pre
    out = (post + res) * os_
    tol = os_ * g * (2 * K + 8) * U32 * P + 4 * U32 * (np.abs(res) * os_ + np.abs(out)) + SUBNORMAL
    if epi == "fp32":
        tol = tol + U16 * np.abs(out)
    else:                   # conv_stream: fp16(pre), fp16(k), fp16(v * k)
        tol = tol + U16 * (g * os_ * np.abs(pre) + 2 * np.abs(out))
    return out, tol


def torgb_ref(feat, t, C, partial=False):
    """(ref, tol) of a fused toRGB from the kernel's own stored fp16 map `feat` [B,H,W,C]; t = dict(w, b, sn, smax, yprev)."""
    ref, A = torgb(feat, t["w"], t["b"], t["sn"], t["smax"], t.get("yprev"))
    return ref, tol_torgb(C + TRGB_SPLIT + (TRGB_PARTIAL if partial else 0), A)


# ---- the fp32 emulation of a faithful kernel --------------------------------------------------------------------------------------------------
class Emulation:
    """float32 accumulators of the mirrored operands (torch float32 conv) and the epilogue in float32 — or, for conv_stream, in packed fp16 —
    ending in the fp16 store.  finish() takes the pieces a planted defect replaces."""

    def __init__(self, inp, family):
        self.inp, self.family = inp, family
        self.form, self.table, self.epi = KERNELS[family]
        self.a, self.b, self.demod = operands(inp, self.form, self.table)
        self.KS, self.stride = inp["w"].shape[2], inp.get("stride", 1)
        self.pad = inp.get("pad", self.KS // 2)
        self.acc = self.accumulate(self.a, self.b)

    def accumulate(self, a, b):
        return _conv(a, b, self.KS, self.stride, self.pad, torch.float32)

    def finish(self, acc=None, noise_planes=None, res_before_act=False):
        inp = self.inp
        f32 = np.float32
        v = (self.acc if acc is None else acc).astype(f32)
        B, Ho, Wo, Cout = v.shape
        if self.demod:
            v = v * np.asarray(inp["dscale"], f32)[:, None, None, :]
        nz = (_planes(inp, Ho, Wo) if noise_planes is None else noise_planes).astype(f32)
        bias = np.asarray(inp["bias"], f32) if inp.get("bias") is not None else np.zeros(Cout, f32)
        act, os_ = bool(inp.get("act")), f32(inp.get("out_scale", 1.0))
        res = np.asarray(inp["res"], f32) if inp.get("res") is not None else None
        if self.epi == "stream":
            t = h16(v + (nz + bias))                                                   # fp32 up to the activation input, then fp16
            if res is not None and res_before_act:
                t = h16(t + res)
            k1 = h16(f32(SQRT2 if act else 1.0) * os_)
            k2 = h16(f32(0.2 * SQRT2 if act else 1.0) * os_)
            out = np.maximum(h16(t * k1), h16(t * k2))
            if res is not None and not res_before_act:                                  # (conv_stream has no residual; the teeth tests give it one)
                out = h16(out + res * os_)
            return out
        v = v + nz
        v = v + bias
        if res is not None and res_before_act:
            v = v + res
        if act:
            v = np.where(v > 0, v, f32(0.2) * v) * f32(SQRT2)
        if res is not None and not res_before_act:
            v = v + res
        return h16(v * os_)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(B, H, W, Cin, Cout, KS=3, stride=1, pad=None, style=False, demod=False, noise=False, batch_size=1, bias=True, act=True, res=False,
                out_scale=1.0, broadcast_x=False, premod=False, seed=0):
    """One launch's inputs.  x and res rounded to fp16; sn / dscale from util.style_tables on random latents (styles change sign and differ by
    O(1) between candidates); a noise plane per minibatch; a distinct bias per channel."""
    rng = np.random.default_rng(100003 * seed + 7919 * B + 131 * H + 17 * W + 3 * Cin + Cout + KS)
    pad = KS // 2 if pad is None else pad
    Ho, Wo = (H + 2 * pad - KS) // stride + 1, (W + 2 * pad - KS) // stride + 1
    inp = dict(B=B, stride=stride, pad=pad, act=act, out_scale=out_scale, batch_size=batch_size, premod=premod)
    inp["x"] = h16(rng.standard_normal((1 if broadcast_x else B, H, W, Cin)))
    inp["w"] = rng.standard_normal((Cout, Cin, KS, KS)).astype(np.float32)
    if style:
        L = 24
        lat = rng.standard_normal((B, L)).astype(np.float32)
        Aw = rng.standard_normal((Cin, L)).astype(np.float32)
        Ab = (0.3 * rng.standard_normal(Cin)).astype(np.float32)      # (no "+ 1": the styles change sign)
        sn, _, ds = style_tables(lat, Aw, Ab, inp["w"], demod=True)
        inp["sn"] = sn
        if demod:
            inp["dscale"] = ds
    elif demod:
        inp["dscale"] = rng.uniform(0.5, 2.0, (B, Cout)).astype(np.float32)
    if noise:
        assert B % batch_size == 0
        inp["noise"] = rng.standard_normal((B // batch_size, Ho, Wo)).astype(np.float32)
        inp["noise_strength"] = 0.3
    if bias:
        inp["bias"] = (0.1 * np.arange(Cout) / Cout - 0.05 + 0.2 * rng.standard_normal(Cout)).astype(np.float32)
    if res:
        inp["res"] = h16(rng.standard_normal((B, Ho, Wo, Cout)))
    return inp


def op_kwargs(inp):
    """The keyword arguments of ops.conv for `inp` (without x, w, impl)."""
    kw = {k: inp[k] for k in ("sn", "dscale", "noise", "noise_strength", "bias", "res") if inp.get(k) is not None}
    kw.update(stride=inp["stride"], pad=inp["pad"], act=inp["act"], out_scale=inp["out_scale"], batch_size=inp["batch_size"])
    if inp["x"].shape[0] != inp["B"]:
        kw.update(broadcast_x=True, B=inp["B"])
    if inp.get("premod"):
        kw.update(premod=True)
    return kw


def take(inp, idx):
    """The launch of the candidates `idx` alone (a noise plane per candidate): the reference of a few samples of a large launch."""
    idx = np.asarray(idx)
    out = dict(inp, B=len(idx), batch_size=1)
    if inp["x"].shape[0] == inp["B"]:
        out["x"] = inp["x"][idx]
    for k in ("sn", "dscale", "res"):
        if inp.get(k) is not None:
            out[k] = inp[k][idx]
    if inp.get("noise") is not None:
        out["noise"] = inp["noise"][idx // inp["batch_size"]]
    return out


def torgb_inputs(B, H, W, C, with_skip, seed=0):
    rng = np.random.default_rng(977 * seed + 31 * B + H + W + C + int(with_skip))
    s = (1 + 0.5 * rng.standard_normal((B, C))) * rng.uniform(0.5, 2.0, (B, 1))
    smax = np.abs(s).max(axis=1)
    return dict(w=(rng.standard_normal((3, C)) / math.sqrt(C)).astype(np.float32), b=(0.1 * rng.standard_normal(3)).astype(np.float32),
                sn=(s / smax[:, None]).astype(np.float32), smax=smax.astype(np.float32),
                yprev=rng.standard_normal((B, 3, H // 2, W // 2)).astype(np.float32) if with_skip else None)


FULL = dict(style=True, demod=True, noise=True, bias=True, act=True, out_scale=0.7)      # the full epilogue (res where the family has one)

# The cases of tests/test_gpu_conv_ops.py: name -> (family, impl, expected kernel symbol, make_inputs arguments).  test_conv_ops_ref.py runs the
# emulation at every one of them.  The derivation of each shape is in test_gpu_conv_ops.py's docstring.
CASES = {
    "direct<1>": ("conv_direct", 1, "conv_direct_kernel<1>", dict(B=2, H=5, W=7, Cin=16, Cout=16)),
    "direct<2> full": ("conv_direct", 1, "conv_direct_kernel<2>", dict(B=2, H=5, W=7, Cin=16, Cout=48, batch_size=2, res=True, **FULL)),
    "direct<4>": ("conv_direct", 1, "conv_direct_kernel<4>", dict(B=1, H=16, W=16, Cin=16, Cout=96)),
    "direct<4,rows>": ("conv_direct", 1, "conv_direct_kernel<4,rows>", dict(B=1, H=16, W=32, Cin=16, Cout=96)),
    "direct s2 res": ("conv_direct", 1, "conv_direct_kernel<1>", dict(B=2, H=9, W=9, Cin=32, Cout=32, stride=2, pad=0, res=True, out_scale=0.7)),
    "direct 1x1": ("conv_direct", 1, "conv_direct_kernel<2>", dict(B=2, H=5, W=7, Cin=16, Cout=48, KS=1, pad=0, bias=False, act=False)),
    "direct bcast": ("conv_direct", 1, "conv_direct_kernel<1>", dict(B=4, H=4, W=4, Cin=32, Cout=32, broadcast_x=True, style=True, demod=True)),
    "tiled<3,1,8,32> full": ("conv_tiled", 2, "conv_tiled_kernel<3,1,8,32>", dict(B=2, H=8, W=32, Cin=32, Cout=32, res=True, **FULL)),
    "tiled<3,1,8,64> full": ("conv_tiled", 2, "conv_tiled_kernel<3,1,8,64>", dict(B=2, H=8, W=32, Cin=96, Cout=64, batch_size=2, res=True, **FULL)),
    "tiled<3,1,8,128> full": ("conv_tiled", 2, "conv_tiled_kernel<3,1,8,128>", dict(B=1, H=16, W=64, Cin=64, Cout=128, res=True, **FULL)),
    "tiled<1,1,8,64>": ("conv_tiled", 2, "conv_tiled_kernel<1,1,8,64>", dict(B=2, H=8, W=32, Cin=32, Cout=64, KS=1, pad=0, bias=False, act=False)),
    "glds<16> full": ("conv_glds", 5, "conv_glds_kernel<16>", dict(B=2, H=16, W=16, Cin=128, Cout=128, res=True, **FULL)),
    "glds<32> full": ("conv_glds", 5, "conv_glds_kernel<32>", dict(B=1, H=16, W=32, Cin=160, Cout=128, res=True, **FULL)),
    "gldsp<f,f,f>": ("conv_glds", 5, "conv_gldsp_kernel<false,false,false>",
                     dict(B=33, H=32, W=64, Cin=128, Cout=256, demod=True, noise=True, res=True, out_scale=0.7)),
    "gldsp<f,f,t> full": ("conv_glds", 5, "conv_gldsp_kernel<false,false,true>", dict(B=33, H=32, W=64, Cin=128, Cout=256, batch_size=3, res=True, **FULL)),
    "wreg plain": ("conv_wreg", 5, "conv_wreg_kernel<false,false>", dict(B=5, H=128, W=128, Cin=64, Cout=64)),
    "wreg full": ("conv_wreg", 5, "conv_wreg_kernel<false,false>", dict(B=5, H=128, W=128, Cin=64, Cout=64, demod=True, noise=True, out_scale=0.7)),
    "wreg premod": ("conv_wreg", 5, "conv_wreg_kernel<false,false>", dict(B=5, H=128, W=128, Cin=64, Cout=64, style=True, demod=True, noise=True, out_scale=0.7, premod=True)),
    "stream full": ("conv_stream", 4, "conv_stream_kernel", dict(B=31, H=200, W=96, Cin=32, Cout=32, **FULL)),
    # the shapes of test_gpu_ops.py::test_conv_gemm_matches_direct
    "gemm conv8": ("conv_gemm", 6, "conv_gemm(im2col+gemm_tiled+finish)", dict(B=6, H=8, W=8, Cin=128, Cout=128, batch_size=2, **FULL)),
    "gemm plain8": ("conv_gemm", 6, "conv_gemm(gather+gemm_tiled+finish)", dict(B=6, H=8, W=8, Cin=128, Cout=128)),
    "gemm plain4": ("conv_gemm", 6, "conv_gemm(gather+gemm_tiled+finish)", dict(B=6, H=4, W=4, Cin=128, Cout=128)),
    "gemm skip1x1": ("conv_gemm", 6, "gemm_tiled_kernel<64>", dict(B=6, H=8, W=8, Cin=128, Cout=256, KS=1, pad=0, bias=False, act=False)),
    "gemm const4": ("conv_gemm", 6, "conv_gemm(im2col+gemm_tiled+finish)", dict(B=16, H=4, W=4, Cin=128, Cout=128, broadcast_x=True, style=True, demod=True)),
}
