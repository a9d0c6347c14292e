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

THE BigGAN FIELDS of glass_conv_desc (csrc/biggan.cpp bg_conv; inputs with pre_shift / in_up / shift / act == 2 / res_cs / res_up / rgb_tanh):

  pre_shift   the input affine a = relu(x A + S), zero at padding pixels, mirrored in the form its site takes:
     family              operand a                                                          where
     conv_tiled          relu(ra * sh + shf) in packed fp16 from the FP16 tables            conv_tiled.hip:165-170
     conv_direct         (half_t)fmaxf((float)x * s + t, 0) from the FP32 tables            conv_direct.hip:85-86
     conv_gemm (im2col)  the same form as conv_direct                                       conv_gemm.hip:37
              The compiler may contract each a * b + c ("fma", one rounding) or not ("sep", two): `pre_form` says which, and a device result
              passes when ONE form holds for the whole output.  Exact sums come from biggan_ops_ref.sum_odd (round to odd), so no float64
              sum is assumed exact.
  in_up       addressing only: (iy >> 1, ix >> 1), the padding tested at the upsampled size.
  shift       bb = bias + shift: one more fp32 addition, inside the "+ 8".
  act == 2    max(v k1, v 0): g = 1; ReLU is 1-Lipschitz, so an element with |v| <= tol may be 0 or v and the bound needs nothing more.
              conv_stream: k1 = (half_t)out_scale, k2 = 0 — the same three fp16 roundings as with act == 1.
  res_cs / res_up   addressing only: the first Cout of res_cs channels, row / column (oy >> 1, ox >> 1).
  rgb_tanh    (conv_tiled.hip:412-418) tanhf of the fp32 v of channels 0..2: NO fp16 store term — the bound of v (tanh is 1-Lipschitz) plus
              biggan_ops_ref.tanh_term, the project's rule for a float32 tanh (test_gpu_biggan_ops._f32_bar).  Returned as [B,3,Ho,Wo].

No term is fitted to an observed error."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from biggan_ops_ref import fma16, fma32, tanh_term
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


def up2(a):
    """Nearest x2 of an NHWC map: what in_up / res_up address."""
    return np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)


def pre_affine(x, A, S, table, pre_form):
    """relu(x A + S) as its site rounds it (module docstring): fp16 tables and a packed fp16 fma (conv_tiled) or fp32 tables, an fp32 fma and
    one conversion to fp16 (conv_direct, conv_gemm).  x [B,H,W,Cin] fp16 values; A, S [B,Cin] fp32."""
    x = np.asarray(x, np.float64)
    A, S = (np.asarray(t, np.float32).astype(np.float64)[:, None, None, :] for t in (A, S))
    if table == "sn16":
        v = fma16(x, h16(A).astype(np.float64), h16(S).astype(np.float64), pre_form)
    else:
        v = h16(fma32(x, A, S, pre_form))
    return np.maximum(v, 0.0).astype(np.float32)


def operands(inp, form, table, pre_form="fma"):
    """The fp16 operands of the MFMAs as float32 arrays: a [B,H,W,Cin] (the map the taps address: upsampled with in_up) and
    b [B or 1][T][Cout][Cin] — and whether dscale still applies."""
    x, sn, B = inp["x"], inp.get("sn"), inp["B"]
    wp = _pack(inp["w"])
    a = np.broadcast_to(x, (B,) + x.shape[1:]) if x.shape[0] != B else x
    b = wp[None]
    demod = inp.get("dscale") is not None
    if inp.get("pre_shift") is not None:
        assert form == "x", "the input affine is staged on the activation operand only (conv_glds / conv_stream refuse it)"
        a, sn = pre_affine(a, sn, inp["pre_shift"], table, pre_form), None
    if inp.get("in_up"):
        a = up2(a)
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


def residual(inp):
    """The residual as the epilogue addresses it: [B,Ho,Wo,Cout] from res [B,Ho >> res_up,Wo >> res_up,res_cs or Cout] (None without)."""
    if inp.get("res") is None:
        return None
    r = np.asarray(inp["res"])
    r = up2(r) if inp.get("res_up") else r
    return r[..., :inp["w"].shape[0]]


def conv_ref(inp, family, pre_form="fma"):
    """(ref, tol) of one launch under `family`'s operand form and epilogue roundings; ref and tol [B,Ho,Wo,Cout] float64 ([B,3,Ho,Wo] with
    rgb_tanh)."""
    form, table, epi = KERNELS[family]
    a, b, demod = operands(inp, form, table, pre_form)
    KS, stride, pad = inp["w"].shape[2], inp.get("stride", 1), inp.get("pad", inp["w"].shape[2] // 2)
    acc = _conv(a, b, KS, stride, pad, torch.float64)
    B, Ho, Wo, Cout = acc.shape
    K = KS * KS * a.shape[3]
    # (A only scales the bound: summed in float32 and raised by that sum's own worst-case error, it stays an upper bound of sum |a_k b_k|)
    A = _conv(np.abs(a), np.abs(b), KS, stride, pad, torch.float32).astype(np.float64) * (1 + 2 * K * U32)
    d = np.asarray(inp["dscale"], np.float64)[:, None, None, :] if demod else 1.0
    nz = _planes(inp, Ho, Wo)
    bias = np.asarray(inp["bias"], np.float64) if inp.get("bias") is not None else np.zeros(Cout)
    shift = np.asarray(inp["shift"], np.float64)[:, None, None, :] if inp.get("shift") is not None else 0.0
    pre = acc * d + nz + bias + shift
    P = A * np.abs(d) + np.abs(nz) + np.abs(bias) + np.abs(shift)
    act = int(inp.get("act") or 0)
    g = SQRT2 if act == 1 else 1.0
    os_ = float(np.float32(inp.get("out_scale", 1.0)))
    res = residual(inp)
    res = 0.0 if res is None else res.astype(np.float64)
    post = np.where(pre > 0, pre, 0.2 * pre) * SQRT2 if act == 1 else np.maximum(pre, 0.0) if act == 2 else pre
    out = (post + res) * os_
    tol = os_ * g * (2 * K + 8) * U32 * P + 4 * U32 * (np.abs(res) * os_ + np.abs(out)) + SUBNORMAL
    if inp.get("rgb_tanh"):          # tanhf of the fp32 v: no store term
        assert epi == "fp32" and family == "conv_tiled"
        v = np.ascontiguousarray(out[..., :3].transpose(0, 3, 1, 2))
        return np.tanh(v), np.ascontiguousarray(tol[..., :3].transpose(0, 3, 1, 2)) + tanh_term(v)
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

    def __init__(self, inp, family, pre_form="fma", table=None):
        self.inp, self.family = inp, family
        self.form, self.table, self.epi = KERNELS[family]
        self.table = table or self.table                                              # (a planted defect: the other family's tables)
        self.a, self.b, self.demod = operands(inp, self.form, self.table, pre_form)
        self.KS, self.stride = inp["w"].shape[2], inp.get("stride", 1)
        self.pad = inp.get("pad", self.KS // 2)
        self.acc = self.accumulate(self.a, self.b)

    def accumulate(self, a, b):
        return _conv(a, b, self.KS, self.stride, self.pad, torch.float32)

    def finish(self, acc=None, noise_planes=None, res_before_act=False, res=None, relu_before_shift=False, tanh_of_fp16=False):
        """acc / noise_planes / res: replacements (a planted defect's); res_before_act, relu_before_shift, tanh_of_fp16: planted defects."""
        inp = self.inp
        f32 = np.float32
        v = (self.acc if acc is None else acc).astype(f32)
        B, Ho, Wo, Cout = v.shape
        if self.demod:
            v = v * np.asarray(inp["dscale"], f32)[:, None, None, :]
        nz = (_planes(inp, Ho, Wo) if noise_planes is None else noise_planes).astype(f32)
        bias = np.asarray(inp["bias"], f32) if inp.get("bias") is not None else np.zeros(Cout, f32)
        shift = np.asarray(inp["shift"], f32)[:, None, None, :] if inp.get("shift") is not None else None
        act, os_ = int(inp.get("act") or 0), f32(inp.get("out_scale", 1.0))
        if res is None:
            res = residual(inp)
        res = None if res is None else np.asarray(res, f32)
        if self.epi == "stream":
            bb = bias if shift is None else bias + shift                                # Cb = bias + shift (conv_stream.hip:200)
            t = h16(v + (nz + bb))                                                     # fp32 up to the activation input, then fp16
            if res is not None and res_before_act:
                t = h16(t + res)
            k1 = h16(f32(SQRT2 if act == 1 else 1.0) * os_)
            k2 = h16(f32(0.2 * SQRT2 if act == 1 else 0.0 if act == 2 else 1.0) * os_)
            out = np.maximum(h16(t * k1), h16(t * k2))
            if res is not None and not res_before_act:                                  # (conv_stream has no residual; the teeth tests give it one)
                out = h16(out + res * os_)
            return out
        v = v + nz
        v = v + bias
        if relu_before_shift:
            v = np.maximum(v, f32(0))
        if shift is not None:
            v = v + shift
        if res is not None and res_before_act:
            v = v + res
        if act == 1:
            v = np.where(v > 0, v, f32(0.2) * v) * f32(SQRT2)
        elif act == 2 and not relu_before_shift:
            v = np.maximum(v, f32(0))
        if res is not None and not res_before_act:
            v = v + res
        if inp.get("rgb_tanh"):
            v = np.ascontiguousarray((v * os_)[..., :3].transpose(0, 3, 1, 2))
            return np.tanh(h16(v) if tanh_of_fp16 else v)
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


# ---- the BigGAN path's conv forms (csrc/biggan.cpp bg_conv): inputs, cases, lattice builders ---------------------------------------------------
FAMILY_OF_IMPL = {1: "conv_direct", 2: "conv_tiled", 4: "conv_stream", 5: "conv_glds", 6: "conv_gemm"}
OLD_BAR = 5e-3                       # x max|ref|: the bar these cases were held to before the per-element bound
PRE_FORMS = ("fma", "sep")


def stream_shape(cus=256):
    """The smallest map choose_conv_stream accepts: 64 nominal candidates x (W / 32) (H / 8) tiles >= 6 per slot, 3 slots per CU."""
    need = -(-cus * 3 * 6 // 64)
    return 64, 32 * -(-need // 8)


def _bg_tables(rng, B, C):
    """Per-(candidate, channel) scale and shift: O(1) apart between candidates and channels, both signs; the shift has a positive mean."""
    A = (rng.standard_normal((B, C)) + 0.8 * rng.choice([-1.0, 1.0], (B, 1))).astype(np.float32)
    S = (0.6 + 0.8 * rng.standard_normal((B, C))).astype(np.float32)
    return A, S


def _bg_xw(rng, B, H, W, Cin, Cout, ks):
    return h16(rng.standard_normal((B, H, W, Cin))), rng.standard_normal((Cout, Cin, ks, ks)).astype(np.float32)


def bg_inputs(form, impl, B, H, W, Cin, Cout, up=False, res_mult=1, res_up=False, seed=None):
    """The inputs of one BigGAN conv form, drawn exactly as test_gpu_biggan_ops.py drew them under the 5e-3 max|ref| bar.  H, W: the STORED
    input map (conv1 with up: the output is twice that)."""
    inp = dict(B=B, stride=1, out_scale=1.0, batch_size=1, act=0, form=form, impl=impl)
    if form == "conv0":
        rng = np.random.default_rng(100 + impl + H if seed is None else seed)
        inp["x"], inp["w"] = _bg_xw(rng, B, H, W, Cin, Cout, 1)
        inp["sn"], inp["pre_shift"] = _bg_tables(rng, B, Cin)
        inp["dscale"], inp["shift"] = _bg_tables(rng, B, Cout)
        inp["act"] = 2
    elif form in ("conv1", "conv2"):
        rng = np.random.default_rng((200 + impl + Cin if form == "conv1" else 300 + Cin) if seed is None else seed)
        inp["x"], inp["w"] = _bg_xw(rng, B, H, W, Cin, Cout, 3)
        inp["dscale"], inp["shift"] = _bg_tables(rng, B, Cout)
        inp["act"], inp["in_up"] = 2, bool(up)
    elif form == "conv3":
        rng = np.random.default_rng(400 + res_mult + res_up if seed is None else seed)
        inp["x"], inp["w"] = _bg_xw(rng, B, H, W, Cin, Cout, 1)
        inp["bias"] = rng.standard_normal(Cout).astype(np.float32)
        rcs = res_mult * Cout
        inp["res"] = h16(rng.standard_normal((B, H >> res_up, W >> res_up, rcs)) + np.arange(B)[:, None, None, None])     # O(1) apart per candidate
        inp["res_cs"], inp["res_up"] = (rcs if res_mult > 1 else 0), bool(res_up)
    elif form == "final":
        rng = np.random.default_rng(500 + H if seed is None else seed)
        inp["x"], inp["w"] = _bg_xw(rng, B, H, W, 128, 32, 3)
        inp["sn"], inp["pre_shift"] = _bg_tables(rng, B, 128)
        inp["bias"] = (0.2 * rng.standard_normal(32)).astype(np.float32)
        inp["rgb_tanh"] = True
    else:
        raise ValueError(form)
    inp["pad"] = inp["w"].shape[2] // 2
    return inp


def bg_op_kwargs(inp):
    """The keyword arguments of ops.conv for a BigGAN form (without x, w)."""
    kw = {k: inp[k] for k in ("sn", "pre_shift", "dscale", "shift", "bias", "res") if inp.get(k) is not None}
    kw.update(impl=inp["impl"], act=inp["act"], in_up=bool(inp.get("in_up")), res_cs=inp.get("res_cs", 0), res_up=bool(inp.get("res_up")),
              rgb_tanh=bool(inp.get("rgb_tanh")))
    return kw


def old_bar(inp, ref):
    """What the case was held to before: 5e-3 max|ref| of the float64 reference WITHOUT the mirrored input affine."""
    return OLD_BAR * float(np.abs(ref).max())


# name -> (arguments of bg_inputs, the symbol ops.last_kernel() must report).  H = 0: stream_shape() of the device.
BG_CASES = {
    "conv0 tiled 8x32": (dict(form="conv0", impl=2, B=3, H=8, W=32, Cin=128, Cout=32), "conv_tiled_kernel<1,1,8,32>"),
    "conv0 tiled 24x64": (dict(form="conv0", impl=2, B=2, H=24, W=64, Cin=128, Cout=32), "conv_tiled_kernel<1,1,8,32>"),
    "conv0 gemm 4x4": (dict(form="conv0", impl=6, B=3, H=4, W=4, Cin=256, Cout=64), "conv_gemm(im2col+gemm_tiled+finish)"),
    "conv0 direct 8x8": (dict(form="conv0", impl=1, B=3, H=8, W=8, Cin=128, Cout=32), "conv_direct_kernel<1>"),
    "conv1 tiled up 32": (dict(form="conv1", impl=2, B=3, H=12, W=32, Cin=32, Cout=32, up=True), "conv_tiled_kernel<3,1,8,32>"),
    "conv1 tiled up 64": (dict(form="conv1", impl=2, B=3, H=12, W=32, Cin=64, Cout=64, up=True), "conv_tiled_kernel<3,1,8,64>"),
    "conv1 gemm up 64": (dict(form="conv1", impl=6, B=3, H=4, W=4, Cin=64, Cout=64, up=True), "conv_gemm(im2col+gemm_tiled+finish)"),
    "conv1 direct up 64": (dict(form="conv1", impl=1, B=3, H=4, W=4, Cin=64, Cout=64, up=True), "conv_direct_kernel<2>"),
    "conv1 gemm up 128": (dict(form="conv1", impl=6, B=3, H=4, W=4, Cin=128, Cout=128, up=True), "conv_gemm(im2col+gemm_tiled+finish)"),
    "conv1 gemm 64": (dict(form="conv1", impl=6, B=3, H=4, W=4, Cin=64, Cout=64), "conv_gemm(gather+gemm_tiled+finish)"),
    "conv1 gemm 256": (dict(form="conv1", impl=6, B=3, H=4, W=4, Cin=256, Cout=256), "conv_gemm(gather+gemm_tiled+finish)"),
    "conv2 glds<16>": (dict(form="conv2", impl=5, B=3, H=16, W=16, Cin=128, Cout=128), "conv_glds_kernel<16>"),
    "conv2 glds<32>": (dict(form="conv2", impl=5, B=3, H=16, W=32, Cin=128, Cout=128), "conv_glds_kernel<32>"),
    "conv2 stream": (dict(form="conv2", impl=4, B=2, H=0, W=0, Cin=32, Cout=32), "conv_stream_kernel"),
    "conv2 tiled": (dict(form="conv2", impl=2, B=2, H=0, W=0, Cin=32, Cout=32), "conv_tiled_kernel<3,1,8,32>"),
    "conv2 gemm 8x8": (dict(form="conv2", impl=6, B=3, H=8, W=8, Cin=64, Cout=64), "conv_gemm(gather+gemm_tiled+finish)"),
    "final tanh 8x32": (dict(form="final", impl=2, B=3, H=8, W=32, Cin=128, Cout=32), "conv_tiled_kernel<3,1,8,32>"),
    "final tanh 24x64": (dict(form="final", impl=2, B=2, H=24, W=64, Cin=128, Cout=32), "conv_tiled_kernel<3,1,8,32>"),
}
_CONV3_KERNEL = {2: "conv_tiled_kernel<1,1,8,64>", 6: "conv_gemm(im2col+gemm_tiled+finish)", 1: "conv_direct_kernel<2>"}
for _impl in (2, 6, 1):
    for _rm, _ru in ((2, True), (1, False), (2, False)):
        BG_CASES["conv3 %s res_cs %d up%d" % (FAMILY_OF_IMPL[_impl][5:], _rm * 64, _ru)] = (
            dict(form="conv3", impl=_impl, B=3, H=8, W=32, Cin=64, Cout=64, res_mult=_rm, res_up=_ru), _CONV3_KERNEL[_impl])


def bg_case_name(args):
    """The name under which BG_CASES holds these bg_inputs arguments."""
    given = {k: v for k, v in args.items() if v not in (False, None)}          # (up / res_up False are the defaults the table leaves out)
    for name, (a, _) in BG_CASES.items():
        if {k: v for k, v in a.items() if v not in (False, None)} == given:
            return name
    raise KeyError(args)


def bg_case(name, cus=256, lattice=False):
    """The inputs of BG_CASES[name] (lattice: on the lattice, with the exact result: (inp, want))."""
    args = dict(BG_CASES[name][0])
    if args["H"] == 0:
        args["H"], args["W"] = stream_shape(cus)
    return bg_lattice(**args) if lattice else bg_inputs(**args)


def bg_lattice(form, impl, B, H, W, Cin, Cout, up=False, res_mult=1, res_up=False, seed=0):
    """A BigGAN form on the lattice, and what a correct kernel MUST return bit for bit: (inp, want).
    x in multiples of 1/4 up to 1; A signed powers of two in +-{1/2, 1, 2} and S in multiples of 1/8, both per candidate and channel, so that
    relu(x A + S) is the same bits under both forms and both tables; packed weights in {0, +-1/4, +-1/2} (through host_pack_conv); dscale signed
    powers of two; shift / bias / res dyadic.  Then the accumulator is exact in every order and v = acc d + bias + shift (+ res) is exact in
    fp32, contracted or not: want = fp16(v), one rounding.  final: want = the exact fp32 v [B,3,H,W] — the output is tanhf of it — and the
    weights are sparse enough that at least half of the values have |v| <= 2.  Every premise is asserted."""
    from fir_ops_ref import assert_order_free, lattice_weights, pow2, quantum
    rng = np.random.default_rng([seed, impl, B, H, W, Cin, Cout, len(form)])
    KS = 1 if form in ("conv0", "conv3") else 3
    f32, f64 = np.float32, np.float64
    inp = dict(B=B, stride=1, pad=KS // 2, out_scale=1.0, batch_size=1, act=0, form=form, impl=impl)
    inp["x"] = (rng.integers(-4, 5, (B, H, W, Cin)) / 4.0).astype(f32)
    w = lattice_weights(rng, (Cout, Cin, KS, KS), [0, 0.25, -0.25, 0.5, -0.5], Cin * KS * KS)
    if form == "final":                                                        # sparse: tanh must not saturate
        w = w * (rng.random(w.shape) < 12.0 / (Cin * KS * KS))
        assert np.array_equal(np.abs(_pack(w)) > 0, np.abs(w.transpose(2, 3, 0, 1).reshape(KS * KS, Cout, Cin)) > 0)
    inp["w"] = w.astype(f32)
    family = FAMILY_OF_IMPL[impl]
    fam_form, table, _ = KERNELS[family]
    if form in ("conv0", "final"):
        inp["sn"] = pow2(rng, (B, Cin), [-1, 0, 1])
        inp["pre_shift"] = (rng.integers(-8, 9, (B, Cin)) / 8.0).astype(f32)
        want_a = np.maximum(inp["x"].astype(f64) * inp["sn"].astype(f64)[:, None, None, :] + inp["pre_shift"].astype(f64)[:, None, None, :], 0.0)
        for tb in ("sn", "sn16"):
            for pf in PRE_FORMS:
                assert np.array_equal(pre_affine(inp["x"], inp["sn"], inp["pre_shift"], tb, pf), want_a), "lattice: relu(x A + S) depends on the form"
    if form in ("conv0", "conv1", "conv2"):
        inp["dscale"] = pow2(rng, (B, Cout), [-1, 0, 1])
        inp["shift"] = (rng.integers(-32, 33, (B, Cout)) / 16.0).astype(f32)
        inp["act"], inp["in_up"] = 2, bool(up)
    if form == "conv3":
        inp["bias"] = (rng.integers(-32, 33, Cout) / 16.0).astype(f32)
        rcs = res_mult * Cout
        inp["res"] = ((rng.integers(-8, 9, (B, H >> res_up, W >> res_up, rcs)) + 4 * np.arange(B)[:, None, None, None]) / 4.0).astype(f32)
        inp["res_cs"], inp["res_up"] = (rcs if res_mult > 1 else 0), bool(res_up)
    if form == "final":               # a bias of 14 fractional bits: v needs more than fp16's 11 bits, so tanhf(fp16(v)) shows
        inp["bias"] = (rng.integers(-8192, 8193, Cout) / 16384.0).astype(f32)
        inp["rgb_tanh"] = True
    a, b, demod = operands(inp, fam_form, table)
    name = "bg lattice %s impl %d" % (form, impl)
    acc = assert_order_free(name, _conv, a, b, KS, 1, KS // 2)
    A = _conv(np.abs(a), np.abs(b), KS, 1, KS // 2, torch.float64)
    d = inp["dscale"].astype(f64)[:, None, None, :] if demod else np.ones((1, 1, 1, 1))
    bb = (inp["bias"].astype(f64) if inp.get("bias") is not None else 0.0) + (inp["shift"].astype(f64)[:, None, None, :] if inp.get("shift") is not None else 0.0)
    bb = np.broadcast_to(bb, acc.shape)
    r = residual(inp)
    r = np.zeros((1, 1, 1, 1)) if r is None else r.astype(f64)
    q = min(quantum(acc) * float(np.abs(d).min()), quantum(bb), quantum(r))
    P = A * np.abs(d) + np.abs(bb) + np.abs(r)
    assert P.max() < 2.0 ** 24 * q, "%s: |acc d| + |bias + shift| + |res| reaches %.3g, v is exact below 2^24 q = %.3g" % (name, P.max(), 2.0 ** 24 * q)
    v = acc * d + bb
    v = (np.maximum(v, 0.0) if inp["act"] == 2 else v) + r
    assert np.array_equal(v, v.astype(f32).astype(f64)) and np.abs(v).max() < 65504
    if form == "final":
        v = np.ascontiguousarray(v[..., :3].transpose(0, 3, 1, 2))
        assert (v != h16(v)).mean() >= 0.25, "%s: v fits fp16 almost everywhere: a tanh of the rounded value would not show" % name
        assert (np.abs(v) <= 2.0).mean() >= 0.5, "%s: tanh saturates on more than half of the pixels (%.2f within 2)" % (name, (np.abs(v) <= 2.0).mean())
        return inp, v
    return inp, h16(v)


# the lattice runs of test_gpu_biggan_ops.py: one per conv form and family reached
BG_LATTICE = ("conv0 tiled 8x32", "conv0 direct 8x8", "conv0 gemm 4x4", "conv1 tiled up 32", "conv1 gemm up 64", "conv2 glds<16>", "conv2 glds<32>",
              "conv2 stream", "conv2 tiled", "conv3 tiled res_cs 128 up1", "conv3 gemm res_cs 128 up1", "conv3 direct res_cs 128 up1", "final tanh 8x32")
