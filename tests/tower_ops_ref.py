"""float64 references of the convolutions, pools and token builder of the two scoring networks (CLIP's ResNet towers, the LPIPS VGG16 walk), an
error bound PER ELEMENT, an fp32 emulation of a faithful kernel, lattice inputs whose result is exact, and the cases the CPU and the GPU tests
share (TEST INFRASTRUCTURE; tests/test_tower_ops_ref.py, tests/test_gpu_tower_ops.py).

Every reference returns (ref, tol), float64 arrays of the output's shape.  Nothing here is measured on the device, no term is fitted to an
observed error.

BN-EPILOGUE CONVS: gemm_tiled mode 5 (gemm_tiled.hip:123-158; 1 x 1 through rn_gemm_1x1, 3 x 3 through the implicit patch matrix of
rn_gemm_3x3, clip.cpp:423-435), rn_conv3x3_kernel (clip_resnet.hip:91-101), and VGG16's features.2 .. features.28 as a = 1, s = bias
(lpips.cpp:105).  The operands are the fp16 values themselves: rn_pack_conv (clip.cpp:178-184) only rounds and reorders, there is no style.
With K = KS^2 Cin products per output element,
  acc = sum a_k w_k,  A = sum |a_k w_k|        (A summed in fp32 and raised by that sum's own worst case, as conv_ops_ref.conv_ref does)
  v = acc a_n + s_n (+ r),  out = relu(v) or v
  tol = (2 K + 8) U32 (A |a_n| + |s_n| + |r|)  +  U16 |out|  +  2^-24
  (2 K + 8) U32 (..)  the order-free summation bound K u sum|terms| of the MFMA chain (gemm_tiled.hip:103-122, clip_resnet.hip:75-89) and the
                      epilogue's fp32 operations (gemm_tiled.hip:152-153: the product with a_n, the sum with s_n, the residual's conversion and
                      sum — at most four; eight is the allowance conv_ops_ref uses).  The factor 2 on K is the project's standing margin for
                      the MFMA's internal accumulation order, which NOBODY HERE HAS MEASURED.
  U16 |out|           the one fp16 rounding, at the store (gemm_tiled.hip:154, clip_resnet.hip:99).
  2^-24               half the smallest fp16 subnormal.
The bound does not pass through the ReLU: an element with |v| <= tol may come back as 0 or as v, both are inside |got - relu(v)| <= tol.
Where (2 K + 8) U32 A |a_n| dominates U16 |out| (K >= 2304) the bound is wider than an fp16 ulp by construction: the LATTICE runs are the sharp
check there.

SCALAR CONVS: rn_stem_conv1_kernel (clip_resnet.hip:27-45: 27 fp32 FMAs in a fixed order, then acc a + s, ReLU, one fp16 store) and
vgg_conv1_kernel (lpips.hip:55-73: the same with + bias).  No MFMA: the same form with (K + 8) U32, K = 27.  The stem's operand is the fp16 image
as launch_image_patches writes it (ops.hip glass_op_rn_stem_conv1); VGG's fourth input channel is zero and has no weights.

rn_avgpool2_kernel (clip_resnet.hip:127): three fp32 additions, an exact product with 0.25, one fp16 store:
  tol = 3 U32 sum|v| / 4 + U16 |out| + 2^-24.
rn_attnpool_tokens_kernel (clip_resnet.hip:145-150): a pixel row is one fp32 addition (v + pos) and the fp16 store:
  tol = U32 (|v| + |pos|) + U16 |out| + 2^-24;
the mean row is HW - 1 additions, a division, the addition of pos and the store:
  tol = (HW + 2) U32 (sum|v| / HW + |pos|) + U16 |out| + 2^-24.
maxpool2_kernel (lpips.hip:95) is exact: the tests ask for equality.

LATTICE INPUTS make the result unique.  The map holds multiples of 1/4 up to 1, the weights lie in {0, +-1/4, +-1/2}: every product is a
multiple of q = 1/16 and sum |a_k w_k| <= K / 2 (2304 = 36864 q at K = 4608) stays below 2^24 q, so the accumulator is exact in fp32 in any
order (fir_ops_ref.assert_order_free).  bn_a takes signed powers of two, bn_s and the residual are dyadic, and A |a| + |s| + |r| stays below
2^24 times the smallest quantum of the three terms: v is exact in fp32 whether or not the compiler contracts acc a + s into an fma (asserted
in float64, lattice_premise).  The output is then fp16(v) with the ReLU applied — one deterministic rounding — and the device must return
these bits."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from fir_ops_ref import _conv as conv_packed
from fir_ops_ref import assert_order_free, pow2, quantum
from glue_ops_ref import U16, U32, h16

f32, f64 = np.float32, np.float64
SUBNORMAL = 2.0 ** -24


# ---- convolutions ---------------------------------------------------------------------------------------------------------------------------------
def _conv(x, w, stride, dtype, pad="zero"):
    """sum_k a_k w_k of NHWC x and w [Cout,Cin,KS,KS] (pad KS // 2; "clamp": the border repeated, a planted defect) in `dtype` -> [B,Ho,Wo,Cout]."""
    xt = torch.as_tensor(np.ascontiguousarray(np.asarray(x).transpose(0, 3, 1, 2))).to(dtype)
    wt = torch.as_tensor(np.ascontiguousarray(w)).to(dtype)
    p = wt.shape[-1] // 2
    if pad == "clamp" and p:
        xt, p = F.pad(xt, (p, p, p, p), mode="replicate"), 0
    return np.ascontiguousarray(F.conv2d(xt, wt, stride=stride, padding=p).permute(0, 2, 3, 1).numpy())


def conv_geometry(inp):
    """(x NHWC, w [Cout,Cin,KS,KS], stride, mfma) of a conv case: the operands as the kernel multiplies them."""
    op = inp["op"]
    if op == "stem1":
        return np.ascontiguousarray(inp["x"].transpose(0, 2, 3, 1)), inp["w"], 2, False
    if op == "vgg1":
        return inp["x"][..., :3], inp["w"], 1, False
    return inp["x"], inp["w"], 1, True


def conv_bn_ref(x, w, a, s, res=None, relu=True, stride=1, mfma=True):
    """(ref, tol) of act(conv(x, w) a + s (+ res)); x, res NHWC and w [Cout,Cin,KS,KS] holding fp16 values (or float64: nothing is rounded here)."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    acc = _conv(np.asarray(x, f64), np.asarray(w, f64), stride, torch.float64)
    A = _conv(np.abs(x).astype(f32), np.abs(w).astype(f32), stride, torch.float32).astype(f64) * (1 + 2 * K * U32)
    a, s = np.asarray(a, f64), np.asarray(s, f64)
    r = np.asarray(res, f64) if res is not None else 0.0
    v = acc * a + s + r
    out = np.maximum(v, 0) if relu else v
    tol = ((2 if mfma else 1) * K + 8) * U32 * (A * np.abs(a) + np.abs(s) + np.abs(r)) + U16 * np.abs(out) + SUBNORMAL
    return out, tol


def avgpool_ref(x):
    x = np.asarray(x, f64)
    B, H, W, C = x.shape
    q = lambda t: t.reshape(B, H // 2, 2, W // 2, 2, C)
    out = q(x).sum(axis=(2, 4)) / 4
    return out, 3 * U32 * q(np.abs(x)).sum(axis=(2, 4)) / 4 + U16 * np.abs(out) + SUBNORMAL


def tokens_ref(x, pos):
    x, pos = np.asarray(x, f64), np.asarray(pos, f64)
    B, HW, C = x.shape
    out = np.concatenate([x.mean(axis=1, keepdims=True), x], axis=1) + pos[None]
    tol = np.empty_like(out)
    tol[:, 1:] = U32 * (np.abs(x) + np.abs(pos[None, 1:]))
    tol[:, 0] = (HW + 2) * U32 * (np.abs(x).sum(axis=1) / HW + np.abs(pos[0]))
    return out, tol + U16 * np.abs(out) + SUBNORMAL


def maxpool_ref(x):
    B, H, W, C = x.shape
    return np.asarray(x, f32).reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def reference(inp):
    """(ref, tol) of a case's inputs."""
    op = inp["op"]
    if op == "avgpool":
        return avgpool_ref(inp["x"])
    if op == "tokens":
        return tokens_ref(inp["x"], inp["pos"])
    x, w, stride, mfma = conv_geometry(inp)
    return conv_bn_ref(x, w, inp["a"], inp["s"], inp.get("res"), inp["relu"], stride, mfma)


# ---- the fp32 emulation of a faithful kernel ------------------------------------------------------------------------------------------------------------
def fp32_emulation(inp, hook=None):
    """fp32 accumulators (torch float32 conv of the operands), the epilogue in fp32 as the kernels write it, one fp16 store.  hook: a dict that
    replaces pieces with planted defects —
      "x", "w"     the operands (arrays in conv_geometry's layout)        "pad"       "clamp": the border repeated instead of zeros
      "acc"        callable(acc) -> accumulators                          "epilogue"  callable(acc, a, s, res, relu) -> the value stored (fp32)
      "out"        callable(out) -> the stored fp16 values"""
    hook = hook or {}
    op = inp["op"]
    if op == "avgpool":
        x = np.asarray(inp["x"], f32)
        B, H, W, C = x.shape
        q = x.reshape(B, H // 2, 2, W // 2, 2, C)
        return h16(((q[:, :, 0, :, 0] + q[:, :, 0, :, 1]) + (q[:, :, 1, :, 0] + q[:, :, 1, :, 1])) * f32(0.25))
    if op == "tokens":
        x, pos = np.asarray(inp["x"], f32), np.asarray(inp["pos"], f32)
        HW = x.shape[1]
        s = np.zeros_like(x[:, 0])
        for i in range(HW):
            s = s + x[:, i]
        return h16(np.concatenate([(s / f32(HW) + pos[0])[:, None], x + pos[None, 1:]], axis=1))
    x, w, stride, _ = conv_geometry(inp)
    acc = _conv(np.asarray(hook.get("x", x), f32), np.asarray(hook.get("w", w), f32), stride, torch.float32, hook.get("pad", "zero"))
    if "acc" in hook:
        acc = np.asarray(hook["acc"](acc), f32)
    a, s = np.asarray(inp["a"], f32), np.asarray(inp["s"], f32)
    res = np.asarray(inp["res"], f32) if inp.get("res") is not None else None
    if "epilogue" in hook:
        v = np.asarray(hook["epilogue"](acc, a, s, res, inp["relu"]), f32)
    else:
        v = acc * a + s
        if res is not None:
            v = v + res
        if inp["relu"]:
            v = np.maximum(v, f32(0))
    out = h16(v)
    return hook["out"](out) if "out" in hook else out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------
def _bn(rng, C, vgg):
    """BatchNorm as scale and shift: scales of both signs around 1 and a shift that leaves both sides of the ReLU populated (accumulators have
    std ~ sqrt 2, the shift 0.3); VGG: a = 1, s = the bias."""
    if vgg:
        return np.ones(C, f32), (0.1 * rng.standard_normal(C)).astype(f32)
    a = rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.125, -1.0, 1.0)
    return a.astype(f32), (0.3 * rng.standard_normal(C)).astype(f32)


def lattice_premise(name, inp):
    """The premise of a lattice case, asserted in float64 (module docstring): exact accumulators in any order, v exact in 24 bits with or without
    contraction, outputs inside fp16's range.  Returns the bits the device must return (float32 array of fp16 values)."""
    x, w, stride, _ = conv_geometry(inp)
    assert stride == 1
    x, w = np.array(x, f32), np.array(w, f32)      # (copies: the shared inputs of case() are read-only)
    Cout, Cin, KS, _ = w.shape
    wp = np.ascontiguousarray(w.transpose(2, 3, 0, 1).reshape(KS * KS, Cout, Cin)).astype(f32)      # [T][Cout][Cin], rn_pack_conv's layout
    acc = assert_order_free(name, conv_packed, np.asarray(x, f32), wp, 1, KS // 2)
    A = conv_packed(np.abs(x).astype(f32), np.abs(wp), 1, KS // 2, torch.float64)
    K = KS * KS * Cin
    assert A.max() <= K / 2 and quantum(x) * quantum(w) >= 1.0 / 16 and A.max() < 2.0 ** 24 / 16
    a, s = np.asarray(inp["a"], f64), np.asarray(inp["s"], f64)
    r = np.asarray(inp["res"], f64) if inp.get("res") is not None else np.zeros(1)
    assert np.all(np.abs(np.frexp(a)[0]) == 0.5), "bn_a is not a signed power of two"
    q = min(quantum(acc) * np.abs(a).min(), quantum(s), quantum(r))
    P = A * np.abs(a) + np.abs(s) + np.abs(r)
    assert P.max() < 2.0 ** 24 * q, "%s: |acc a| + |s| + |r| reaches %.3g, v is exact below 2^24 q = %.3g" % (name, P.max(), 2.0 ** 24 * q)
    v = acc * a + s + r
    assert np.array_equal(v, v.astype(f32).astype(f64)) and np.array_equal(acc * a, (acc * a).astype(f32).astype(f64))
    out = np.maximum(v, 0) if inp["relu"] else v
    assert np.abs(out).max() < 65504
    return h16(out)


def make_inputs(name):
    """The inputs of CASES[name]: dict(op, x, w, a, s, res, relu, lattice) — conv ops — or dict(op, x[, pos])."""
    op, _, sh, seed = CASES[name]
    rng = np.random.default_rng([seed, len(name)] + [ord(c) for c in name])
    if op == "avgpool":
        return dict(op=op, x=h16(rng.standard_normal((sh["B"], sh["H"], sh["W"], sh["C"]))))
    if op == "tokens":
        return dict(op=op, x=h16(rng.standard_normal((sh["B"], sh["HW"], sh["C"]))), pos=(0.3 * rng.standard_normal((sh["HW"] + 1, sh["C"]))).astype(f32))
    if op == "stem1":
        a, s = _bn(rng, sh["C1"], False)
        return dict(op=op, x=h16(rng.standard_normal((sh["B"], 3, sh["S"], sh["S"]))), w=h16(rng.standard_normal((sh["C1"], 3, 3, 3)) * (2.0 / 27) ** 0.5),
                    a=a, s=s, res=None, relu=True, lattice=False)
    if op == "vgg1":
        x = np.zeros((sh["B"], sh["S"], sh["S"], 4), f32)
        x[..., :3] = h16(2.0 * rng.standard_normal((sh["B"], sh["S"], sh["S"], 3)))
        a, s = _bn(rng, 64, True)
        return dict(op=op, x=x, w=h16(rng.standard_normal((64, 3, 3, 3)) * (2.0 / 27) ** 0.5), a=a, s=s, res=None, relu=True, lattice=False)
    B, H, W, Cin, Cout = sh["B"], sh["H"], sh["W"], sh["Cin"], sh["Cout"]
    KS = 1 if op == "conv1x1" else 3
    relu, res, lattice = sh.get("relu", True), sh.get("res", False), sh.get("lattice", False)
    if not lattice:
        a, s = _bn(rng, Cout, op == "vgg")
        return dict(op=op, x=h16(rng.standard_normal((B, H, W, Cin))), w=h16(rng.standard_normal((Cout, Cin, KS, KS)) * (2.0 / (Cin * KS * KS)) ** 0.5),
                    a=a, s=s, res=h16(rng.standard_normal((B, H, W, Cout))) if res else None, relu=relu, lattice=False)
    x = (rng.integers(-4, 5, (B, H, W, Cin)) / 4.0).astype(f32)
    w = rng.choice(np.array([0, 0.25, -0.25, 0.5, -0.5], f32), size=(Cout, Cin, KS, KS))
    a = np.ones(Cout, f32) if op == "vgg" else pow2(rng, (Cout,), [-2, -1, 0])
    s = (rng.integers(-32, 33, Cout) / 64.0).astype(f32)
    r = (rng.integers(-4, 5, (B, H, W, Cout)) / 4.0).astype(f32) if res else None
    if sh.get("negsum"):      # the sum negative where the residual alone is positive: x >= 0, the first half of the channels with w <= 0 and a > 0, r = 1/4
        x, a, r = np.abs(x), np.abs(a), np.full((B, H, W, Cout), 0.25, f32)
        w = np.abs(w)
        w[:Cout // 2] *= -1
    return dict(op=op, x=x, w=w, a=a, s=s, res=r, relu=relu, lattice=True)


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, ref, tol) of CASES[name], computed once per process and shared by the tests that need them (do not modify the arrays)."""
    inp = make_inputs(name)
    ref, tol = reference(inp)
    for arr in [ref, tol] + [v for v in inp.values() if isinstance(v, np.ndarray)]:
        arr.setflags(write=False)
    return inp, ref, tol


def run(inp):
    """The diagnostic op of a case's inputs on the device."""
    from clip_glass_amd import ops
    op = inp["op"]
    if op == "avgpool":
        return ops.rn_avgpool(inp["x"])
    if op == "tokens":
        return ops.rn_tokens(inp["x"], inp["pos"])
    if op == "stem1":
        return ops.rn_stem_conv1(inp["x"], inp["w"], inp["a"], inp["s"])
    if op == "vgg1":
        return ops.vgg_conv1(inp["x"], inp["w"], inp["s"])
    return ops.rn_conv_bn(inp["x"], inp["w"], inp["a"], inp["s"], res=inp.get("res"), relu=inp["relu"], form=1 if op == "stem3x3" else 0)


def relu_sides(ref):
    """(fraction above 0, fraction at 0) of a reference."""
    return float((ref > 0).mean()), float((ref == 0).mean())


def border_slices(ref):
    """The four border slices of an image-shaped output [B,H,W,C]."""
    return (("top", np.s_[:, 0]), ("bottom", np.s_[:, -1]), ("left", np.s_[:, :, 0]), ("right", np.s_[:, :, -1])) if ref.ndim == 4 else ()


# ---- the cases: name -> (op, expected kernel symbol, shapes, seed) -------------------------------------------------------------------------------------
# ops: conv1x1 / gather / vgg = ops.rn_conv_bn form 0 (KS 1 / 3 / 3 with a = 1, s = bias); stem3x3 = form 1; stem1, vgg1, avgpool, tokens.
# gemm_tiled's fill rule (gemm_tiled.hip:223-229, cand_rows = H W, GLASS_NOMINAL_POP = 64): the 128-wide instance runs when N % 128 == 0 and
# ceil(H W 64 / 128) (N / 128) >= 256 — at N = 256 from H W = 255 on (15 x 17: 128 x 2 = 256; 254 gives 254).  N = 192 is no multiple of 128: 64-wide.
G64, G128, T64, T128 = ("gemm_tiled_kernel<64,false,bn>", "gemm_tiled_kernel<128,false,bn>", "gemm_tiled_kernel<64,true,bn>", "gemm_tiled_kernel<128,true,bn>")
CASES = {}
for _B, _H in ((2, 7), (3, 2)):                      # M = 98 (no tile multiple) and M = 12 (below 64: the padded rows are computed and stored)
    for _K, _N in ((64, 64), (256, 64), (64, 192), (256, 192)):
        for _res, _relu in ((False, True), (True, True), (True, False), (False, False)):
            CASES["1x1 M%d K%d N%d res%d relu%d" % (_B * _H * _H, _K, _N, _res, _relu)] = ("conv1x1", G64, dict(B=_B, H=_H, W=_H, Cin=_K, Cout=_N, res=_res, relu=_relu), 32)
CASES.update({
    "1x1 128-wide 17x17": ("conv1x1", G128, dict(B=1, H=17, W=17, Cin=64, Cout=256, res=True), 33),          # M = 289: two m tiles and 33 rows
    "gather rn 7x7": ("gather", T64, dict(B=2, H=7, W=7, Cin=64, Cout=64), 34),
    "gather rn 5x9": ("gather", T64, dict(B=2, H=5, W=9, Cin=64, Cout=64), 34),
    "gather rn 2x2 M12": ("gather", T64, dict(B=3, H=2, W=2, Cin=64, Cout=64), 34),                          # M = 12: the poisoned tail is never fetched
    "vgg 64-128 8x8": ("vgg", T64, dict(B=1, H=8, W=8, Cin=64, Cout=128), 35),
    "vgg 128-256 4x4": ("vgg", T64, dict(B=1, H=4, W=4, Cin=128, Cout=256), 35),
    "vgg 256-512 2x2": ("vgg", T64, dict(B=2, H=2, W=2, Cin=256, Cout=512), 35),                             # M = 8
    "vgg 512-512 2x2": ("vgg", T64, dict(B=1, H=2, W=2, Cin=512, Cout=512), 35),                             # M = 4, K = 4608
    "vgg 512-512 1x1": ("vgg", T64, dict(B=3, H=1, W=1, Cin=512, Cout=512), 35),                             # M = 3: eight of nine taps are padding
    "gather 128-wide 16x16": ("gather", T128, dict(B=1, H=16, W=16, Cin=128, Cout=256), 36),
    "gather 128-wide 15x17": ("gather", T128, dict(B=1, H=15, W=17, Cin=64, Cout=256), 36),                 # H W = 255: the least that fills; M = 255
    "stem3x3<1> 16-32": ("stem3x3", "rn_conv3x3_kernel<1>", dict(B=3, H=7, W=7, Cin=16, Cout=32), 37),      # M = 147: a partial wave
    "stem3x3<1> 32-32 5x9": ("stem3x3", "rn_conv3x3_kernel<1>", dict(B=2, H=5, W=9, Cin=32, Cout=32), 37),
    "stem3x3<2> 16-64": ("stem3x3", "rn_conv3x3_kernel<2>", dict(B=3, H=7, W=7, Cin=16, Cout=64), 37),
    "stem3x3<2> 32-64 5x9": ("stem3x3", "rn_conv3x3_kernel<2>", dict(B=2, H=5, W=9, Cin=32, Cout=64), 37),
    "stem1 S64 C8": ("stem1", "rn_stem_conv1_kernel", dict(B=2, S=64, C1=8), 38),
    "stem1 S64 C32": ("stem1", "rn_stem_conv1_kernel", dict(B=2, S=64, C1=32), 38),
    "stem1 S96 C8": ("stem1", "rn_stem_conv1_kernel", dict(B=2, S=96, C1=8), 38),
    "stem1 S96 C32": ("stem1", "rn_stem_conv1_kernel", dict(B=2, S=96, C1=32), 38),
    "vgg1 S16": ("vgg1", "vgg_conv1_kernel", dict(B=3, S=16), 39),
    "avgpool 6x6 C64": ("avgpool", "rn_avgpool2_kernel", dict(B=2, H=6, W=6, C=64), 40),
    "avgpool 2x2 C8": ("avgpool", "rn_avgpool2_kernel", dict(B=2, H=2, W=2, C=8), 40),
    "tokens HW1 C128": ("tokens", "rn_attnpool_tokens_kernel", dict(B=2, HW=1, C=128), 41),
    "tokens HW9 C128": ("tokens", "rn_attnpool_tokens_kernel", dict(B=2, HW=9, C=128), 41),
    "tokens HW1 C264": ("tokens", "rn_attnpool_tokens_kernel", dict(B=2, HW=1, C=264), 41),                 # two workgroups, the second partial
    "tokens HW9 C264": ("tokens", "rn_attnpool_tokens_kernel", dict(B=2, HW=9, C=264), 41),
    # lattice runs: the device returns lattice_premise's bits
    "lattice 1x1 <64>": ("conv1x1", G64, dict(B=2, H=7, W=7, Cin=256, Cout=192, res=True, lattice=True), 50),
    "lattice 1x1 <128>": ("conv1x1", G128, dict(B=1, H=17, W=17, Cin=64, Cout=256, res=True, lattice=True), 50),
    "lattice 1x1 negative sum": ("conv1x1", G64, dict(B=2, H=7, W=7, Cin=64, Cout=64, res=True, lattice=True, negsum=True), 50),
    "lattice gather <64> 512-512 2x2": ("vgg", T64, dict(B=1, H=2, W=2, Cin=512, Cout=512, lattice=True), 51),      # K = 4608
    "lattice gather <64> 512-512 1x1": ("vgg", T64, dict(B=3, H=1, W=1, Cin=512, Cout=512, lattice=True), 51),
    "lattice gather <64> rn 5x9": ("gather", T64, dict(B=2, H=5, W=9, Cin=64, Cout=64, lattice=True), 51),
    "lattice gather <128> 15x17": ("gather", T128, dict(B=1, H=15, W=17, Cin=64, Cout=256, lattice=True), 51),
    "lattice stem3x3<1>": ("stem3x3", "rn_conv3x3_kernel<1>", dict(B=3, H=7, W=7, Cin=16, Cout=32, lattice=True), 52),
    "lattice stem3x3<2>": ("stem3x3", "rn_conv3x3_kernel<2>", dict(B=2, H=5, W=9, Cin=32, Cout=64, lattice=True), 52),
})
LATTICE_CASES = sorted(n for n, c in CASES.items() if c[2].get("lattice"))
