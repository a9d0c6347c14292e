"""Mirrors and float64 references of the kernels whose operands or outputs go through a packed-fp16 FIR chain (TEST INFRASTRUCTURE;
tests/test_fir_ops_ref.py, tests/test_gpu_fir_ops.py): upfir2_kernel<true> / <false>, conv_down_kernel, conv_down64_kernel, dblock0_kernel, the
two-kernel form conv_stream_kernel<fromrgb> + conv_down_kernel, conv_s2_kernel and conv_tiled<3,2,4,N,skip>.  Everything here is vectorised and
geometry-free: an image at a time, no tiles, no LDS.  tests/emu_ops.py and tests/emu_down64.py hold the same arithmetic at the kernels' index
level and take fir4 from here.  Nothing here is measured on the device.

TWO KINDS OF CHECK.
  bit-exact   LATTICE inputs (the lattice_* builders) make every MFMA accumulator a sum of multiples of one quantum q below 2^24 q: the fp32 result
              is exact in any summation order and equals the float64 sum.  Everything after the accumulator is a deterministic sequence of fp32
              and packed-fp16 operations that numpy reproduces: *_mirror() is the device's output bit for bit.  The builders assert their own
              premise (fp32 sums in two orders and the float64 sum are equal; sum |a b| < 2^24 q).
  bounded     RANDOM inputs: the fp16 operands of the LAST MFMA are mirrored bit for bit (FIR included), the rest is float64, and *_ref()
              returns (ref, tol) per element as tests/conv_ops_ref.py does: (2 K + 8) U32 P, one fp16 store, 2^-24.

CONTRACTION FORMS.  A packed-fp16 a * b + c compiles to v_pk_mul + v_pk_add (two roundings, form "sep") or to v_pk_fma (one, form "fma").  Which one
is the compiler's choice, so every mirror takes the form of each distinct site as an argument, and a device test passes when ONE combination of
forms holds for the whole output (FORMS / UP_FORMS).  As built (hipcc -O3 --offload-arch=gfx950; read from the disassembly of conv_down.hip,
conv_down64.hip, conv_d0.hip, upfir.hip; add : mul : fma = 2 : 1 : 1 per fir4) every site below is "fma":

  site                where                                   source                                                    as built
  fir4                conv_down.hip:59-61 (used :185-211)     (a + d) * 0.125h + (b + c) * 0.375h                       2 v_pk_add, v_pk_mul by 0x3000 (exact), v_pk_fma by 0x3600
                      conv_d0.hip:76-78 (P2 :279-282, P3 :363, P4 :380), conv_stream.hip:337-339 (<fromrgb> by-product)  the same
                      conv_down64.hip:57-61                   __builtin_elementwise_fma(b + c, k375, (a + d) * k125)    explicit: no choice
  up "h"              upfir.hip:415 / :523                    hs = (cv1 + cv2) * 3h + (cv0 + cv3)                       2 v_pk_add, v_pk_fma
  up "v"              upfir.hip:423 / :525                    (hs[r-3] + hs[r]) * 0.0625h + ((hs[r-2] + hs[r-1]) * 0.1875h + bn)   2 v_pk_add, 2 v_pk_fma (the outer
                                                                                                                        product by 1/16 is exact either way)

ROUNDINGS MIRRORED, in the order the kernels make them (h = fp16, f = fp32):
  conv_down / conv_down64 (FIR order "vh": vertical pass on the window column, then horizontal; conv_down.hip:171-211, conv_down64.hip step())
     weights h(f(w) coef) [glass_pack_conv]; skip weights h(f(ws16) * 0.70710678f) [conv_down.hip:162, conv_down64.hip:139]
     operand: fir4 down the zero-padded (pad 2) columns, fir4 along the rows                                     -> exact
     acc (MFMA, f) + b1 (f); max(v, 0.2f v) (f) [conv_down.hip:253-264]; skip MFMAs on top [:265-271]; h(acc) [:283]
  dblock0 (conv_d0.hip; FIR order "hv": P3 horizontal :354-363, P4 vertical :371-380; skip input P2 :259-282 pad 1, horizontal first, [::2])
     front: c = h(med3(y, -1, 1)) [:236-238]; Wrgb = h(rgb_w * sqrt2f), h(rgb_b * sqrt2f) [:119-122]; z = MFMA K = 4 (f); v = h(z) [:251];
            x = max(v, v * 0.2h) packed [:252]; conv0 acc starts at b0 [:297-305]; v = h(acc) [:343]; h = max(v * k1, v * k2) packed,
            k1 = h(sqrt2f), k2 = h(0.2f * sqrt2f) [:333-344]; zero outside the image [:292-295, :345]
     back:  acc starts at b1 [:387-393]; MFMAs; max(v, v * 0.2f) (f) [:418]; skip MFMAs with h(f(ws16) * 0.70710678f) [:139, :425]; h(acc) [:439 / :454]
  conv_stream<fromrgb> + conv_down (dblock0 impl 1): c = h(clamp((y + 1) / 2, 0, 1) * 2 - 1) [conv_stream.hip:243-244]; z = a chain of packed fp16
     fma fw0 * c0 + fw1 * c1 + fw2 * c2 + fw3 [:249] — NOT the fused kernel's fp32 MFMA rounded once: on random inputs the two x differ by an fp16
     ulp; on a lattice front both are exact.  v = h(acc * d + (nz + b0)) [:403]; h = max(v * k1, v * k2) [:345-346, :404]; the skip input is the
     by-product [:337-340] (horizontal first); then conv_down as above ("vh").
  conv_s2 / conv_tiled<3,2,4,N,skip>: no FIR inside (the input is the blurred map); what conv_ops_ref.py left out is the skip branch:
     conv_s2.hip:332   v = act_apply(acc + b, {sqrt2f s, 0.2f sqrt2f s}) + acc_skip * s; h(v)                      separate skip accumulators
     conv_tiled.hip:306-338, 410-423   acc = act_apply(acc + b, {sqrt2f, 0.2f sqrt2f}); skip MFMAs on top; h(acc * s)
  upfir2 (upfir.hip; <true> the grid instance :331-433, <false> the lean instance :434-537)
     operands <true>: x * sn16 packed [:196], shared weights; <false>: x, per-sample weights h(f(w16) * sn * d) [kernels_misc.hip modulate_weights_kernel]
     T = h(acc * d) [:379] (<false>: h(acc) [:480]); hs [:415 / :523]; bias8 = h(bias) [:355 / :491]; (half)nz, nz = f(strength * noise) [:268,
     :422 / :464, :524]; bn = bias8 + nz16; v [:423 / :525]; slope = h(0.2f), gain = h(sqrt2f * out_scale) [:391-392 / :495-496]; kps = ps16 * gain
     [:393 / :496]; out = max(v, v * slope) * kps [:425 / :526].  The window rows a segment's first step finds in LDS are never used for a stored row.

COUNTED BOUND OF upfir_ref (random inputs).  Exact float64 of the mirrored MFMA operands: t = acc d, the FIR, the epilogue.  Every fp16 rounding
contributes U16 |value rounded| (first order, times (1 + 16 U16) for the products of error terms), carried to the output through the FIR's positive
weights, the activation's largest slope (1: the gain is in kps) and |kps|.  The roundings, 16 per output with a consumer style, 15 without, the same
count for both instances: the T store (1); the horizontal pass: cv1 + cv2, cv0 + cv3, the fma (3); bias8, (half)nz, their sum (3); the vertical pass:
two sums, two fma (4); v * slope (1); the constants slope and gain (2); ps * gain (1, with post_scale only); the final product (1).  The MFMA term
(2 K + 8) U32 A |d| (K = 4 Cin: at most four taps feed one parity class) and the fp32 product strength * noise are carried the same way; 2^-24 for
outputs below 2^-14.  No term is fitted to an observed error."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

from glue_ops_ref import U16, U32, h16

f16, f32, f64 = np.float16, np.float32, np.float64
SQRT2F = f32(1.41421356237309504880)            # GLASS_SQRT2 (common.h)
SKIP_SCALE = f32(0.70710678118654752440)        # conv_down.hip:162
SUBNORMAL = 2.0 ** -24
FORMS = ("fma", "sep")
UP_FORMS = tuple(itertools.product(FORMS, FORMS))      # (site "h", site "v")


def _pack(w):
    from clip_glass_amd import ops
    return ops.host_pack_conv(np.asarray(w, f32))


def _fma16(a, k, c, form):
    """a * k + c on fp16 arrays, k a python float or array exact in fp16: one rounding ("fma") or the product rounded first ("sep")."""
    with np.errstate(invalid="ignore", over="ignore"):
        if form == "fma":
            return (a.astype(f64) * np.asarray(k, f64) + c.astype(f64)).astype(f16)     # exact in float64 (22 + 11 bits, exponents within 2^40), one rounding
        if form == "sep":
            return (a.astype(f32) * np.asarray(k, f32)).astype(f16) + c
    raise ValueError(form)


def fir4(a, b, c, d, form="fma"):
    """[1, 3, 3, 1] / 8 on fp16 arrays as the kernels' fir4(): (a + d) * 0.125 (the product is exact) + (b + c) * 0.375, contracted or not."""
    a, b, c, d = (np.asarray(v, f16) for v in (a, b, c, d))
    with np.errstate(invalid="ignore", over="ignore"):
        m = (a + d) * f16(0.125)
        s = b + c
    return _fma16(s, 0.375, m, form)


def _fir_pass(v, axis, form):
    n = v.shape[axis] - 3
    sl = [np.take(v, range(i, i + n), axis=axis) for i in range(4)]
    return fir4(sl[0], sl[1], sl[2], sl[3], form)


def blur_operand(h, order, form="fma", pad=2):
    """The zero-padded FIR of an fp16 map [B,R,R,C] as the kernels make their stride-2 operand: `order` "vh" (conv_down, conv_down64) or "hv"
    (conv_d0, conv_stream's by-product).  pad 2 -> [B,R+1,R+1,C]; pad 1 -> [B,R-1,R-1,C], of which the skip input is [:, ::2, ::2]."""
    v = np.pad(np.asarray(h).astype(f16), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    for ax in order:
        v = _fir_pass(v, {"v": 1, "h": 2}[ax], form)
    return v


def skip_input(x, form="fma"):
    """FIR pad 1 + [::2] of the block input, horizontal pass first (conv_d0.hip P2, conv_stream.hip:337-340)."""
    return blur_operand(x, "hv", form, pad=1)[:, ::2, ::2]


# ---- convolutions of mirrored operands (torch CPU) ----------------------------------------------------------------------------------------------
def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, f32).transpose(0, 3, 1, 2))).to(dtype)


def _conv(a, wp, stride, pad, dtype):
    """a [B,H,W,Cin], wp [T][Cout][Cin] (packed) -> [B,Ho,Wo,Cout] float64 array holding the sum in `dtype`."""
    KS = int(round(math.sqrt(wp.shape[0])))
    w = torch.as_tensor(np.ascontiguousarray(wp.reshape(KS, KS, wp.shape[1], wp.shape[2]).transpose(2, 3, 0, 1))).to(dtype)
    y = F.conv2d(_t(a, dtype), w, stride=stride, padding=pad)
    return np.ascontiguousarray(y.numpy().transpose(0, 2, 3, 1)).astype(f64)


def _upconv(a, wp, dtype):
    """t[2 m + k] += a[m] w[k] (upfir.hip:8): a [B,H,W,Cin], wp [9][Cout][Cin] shared or [B][9][Cout][Cin] per sample -> [B,2H+1,2W+1,Cout]."""
    B, H, W, Cin = a.shape
    if wp.ndim == 3:
        w = torch.as_tensor(np.ascontiguousarray(wp.reshape(3, 3, wp.shape[1], Cin).transpose(3, 2, 0, 1))).to(dtype)      # [Cin,Cout,3,3]
        y = F.conv_transpose2d(_t(a, dtype), w, stride=2)
    else:
        Cout = wp.shape[2]
        w = torch.as_tensor(np.ascontiguousarray(wp.reshape(B, 3, 3, Cout, Cin).transpose(0, 4, 3, 1, 2))).to(dtype).reshape(B * Cin, Cout, 3, 3)
        y = F.conv_transpose2d(_t(a, dtype).reshape(1, B * Cin, H, W), w, stride=2, groups=B).reshape(B, Cout, 2 * H + 1, 2 * W + 1)
    return np.ascontiguousarray(y.numpy().transpose(0, 2, 3, 1)).astype(f64)


def _abs_sum(fn, a, b, K, *args):
    """An upper bound of sum |a_k b_k|: summed in float32 and raised by that sum's own worst-case error (conv_ops_ref.conv_ref)."""
    return fn(np.abs(a), np.abs(b), *args, torch.float32) * (1 + 2 * K * U32)


# ---- the lattice premise ----------------------------------------------------------------------------------------------------------------------------
def quantum(a):
    """The largest power of two that divides every non-zero element of `a`."""
    v = np.abs(np.asarray(a, f64))
    v = v[v != 0]
    if not v.size:
        return 1.0
    m, e = np.frexp(v)
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mi & -mi).astype(f64))
    return 2.0 ** int((e - 53 + tz).min())


def assert_order_free(name, fn, a, b, *args, start=None):
    """The premise of a lattice MFMA stage, asserted: every product a_k b_k (and the starting value) is a multiple of q = quantum(a) quantum(b),
    sum |a_k b_k| + |start| < 2^24 q — so every partial sum in every order is exact in fp32 — and, as a check of the check, the fp32 sum in two
    channel orders and the float64 sum are equal.  Returns the sum (float64 array, exact)."""
    q = quantum(a) * quantum(b)
    s = 0.0 if start is None else np.asarray(start, f64)
    if start is not None and np.any(s != 0):
        q = min(q, quantum(s))
    A = fn(np.abs(a), np.abs(b), *args, torch.float64) + np.abs(s)
    assert A.max() < 2.0 ** 24 * q, "%s: sum |a b| reaches %.3g, the lattice holds below 2^24 q = %.3g" % (name, A.max(), 2.0 ** 24 * q)
    r64 = fn(a, b, *args, torch.float64) + s
    r32 = fn(a, b, *args, torch.float32) + s
    r32r = fn(np.ascontiguousarray(a[..., ::-1]), np.ascontiguousarray(b[..., ::-1]), *args, torch.float32) + s
    assert np.array_equal(r64, r32) and np.array_equal(r32, r32r), "%s: fp32 sums in two orders and the float64 sum differ" % name
    assert np.array_equal(r64, r64.astype(f32).astype(f64))
    return r64


def lattice_weights(rng, shape, values, fan_in):
    """w (reference layout, fp32) whose PACKED value fp16(fp32(w) * 1 / sqrt(fan_in)) is the drawn lattice value: w = fp32(k sqrt(fan_in)).
    Asserted through the library's own packer."""
    k = rng.choice(np.asarray(values, f64), size=shape)
    w = (k * math.sqrt(fan_in)).astype(f32)
    pk = _pack(w)                                                        # [T][Cout][Cin]
    KS = shape[2]
    want = k.transpose(2, 3, 0, 1).reshape(KS * KS, shape[0], shape[1])
    assert np.array_equal(pk.astype(f64), want), "lattice weights do not survive host_pack_conv"
    return w


def pow2(rng, shape, exps):
    """Signed powers of two."""
    return (rng.choice([-1.0, 1.0], size=shape) * 2.0 ** rng.choice(np.asarray(exps), size=shape)).astype(f32)


# ---- conv_down, conv_down64, conv_s2, conv_tiled<..,skip> --------------------------------------------------------------------------------------------
DOWN_KERNELS = ("conv_down", "conv_down64", "conv_s2", "conv_tiled_skip")


def down_operands(kernel, inp, form="fma"):
    """(a [B,R+1,R+1,Cin] the stride-2 conv's operand, w1 packed [9][Cout][Cin], wk [Cout][Cin] the skip weights as the MFMA sees them), float32
    arrays of fp16 values."""
    w1 = _pack(inp["w1"])
    ws = _pack(inp["ws"])[0]
    if kernel in ("conv_down", "conv_down64"):
        return blur_operand(inp["h"], "vh", form).astype(f32), w1, h16(ws * SKIP_SCALE)
    return np.asarray(inp["hb"], f32), w1, ws


def _down_consts(kernel, inp):
    """(activation gain in the accumulators, out_scale): conv_down folds sqrt2 / sqrt2 away."""
    if kernel in ("conv_down", "conv_down64"):
        return 1.0, 1.0
    return math.sqrt(2.0), float(f32(inp.get("out_scale", 2.0 ** -0.5)))


def down_ref(kernel, inp, form="fma"):
    """(ref, tol) [B,R/2,R/2,Cout] float64.  inp: h [B,R,R,Cin] (conv_down, conv_down64) or hb [B,R+1,R+1,Cin] (conv_s2, conv_tiled_skip), xs
    [B,R/2,R/2,Cin] the skip input as the kernel reads it, w1, ws, b1 in reference layout, out_scale."""
    a, w1, wk = down_operands(kernel, inp, form)
    xs = np.asarray(inp["xs"], f64)
    Cin = a.shape[3]
    K = 10 * Cin                                                         # nine taps and the skip stage
    acc = _conv(a, w1, 2, 0, torch.float64)
    A = _abs_sum(_conv, a, w1, K, 2, 0)
    sk = xs @ wk.astype(f64).T
    As = (np.abs(xs) @ np.abs(wk).astype(f64).T) * (1 + 2 * K * U32)
    b1 = np.asarray(inp["b1"], f64)
    g, s = _down_consts(kernel, inp)
    pre = acc + b1
    out = (np.where(pre > 0, pre, 0.2 * pre) * g + sk) * s
    tol = s * (2 * K + 8) * U32 * (g * (A + np.abs(b1)) + As) + U16 * np.abs(out) + SUBNORMAL
    return out, tol


def _down_finish(kernel, a, w1, wk, xs, b1, out_scale, dtype):
    """Accumulators summed in `dtype`, the epilogue as the kernel makes it in fp32, the fp16 store."""
    acc = _conv(a, w1, 2, 0, dtype).astype(f32)
    sk = (torch.as_tensor(np.asarray(xs, f32)).to(dtype) @ torch.as_tensor(wk).to(dtype).T).numpy()      # (float64 sums stay float64 up to the
    v = acc + np.asarray(b1, f32)                                                                          # store, as the emulators keep them)
    if kernel in ("conv_down", "conv_down64"):
        v = np.maximum(v, f32(0.2) * v)
        return h16(v.astype(sk.dtype) + sk)
    s = f32(out_scale)
    if kernel == "conv_s2":
        k1, k2 = SQRT2F * s, f32(0.2) * SQRT2F * s
        return h16((np.maximum(v * k1, v * k2)).astype(sk.dtype) + sk * s)
    k1, k2 = SQRT2F * f32(1), f32(0.2) * SQRT2F * f32(1)
    return h16(((np.maximum(v * k1, v * k2)).astype(sk.dtype) + sk) * s)


def down_mirror(kernel, inp, form="fma", dtype=torch.float64, a=None, wk=None):
    """The kernel's output with the accumulators summed in `dtype` and the epilogue as the kernel makes it, in fp32: on lattice inputs the device's
    bits (any dtype), on random inputs the emulators' arithmetic (float64 sums) or an fp32 emulation of a faithful kernel (float32 sums).  a / wk
    replace the operand / the skip weights (planted defects)."""
    a0, w1, wk0 = down_operands(kernel, inp, form)
    return _down_finish(kernel, a0 if a is None else a, w1, wk0 if wk is None else wk, inp["xs"], inp["b1"], inp.get("out_scale", 2.0 ** -0.5), dtype)


def down_inputs(B, R, Cin, Cout, seed=14):
    """Random inputs of ops.dblock_down as test_d_block_down_fused builds them (NHWC, fp16-rounded maps); xs is left to the caller."""
    from clip_glass_amd import synth
    r = lambda name, shape, std=1.0: synth.normal(seed, name, shape, std)
    nhwc = lambda t: np.ascontiguousarray(t.transpose(0, 2, 3, 1))
    return dict(h=h16(nhwc(r("h", (B, Cin, R, R)))), x=h16(nhwc(r("x", (B, Cin, R, R)))), w1=r("w1", (Cout, Cin, 3, 3)), b1=r("b1", (Cout,), 0.3),
                ws=r("ws", (Cout, Cin, 1, 1)))


def s2_inputs(B, R, Cin, Cout, seed=17):
    """test_gpu_ops._stride2_skip_case's inputs."""
    rng = np.random.default_rng(seed)
    return dict(hb=h16(rng.standard_normal((B, R + 1, R + 1, Cin))), xs=h16(rng.standard_normal((B, R // 2, R // 2, Cin))),
                w1=rng.standard_normal((Cout, Cin, 3, 3)).astype(f32), ws=rng.standard_normal((Cout, Cin, 1, 1)).astype(f32),
                b1=(rng.standard_normal(Cout) * 0.2).astype(f32), out_scale=2.0 ** -0.5)


def take_down(inp, idx):
    return {k: (v[np.asarray(idx)] if k in ("h", "x", "hb", "xs") else v) for k, v in inp.items()}


def lattice_down(B, R, Cin, Cout, seed=0):
    """conv_down / conv_down64 main branch on a lattice: h in multiples of 1/4 up to 1 (both FIR passes are then exact in either order and form:
    multiples of 2^-8 up to 1), packed weights in {0, +-1/4, +-1/2}, dyadic bias, wskip = 0 (the skip MFMAs add exact zeros; lrelu's 0.2f v
    is one deterministic fp32 product).  x is random: its FIR only meets zero weights."""
    rng = np.random.default_rng(7000 + 131 * seed + 17 * B + R + Cin)
    inp = dict(h=(rng.integers(-4, 5, (B, R, R, Cin)) / 4.0).astype(f32), x=h16(rng.standard_normal((B, R, R, Cin))),
               w1=lattice_weights(rng, (Cout, Cin, 3, 3), [0, 0.25, -0.25, 0.5, -0.5], 9 * Cin),
               ws=np.zeros((Cout, Cin, 1, 1), f32), b1=(rng.integers(-16, 17, Cout) / 16.0).astype(f32))
    ops_ = [blur_operand(inp["h"], o, fm) for o in ("vh", "hv") for fm in FORMS]
    assert all(np.array_equal(ops_[0], o) for o in ops_[1:]), "the FIR of the lattice map is not exact"
    assert quantum(ops_[0]) >= 2.0 ** -8
    assert_order_free("conv_down lattice", _conv, ops_[0].astype(f32), _pack(inp["w1"]), 2, 0)
    return inp


def lattice_down_skip(B, R, Cin, Cout, seed=0):
    """The SKIP branch of conv_down / conv_down64 on a lattice (the main-branch lattice has wskip = 0): h = 0 and b1 >= 0, so the activated
    accumulator is b1 itself; x in {-1, 0, 1}, whose pad-1 FIR [::2] is exact (multiples of 1/64: asserted, and the GPU test asserts that the
    device's launch_blur_down returns these bits); RANDOM skip weights of one binade (they pack to +-[1/4, 1/2) with all eleven bits, the MFMA sees
    h(ws16 * 0.70710678f) in +-[0.177, 0.354): multiples of 2^-13), so the products are multiples of 2^-19 and the sums of Cin of them stay exact,
    while any other rounding of the skip rows changes the output's bits."""
    rng = np.random.default_rng(8000 + 131 * seed + 17 * B + R + Cin)
    inp = dict(h=np.zeros((B, R, R, Cin), f32), x=rng.integers(-1, 2, (B, R, R, Cin)).astype(f32),
               w1=rng.standard_normal((Cout, Cin, 3, 3)).astype(f32), ws=(rng.choice([-1.0, 1.0], size=(Cout, Cin, 1, 1)) * rng.uniform(0.26, 0.49, (Cout, Cin, 1, 1)) * math.sqrt(Cin)).astype(f32),
               b1=(rng.integers(0, 33, Cout) / 16.0).astype(f32))
    xs = [skip_input(inp["x"], fm) for fm in FORMS] + [blur_operand(inp["x"], "vh", "fma", pad=1)[:, ::2, ::2]]
    assert all(np.array_equal(xs[0], v) for v in xs[1:]) and quantum(xs[0]) >= 2.0 ** -6, "the skip input of the lattice map is not exact"
    inp["xs"] = xs[0].astype(f32)
    wk = h16(_pack(inp["ws"])[0] * SKIP_SCALE)
    assert_order_free("conv_down skip lattice", _conv, inp["xs"], wk[None], 1, 0, start=inp["b1"].astype(f64))
    return inp


# ---- dblock0 ----------------------------------------------------------------------------------------------------------------------------------------
def _act16(v, k1, k2):
    """max(v * k1, v * k2) in packed fp16."""
    return np.maximum((v.astype(f32) * f32(k1)).astype(f16), (v.astype(f32) * f32(k2)).astype(f16))


def dblock0_front(inp, variant="fused", check=True):
    """(x, h) [B,R,R,32] fp16 of a LATTICE front: the fromRGB map and conv0's output as dblock0_kernel ("fused") or conv_stream_kernel<fromrgb>
    ("stream") form them.  With check the premise is asserted: both MFMA stages (fused) are order-free and exact."""
    y = np.asarray(inp["y"], f32)
    B, _, R, _ = y.shape
    yc = np.ascontiguousarray(y.transpose(0, 2, 3, 1))
    Cw = (np.asarray(inp["frgb_w"], f32) * SQRT2F).astype(f16)                                   # [32,3]
    Cb = (np.asarray(inp["frgb_b"], f32) * SQRT2F).astype(f16)
    if variant == "fused":
        c = np.clip(yc, f32(-1), f32(1)).astype(f16)
        wrgb = Cw.astype(f32)[None]                                                               # a 1 x 1 conv: [1][32][3]
        if check:
            z = assert_order_free("fromRGB", _conv, c.astype(f32), wrgb, 1, 0, start=Cb.astype(f64))
        else:
            z = _conv(c.astype(f32), wrgb, 1, 0, torch.float64) + Cb.astype(f64)
        v = z.astype(f32).astype(f16)
    elif variant == "stream":
        c = (np.minimum(np.maximum((yc + f32(1)) * f32(0.5), f32(0)), f32(1)) * f32(2) - f32(1)).astype(f16)
        zs = []
        for form in FORMS:                      # ((fw0 * c0 + fw1 * c1) + fw2 * c2) + fw3; exact on a lattice: the forms agree
            with np.errstate(invalid="ignore"):
                z = (Cw[:, 0].astype(f32) * c[..., 0:1].astype(f32)).astype(f16)
                for ch in (1, 2):
                    z = _fma16(np.broadcast_to(c[..., ch:ch + 1], z.shape), Cw[:, ch], z, form)
                zs.append(z + Cb)
        if check:
            assert np.array_equal(zs[0], zs[1]), "conv_stream<fromrgb>'s packed fma chain is not exact on this front"
        v = zs[0]
    else:
        raise ValueError(variant)
    x = np.maximum(v, (v.astype(f32) * f32(f16(0.2))).astype(f16))
    pk0 = _pack(inp["w0"])
    b0 = np.asarray(inp["b0"], f64)
    if check:
        acc = assert_order_free("conv0", _conv, x.astype(f32), pk0, 1, 1, start=b0)
    else:
        acc = _conv(x.astype(f32), pk0, 1, 1, torch.float64) + b0
    v = acc.astype(f32).astype(f16)
    h = _act16(v, f16(SQRT2F), f16(f32(0.2) * SQRT2F))
    return x, h


def dblock0_operands(inp, form="fma", variant="fused", front=None):
    """(a, xs, w1, wk): the stride-2 conv's operand and the skip input from the exact front (or from the maps `front` = (x, h)), the packed weights."""
    x, h = dblock0_front(inp, variant, check=False) if front is None else front
    a = blur_operand(h, "hv" if variant == "fused" else "vh", form)
    return a.astype(f32), skip_input(x, form).astype(f32), _pack(inp["w1"]), h16(_pack(inp["ws"])[0] * SKIP_SCALE)


def dblock0_ref(inp, form="fma", variant="fused", front=None):
    """(ref, tol) [B,R/2,R/2,64] float64 of ops.dblock0 on a lattice front: operands from dblock0_front, the rest as down_ref (K counts the nine
    taps, the skip stage and the accumulator's start at the bias)."""
    a, xs, w1, wk = dblock0_operands(inp, form, variant, front)
    K = 10 * 32 + 1
    acc = _conv(a, w1, 2, 0, torch.float64)
    A = _abs_sum(_conv, a, w1, K, 2, 0)
    sk = xs.astype(f64) @ wk.astype(f64).T
    As = (np.abs(xs).astype(f64) @ np.abs(wk).astype(f64).T) * (1 + 2 * K * U32)
    b1 = np.asarray(inp["b1"], f64)
    pre = acc + b1
    out = np.where(pre > 0, pre, 0.2 * pre) + sk
    return out, (2 * K + 8) * U32 * (A + np.abs(b1) + As) + U16 * np.abs(out) + SUBNORMAL


def dblock0_mirror(inp, form="fma", variant="fused", dtype=torch.float64, a=None, xs=None, wk=None):
    """As down_mirror: the emulator's arithmetic (float64 sums) or a faithful fp32 kernel (float32 sums) behind the exact front."""
    a0, xs0, w1, wk0 = dblock0_operands(inp, form, variant)
    a, xs, wk = (a0 if a is None else a), (xs0 if xs is None else xs), (wk0 if wk is None else wk)
    return _down_finish("conv_down", a, w1, wk, xs, inp["b1"], 1.0, dtype)


def dblock0_args(inp):
    return tuple(inp[k] for k in ("y", "frgb_w", "frgb_b", "w0", "b0", "w1", "ws", "b1"))


def lattice_dblock0(B, R, seed=0):
    """A lattice FRONT (y, fromRGB weights and bias, w0, b0) with random w1 / wskip / b1.  y in multiples of 1/4 with a few values outside
    [-1, 1] (the clamp); fromRGB rows and bias sqrt2-scale to {0, +-1/2} and multiples of 1/4: z is a multiple of 1/8 up to 2, the fromRGB map
    x = max(z, h(z * 0.2h)) holds multiples of 2^-16; w0 packs to {0, +-1/8} at half density."""
    rng = np.random.default_rng(9000 + 31 * seed + 7 * B + R)
    y = (rng.integers(-4, 5, (B, 3, R, R)) / 4.0).astype(f32)
    y[rng.random(y.shape) < 0.05] = 1.5
    y[rng.random(y.shape) < 0.05] = -1.25
    s2 = float(SQRT2F)
    inp = dict(y=y, frgb_w=(rng.choice([0.0, 0.5, -0.5], size=(32, 3)) / s2).astype(f32), frgb_b=(rng.integers(-2, 3, 32) / 4.0 / s2).astype(f32),
               w0=lattice_weights(rng, (32, 32, 3, 3), [0, 0, 0.125, -0.125], 9 * 32), b0=(rng.integers(-8, 9, 32) / 16.0).astype(f32))
    assert np.array_equal((inp["frgb_w"] * SQRT2F).astype(f16).astype(f64) * 2, np.round((inp["frgb_w"] * SQRT2F).astype(f64) * 2)), "fromRGB rows off the lattice"
    assert np.array_equal((inp["frgb_b"] * SQRT2F).astype(f16).astype(f64) * 4, np.round((inp["frgb_b"] * SQRT2F).astype(f64) * 4)), "fromRGB bias off the lattice"
    from clip_glass_amd import synth
    r = lambda name, shape, std=1.0: synth.normal(21 + seed, name, shape, std)
    inp.update(w1=r("w1", (64, 32, 3, 3)), b1=r("b1", (64,), 0.3), ws=r("ws", (64, 32, 1, 1)))
    xf, hf = dblock0_front(inp, "fused", check=True)
    xs_, hs_ = dblock0_front(inp, "stream", check=True)
    assert np.array_equal(xf, xs_) and np.array_equal(hf, hs_), "the two forms' fronts differ on the lattice"
    assert np.abs(hf.astype(f64)).max() > 0.5 and (xf < 0).mean() > 0.1
    return inp


def lattice_dblock0_skip(B, R, seed=0):
    """dblock0's SKIP branch on a lattice, as lattice_down_skip: y in {0, 1} and fromRGB rows that sqrt2-scale to {0, 1/2} without a bias make the
    fromRGB map x a multiple of 1/2 up to 3/2 (never negative: no 0.2h product), whose pad-1 FIR is exact; w0 = 0 and b0 = 0 make h = 0, b1 >= 0 is
    the activated accumulator; random skip weights of one binade.  P2's patch walk and the XS ring are then pinned to the last bit."""
    rng = np.random.default_rng(9500 + 31 * seed + 7 * B + R)
    s2 = float(SQRT2F)
    inp = dict(y=rng.integers(0, 2, (B, 3, R, R)).astype(f32), frgb_w=(rng.choice([0.0, 0.5], size=(32, 3)) / s2).astype(f32), frgb_b=np.zeros(32, f32),
               w0=np.zeros((32, 32, 3, 3), f32), b0=np.zeros(32, f32), w1=rng.standard_normal((64, 32, 3, 3)).astype(f32),
               ws=(rng.choice([-1.0, 1.0], size=(64, 32, 1, 1)) * rng.uniform(0.26, 0.49, (64, 32, 1, 1)) * math.sqrt(32)).astype(f32),
               b1=(rng.integers(0, 33, 64) / 16.0).astype(f32))
    x, h = dblock0_front(inp, "fused", check=True)
    xs_, hs_ = dblock0_front(inp, "stream", check=True)
    assert np.array_equal(x, xs_) and not h.any() and not hs_.any() and x.min() >= 0 and x.max() >= 1 and quantum(x) >= 0.5
    xs = [skip_input(x, fm) for fm in FORMS]
    assert np.array_equal(xs[0], xs[1]) and quantum(xs[0]) >= 2.0 ** -7, "the skip input of the lattice map is not exact"
    wk = h16(_pack(inp["ws"])[0] * SKIP_SCALE)
    assert_order_free("dblock0 skip lattice", _conv, xs[0].astype(f32), wk[None], 1, 0, start=inp["b1"].astype(f64))
    return inp


# ---- upfir2 -------------------------------------------------------------------------------------------------------------------------------------------
def up_operands(inp, lean):
    """(a [B,H,W,Cin], b [9][Cout][Cin] or [B][9][Cout][Cin], d [B,Cout] float32 or None): the MFMA operands and the demodulation left to apply."""
    x = np.asarray(inp["x"], f32)
    wk = _pack(inp["w"])
    sn, ds = inp.get("sn"), inp.get("dscale")
    if lean:
        B = x.shape[0]
        s = np.asarray(sn, f32)
        d = np.asarray(ds, f32) if ds is not None else np.ones((B, wk.shape[1]), f32)
        return x, h16((wk[None] * s[:, None, None, :]).astype(f32) * d[:, None, :, None]), None
    a = x if sn is None else h16(x * h16(sn)[:, None, None, :])
    return a, wk, (None if ds is None else np.asarray(ds, f32))


def _up_tables(inp):
    """bias8, nz16 [B,Ho,Wo,1], slope, kps [B,1,1,Cout] as fp16 arrays; act, gain."""
    x = inp["x"]
    B, H, W, _ = x.shape
    Cout = inp["w"].shape[0]
    act = bool(inp.get("act", True))
    bias8 = (np.zeros(Cout, f32) if inp.get("bias") is None else np.asarray(inp["bias"], f32)).astype(f16)
    if inp.get("noise") is None:
        nz32 = np.zeros((B, 2 * H, 2 * W, 1), f32)
    else:
        nz32 = (f32(inp.get("noise_strength", 0.0)) * np.repeat(np.asarray(inp["noise"], f32), inp.get("batch_size", 1), axis=0))[..., None]
    slope = f16(f32(0.2) if act else f32(1))
    gain = f16((SQRT2F if act else f32(1)) * f32(inp.get("out_scale", 1.0)))
    if inp.get("post_scale") is None:
        kps = np.full((B, 1, 1, Cout), gain, f16)
    else:
        kps = (np.asarray(inp["post_scale"], f32).astype(f16).astype(f32) * f32(gain)).astype(f16)[:, None, None, :]
    return bias8, nz32, slope, kps, act, gain


def up_T(inp, lean, dtype=torch.float64, defect=None):
    """The T values h(acc * d) (<false>: h(acc)) of every image, zero-padded by one: [B,2H+3,2W+3,Cout] fp16 (index i + 1 holds t[i], upfir.hip:34)."""
    a, b, d = up_operands(inp, lean)
    acc = _upconv(a, b, dtype).astype(f32)
    if d is not None:
        dd = np.broadcast_to(d[:, None, None, :], acc.shape)
        if defect is not None and defect[0] == "dscale_group":                 # one 8-channel group of one 16 x 30 piece with another candidate's table row
            _, b_, other, ch = defect
            dd = dd.copy()
            dd[b_, 0:16, 0:30, ch:ch + 8] = d[other, ch:ch + 8]
        acc = acc * dd
    return np.pad(acc.astype(f16), ((0, 0), (1, 1), (1, 1), (0, 0)))


def up_chain(T, inp, form=("fma", "fma"), defect=None):
    """upfir.hip:379-425 / :480-533 from the T tile on, as array operations on whole images: horizontal pass, bias + noise, vertical pass,
    activation, gain * consumer style.  form = (site "h", site "v").  defect: a planted fault (test_fir_ops_ref.py)."""
    fh, fv = form
    bias8, nz32, slope, kps, act, gain = _up_tables(inp)
    B, Hp, Wp, Cout = T.shape
    Ho, Wo = Hp - 3, Wp - 3
    with np.errstate(invalid="ignore", over="ignore"):
        cv = [T[:, :, j:j + Wo] for j in range(4)]
        hs = _fma16(cv[1] + cv[2], 3.0, cv[0] + cv[3], fh)                      # [B,2H+3,Wo,Cout]: 4 x the filtered row
        if defect is not None and defect[0] == "stale_hs":                     # one window row kept from the rows 16 further up
            _, b_, row = defect
            hs = hs.copy()
            hs[b_, row] = hs[b_, row - 16]
        rows = [hs[:, j:j + Ho] for j in range(4)]
        if defect is not None and defect[0] == "noise_plane":
            nz32 = nz32.copy()
            nz32[defect[1]] = nz32[defect[2]]
        bn = bias8 + nz32.astype(f16)
        inner = _fma16(rows[1] + rows[2], 0.1875, bn, fv)
        v = _fma16(rows[0] + rows[3], 0.0625, inner, fv)
        o = np.maximum(v, (v.astype(f32) * f32(slope)).astype(f16))
        if defect is not None and defect[0] == "kps_row":                       # another image row's consumer style
            kps = np.broadcast_to(kps, (B, 1, 1, Cout)).copy()
            kps[defect[1]] = kps[defect[2]]
        return (o.astype(f32) * kps.astype(f32)).astype(f16).astype(f32)


def upfir_mirror(inp, lean, form=("fma", "fma"), dtype=torch.float64, defect=None):
    """The up-conv's output [B,2H,2W,Cout]: the device's bits on lattice inputs (the accumulators are exact, the rest is deterministic), the emulator's
    arithmetic on random ones."""
    return up_chain(up_T(inp, lean, dtype, defect), inp, form, defect)


def upfir_ref(inp, lean):
    """(ref, tol) [B,2H,2W,Cout] float64 for random inputs: see COUNTED BOUND in the module docstring."""
    a, b, d = up_operands(inp, lean)
    Cin = a.shape[3]
    K = 4 * Cin
    dd = 1.0 if d is None else d.astype(f64)[:, None, None, :]
    t = np.pad(_upconv(a, b, torch.float64) * dd, ((0, 0), (1, 1), (1, 1), (0, 0)))
    eT = np.pad(_abs_sum(_upconv, a, b, K) * np.abs(dd), ((0, 0), (1, 1), (1, 1), (0, 0))) * (2 * K + 8) * U32 + U16 * np.abs(t)
    bias8, nz32, slope, kps16, act, gain = _up_tables(inp)
    B, Hp, Wp, Cout = t.shape
    Ho, Wo = Hp - 3, Wp - 3
    c = [t[:, :, j:j + Wo] for j in range(4)]
    e = [eT[:, :, j:j + Wo] for j in range(4)]
    s, q = c[1] + c[2], c[0] + c[3]
    hs = 3 * s + q
    ehs = 3 * (e[1] + e[2]) + e[0] + e[3] + U16 * (3 * np.abs(s) + np.abs(q) + np.abs(hs))
    r = [hs[:, j:j + Ho] for j in range(4)]
    er = [ehs[:, j:j + Ho] for j in range(4)]
    bias = np.zeros(Cout) if inp.get("bias") is None else np.asarray(inp["bias"], f64)
    if inp.get("noise") is None:
        nz = np.zeros((B, Ho, Wo, 1))
    else:
        nz = (float(f32(inp.get("noise_strength", 0.0))) * np.repeat(np.asarray(inp["noise"], f64), inp.get("batch_size", 1), axis=0))[..., None]
    bn = bias + nz
    ebn = U16 * (np.abs(bias) + np.abs(nz) + np.abs(bn)) + U32 * np.abs(nz)
    av, mv = r[0] + r[3], r[1] + r[2]
    inner = mv * 0.1875 + bn
    v = av * 0.0625 + inner
    ev = (er[0] + er[3]) * 0.0625 + (er[1] + er[2]) * 0.1875 + ebn + U16 * (np.abs(av) * 0.0625 + np.abs(mv) * 0.1875 + np.abs(inner) + np.abs(v))
    sl = 0.2 if act else 1.0
    o = np.maximum(v, sl * v) if act else v
    eo = ev + (2 * U16 * sl * np.abs(v) if act else 0.0)                 # the constant slope = h(0.2f) and the product v * slope
    g = (math.sqrt(2.0) if act else 1.0) * float(f32(inp.get("out_scale", 1.0)))
    has_ps = inp.get("post_scale") is not None
    ps = h16(inp["post_scale"]).astype(f64)[:, None, None, :] if has_ps else 1.0
    out = o * g * ps
    tol = (np.abs(g * ps) * eo + (3 if has_ps else 2) * U16 * np.abs(out)) * (1 + 16 * U16) + SUBNORMAL      # gain, (ps * gain), the final product
    return out, tol


def up_inputs(seed, B, H, Cin, Cout, batch_size=1, L=24, post_scale=False):
    """One modulated up-conv layer as test_gpu_ops._modconv_case (seed 3) / test_gpu_conv_engine_forms._layer (seed 51) build it, NHWC."""
    from clip_glass_amd import synth
    from util import style_tables
    r = lambda name, shape, std=1.0: synth.normal(seed, name, shape, std)
    x = h16(np.ascontiguousarray(r("x", (B, Cin, H, H)).transpose(0, 2, 3, 1)))
    w = r("w", (Cout, Cin, 3, 3)); lat = r("lat", (B, L)); A = r("A", (Cin, L)); Ab = r("Ab", (Cin,), 0.2) + 1
    bias = r("b", (Cout,), 0.3)
    noise = r("noise", (B // batch_size, 2 * H, 2 * H))
    sn, _, ds = style_tables(lat, A, Ab, w, demod=True)
    inp = dict(x=x, w=w, sn=sn, dscale=ds, noise=noise, noise_strength=0.37, batch_size=batch_size, bias=bias, act=True, out_scale=1.0)
    if post_scale:
        inp["post_scale"] = (np.abs(r("ps", (B, Cout))) + 0.5).astype(f32)
    return inp


def lattice_up(B, H, Cin, Cout, batch_size=1, post_scale=False, seed=0):
    """An up-conv launch whose accumulators are exact: x in multiples of 1/16 up to 1 (T then holds sums of 12 and more bits: its fp16 store and
    every FIR stage round, deterministically), packed weights in {0, +-1/4, +-1/2}, styles, demodulation and
    consumer styles signed powers of two that differ between candidates, dyadic noise planes per minibatch with a power-of-two strength, dyadic bias."""
    assert B % batch_size == 0
    rng = np.random.default_rng(5000 + 977 * seed + 131 * B + 17 * H + Cin + Cout)
    inp = dict(x=(rng.integers(-16, 17, (B, H, H, Cin)) / 16.0).astype(f32), w=lattice_weights(rng, (Cout, Cin, 3, 3), [0, 0.25, -0.25, 0.5, -0.5], 9 * Cin),
               sn=pow2(rng, (B, Cin), [-2, -1, 0]), dscale=pow2(rng, (B, Cout), [-3, -2, -1]),
               noise=(rng.integers(-16, 17, (B // batch_size, 2 * H, 2 * H)) / 8.0).astype(f32), noise_strength=0.5, batch_size=batch_size,
               bias=(rng.integers(-8, 9, Cout) / 16.0).astype(f32), act=True, out_scale=1.0)
    if post_scale:
        inp["post_scale"] = pow2(rng, (B, Cout), [-1, 0, 1])
    for k in ("sn", "dscale", "post_scale"):
        if k in inp and B > 1:
            assert all(not np.array_equal(inp[k][i], inp[k][j]) for i in range(B) for j in range(i)), "candidates share their " + k
    nb = inp["noise"].shape[0]
    assert all(not np.array_equal(inp["noise"][i], inp["noise"][j]) for i in range(nb) for j in range(i)), "minibatches share a noise plane"
    for lean in (False, True):
        a, b, d = up_operands(inp, lean)
        assert_order_free("up-conv lattice lean=%d" % lean, _upconv, a, b)
    return inp


def up_kwargs(inp, premod=False):
    """Keyword arguments of ops.conv for an up-conv `inp` (without x, w)."""
    kw = {k: inp[k] for k in ("sn", "dscale", "noise", "noise_strength", "batch_size", "bias", "act", "out_scale", "post_scale") if inp.get(k) is not None}
    kw.update(up=True, impl=3)
    if premod:
        kw.update(premod=True)
    return kw


def take_up(inp, idx):
    idx = np.asarray(idx)
    out = dict(inp, batch_size=1)
    for k in ("x", "sn", "dscale", "post_scale"):
        if inp.get(k) is not None:
            out[k] = inp[k][idx]
    if inp.get("noise") is not None:
        out["noise"] = inp["noise"][idx // inp["batch_size"]]
    return out


# ---- one form for the whole output --------------------------------------------------------------------------------------------------------------------
def bound_ratio(got, ref, tol):
    """Worst err / tol over the whole output (inf where got is not finite)."""
    got = np.asarray(got, f64)
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    return float((err / tol).max())


# ---- the cases tests/test_gpu_fir_ops.py runs on the device and tests/test_fir_ops_ref.py runs through the fp32 emulation -------------------------------
# up-conv: (B, H, Cin, Cout, batch_size, post_scale)
UP_GRID_CASES = [(5, 8, 32, 32, 1, False), (5, 8, 32, 32, 1, True), (9, 32, 32, 32, 3, False), (20, 16, 32, 96, 1, False), (70, 16, 32, 32, 2, False),
                 (26, 8, 64, 96, 2, False), (3, 64, 96, 64, 1, False), (3, 64, 96, 64, 1, True)]
UP_LEAN_CASES = [(B, H, Ci, Co, bs, ps) for (B, H, Ci, Co, bs) in [(2, 16, 32, 32, 2), (3, 40, 32, 96, 1), (4, 64, 64, 64, 2)] for ps in (False, True)]
# conv_down / conv_down64: (kernel, B, R, Cin, Cout)
DOWN_LATTICE_CASES = [("conv_down", 2, 64, 32, 64), ("conv_down", 1, 128, 32, 64), ("conv_down64", 2, 64, 64, 128), ("conv_down64", 1, 116, 64, 128)]
DOWN_CASES = [("conv_down", 2, 64, 32, 64), ("conv_down", 1, 128, 32, 64), ("conv_down", 3, 192, 32, 64),
              ("conv_down64", 2, 64, 64, 128), ("conv_down64", 1, 116, 64, 128), ("conv_down64", 3, 192, 64, 128)]
S2_CASES = [("conv_s2", 2, 64, 64, 128), ("conv_s2", 1, 64, 32, 256), ("conv_s2", 37, 64, 96, 384), ("conv_tiled_skip", 3, 64, 32, 64), ("conv_tiled_skip", 2, 64, 64, 128)]
D0_CASES = [(1, 64), (2, 68), (3, 192)]
D0_TWO_KERNEL_CASE = (1, 192)


def three(B):
    """First, middle, last candidate: the reference of a launch too large for a float64 pass over all of it."""
    return sorted({0, B // 2, B - 1})
