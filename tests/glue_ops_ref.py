"""float64 references of the StyleGAN2 glue kernels (csrc/kernels_misc.hip: toRGB + skip, the two FIR blurs, fromRGB), their error bounds,
and the inputs the CPU and the GPU tests share (TEST INFRASTRUCTURE; tests/test_glue_ops_ref.py, tests/test_gpu_glue_ops.py).

Each reference returns (ref, A): A is the same expression with the absolute value taken of every term, i.e. the sum of the magnitudes the
device adds up.  The bars come from the summation bound |fl(sum) - sum| <= n u sum|terms| with u = 2^-24, which holds for any order of the
additions and with or without FMA; an fp16 output adds one rounding, 2^-11 |ref| (and 2^-24 absolute for the subnormal range).  n counts
the roundings along the longest chain of an output element:
  toRGB    C products and additions of the dot product, two roundings of the modulated weight (wrgb * (sn * smax)), the bias, the four skip
           taps with their weight products and the two closing additions: C + 16 covers them.
  blur     16 taps, each through two products and two sums of four: 32 covers them.
  fromRGB  three products and four additions, the rounding of v = clip((y + 1) / 2) * 2 - 1 itself (the "+ 1" next to |v| in A), the slope
           and the sqrt 2 gain: 16 covers them; sqrt 2 carries A through the activation.
Nothing here is measured on the device."""
import math

import numpy as np

from util import _torgb_ref

U32 = 2.0 ** -24       # unit roundoff of float32
U16 = 2.0 ** -11       # of fp16
FIR = np.array([1.0, 3.0, 3.0, 1.0]) / 8


def h16(a):
    """Round to fp16 as the device does for activations."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ---- references -----------------------------------------------------------------------------------------------------------------------
def torgb(x16, wrgb, bias, sn, smax, yprev):
    """x16 [B,H,H,C] NHWC, wrgb [3,C] (scaled by 1/sqrt C), bias [3], sn [B,C], smax [B], yprev [B,3,H/2,H/2] or None -> [B,3,H,H]."""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    args = [f64(a) for a in (x16, wrgb, bias, sn, smax, yprev)]
    return _torgb_ref(*args), _torgb_ref(*[None if a is None else np.abs(a) for a in args])


def _fir_sep(x, pad, stride):
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C))
    xp[:, pad:pad + H, pad:pad + W] = x
    Ho, Wo = (H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1
    rows = sum(FIR[j] * xp[:, :, j:j + (Wo - 1) * stride + 1:stride] for j in range(4))            # along W
    return sum(FIR[j] * rows[:, j:j + (Ho - 1) * stride + 1:stride] for j in range(4))             # along H


def blur(x16, pad, stride):
    """Separable [1,3,3,1]/8 FIR of an NHWC map with zero padding `pad` on all four sides: pad 2, stride 1 -> (H+1)^2; pad 1, stride 2 -> (H/2)^2."""
    x = np.asarray(x16, np.float64)
    return _fir_sep(x, pad, stride), _fir_sep(np.abs(x), pad, stride)


def fromrgb(y, w, bias):
    """y [B,3,R,R] NCHW, w [Cout,3] (scaled by 1/sqrt 3), bias [Cout] -> [B,R,R,Cout] NHWC: denorm clamp, 1x1 conv, bias, lrelu(0.2) * sqrt 2."""
    y, w, bias = (np.asarray(a, np.float64) for a in (y, w, bias))
    v = np.clip((y + 1) / 2, 0, 1) * 2 - 1
    t = np.einsum("bchw,oc->bhwo", v, w) + bias
    A = np.einsum("bchw,oc->bhwo", np.abs(v) + 1, np.abs(w)) + np.abs(bias)
    return np.where(t > 0, t, 0.2 * t) * math.sqrt(2), A


# ---- bars (elementwise arrays) ---------------------------------------------------------------------------------------------------------
def tol_torgb(C, A):
    return (C + 16) * U32 * A


def tol_blur(ref, A):
    return U16 * np.abs(ref) + U32 + 32 * U32 * A


def tol_fromrgb(ref, A):
    return U16 * np.abs(ref) + U32 + 16 * U32 * math.sqrt(2) * A


# ---- cases and inputs -------------------------------------------------------------------------------------------------------------------
TORGB_C = (16, 32, 64, 128, 256, 512)       # torgb_pix_kernel<16|32|64>, torgb_kernel<16|32|64>
TORGB_H = (4, 20)                           # the first layer (16 pixels in 32 .. 256 pixel slots); hw = 400: a tail in every instance
BLUR_PAD2 = ((4, 8), (16, 24), (17, 64), (33, 512))          # (H, C): cg = 1; cg no power of two; a second strip of 1 / 2 rows; odd H
BLUR_PLANAR_C = (32, 128, 256, 512)                          # cg < 32: groups fastest; cg >= 32: re-dealt (P = 8, 4)
BLUR_PLANAR_H = (4, 16)                                      # Wo = 17: the last workgroup of the re-dealt form holds one live column
BLUR_DOWN = ((4, 8), (8, 24), (34, 64), (16, 512))           # Ho = 17: three 8-row strips, the last with one row
FROMRGB_COUT = (8, 32, 64, 128)
FROMRGB_R = (4, 10, 16, 18)                 # hw = 16: a partial wave; 100: + two waves behind the image; 256: exact; 324: a partial workgroup


def torgb_inputs(C, H, with_skip, B=3):
    """Features, weights and the skip image of the same magnitude (O(1)); smax differs per sample by design (0.6 / 1.0 / 1.7 x)."""
    rng = np.random.default_rng(1000 * C + 10 * H + int(with_skip))
    x = h16(rng.standard_normal((B, H, H, C)))
    wrgb = (rng.standard_normal((3, C)) / math.sqrt(C)).astype(np.float32)
    bias = (0.3 * rng.standard_normal(3)).astype(np.float32)
    s = (1 + 0.5 * rng.standard_normal((B, C))) * np.array([0.6, 1.0, 1.7])[:B, None]
    smax = np.abs(s).max(axis=1)
    sn = (s / smax[:, None]).astype(np.float32)
    smax = smax.astype(np.float32)
    yprev = rng.standard_normal((B, 3, H // 2, H // 2)).astype(np.float32) if with_skip else None
    return x, wrgb, bias, sn, smax, yprev


def blur_inputs(H, C, B=2):
    return h16(np.random.default_rng(77 * H + C).standard_normal((B, H, H, C)))


def fromrgb_inputs(Cout, R, B=2):
    """Images that leave [-1, 1] (std 0.8, and +-1.5 planted) and hold exactly -1, 1 and 0."""
    rng = np.random.default_rng(500 * Cout + R)
    y = (0.8 * rng.standard_normal((B, 3, R, R))).astype(np.float32)
    flat = y.reshape(-1)
    flat[[0, 1, 2, 3, 4, flat.size - 1, flat.size - 2]] = [-1.0, 1.0, 1.5, -1.5, 0.0, 1.5, -1.0]
    w = (rng.standard_normal((Cout, 3)) / math.sqrt(3)).astype(np.float32)
    bias = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
    return y, w, bias
