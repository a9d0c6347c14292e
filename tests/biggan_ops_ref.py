"""Float64 restatements of the BigGAN-deep path's device operations, one per kernel family (test infrastructure).

tests/test_gpu_biggan_ops.py compares each HIP kernel with the function of the same name here; tests/test_biggan_ops_ref.py composes
these functions into a GenBlock, the self-attention block and the generator tail and pins them to oracle/biggan_ref.py on the CPU, so
the GPU tests do not test the kernels against a private opinion.  Activations are NHWC numpy float64; nothing here rounds unless a
`round_*` argument asks for a rounding the device declares (csrc/common.h ConvParams).
"""
import numpy as np
import torch
import torch.nn.functional as F


def f64(a):
    return np.asarray(a, dtype=np.float64)


def h16(a):
    """Round to fp16 (round to nearest even, overflow to inf) and return float64."""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def softmax(s):
    """Row softmax over the last axis."""
    s = f64(s)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def cond(x, emb, zd):
    """latent.py:20-24 + BigGAN.forward: rows x = [z (zd) | class bits (nc)], emb = embeddings.weight [zd, nc] ->
    [clip(z, -2, 2) | softmax(class bits) @ emb^T]  [P, 2 zd]."""
    x, emb = f64(x), f64(emb)
    nc = emb.shape[1]
    return np.concatenate([np.clip(x[:, :zd], -2.0, 2.0), softmax(x[:, zd:zd + nc]) @ emb.T], axis=1)


def bn_affine(cnd, w_scale, w_offset, mean, var, eps, prebias=None):
    """BigGANBatchNorm folded to y = x A + S for an input x = conv + prebias:
    A = (1 + scale . cond) / sqrt(var + eps),  S = offset . cond + (prebias - mean) A.   cnd [P, cd], w_* [C, cd] -> A, S [P, C]."""
    cnd, mean, var = f64(cnd), f64(mean), f64(var)
    pb = 0.0 if prebias is None else f64(prebias)
    A = (1.0 + cnd @ f64(w_scale).T) / np.sqrt(var + eps)
    return A, cnd @ f64(w_offset).T + (pb - mean) * A


def bn_tables(cnd, wt, bias, inv_std, mean, prebias):
    """The same affine from the engine's table operands (glass_biggan_prepare): wt [cd, 2C] = (gain | offset) columns, bias [2C]
    (1 in the gain columns of a conditional norm) -> tab [P, 2C] = [A | S]."""
    lin = f64(cnd) @ f64(wt) + f64(bias)
    C = f64(inv_std).shape[0]
    A = lin[:, :C] * f64(inv_std)
    return np.concatenate([A, lin[:, C:] + (f64(prebias) - f64(mean)) * A], axis=1)


def up2(x):
    """Nearest x2 of an NHWC map."""
    return np.repeat(np.repeat(f64(x), 2, axis=1), 2, axis=2)


def pre_bn_relu(x, A, S, rounding=None):
    """relu(x A + S) per (sample, channel) on every pixel of the map (the conv's zero padding comes AFTER it).
    rounding None: exact.  "f16": the tables rounded to fp16 and the fused multiply-add rounded to fp16 once (conv_tiled's packed
    fp16 staging).  "f32": fp32 tables, the result rounded to fp16 once (conv_direct / conv_gemm's staging)."""
    x, A, S = f64(x), f64(A)[:, None, None, :], f64(S)[:, None, None, :]
    if rounding == "f16":
        return np.maximum(h16(x * h16(A) + h16(S)), 0.0)
    v = np.maximum(x * A + S, 0.0)
    return h16(v) if rounding == "f32" else v


def conv(x, w, pre=None, in_up=False, dscale=None, bias=None, shift=None, relu=False, res=None, res_up=False, pre_rounding=None):
    """One convolution of the BigGAN path (biggan.cpp bg_conv).  x [B,h,w,Cin] (the STORED map: half-size with in_up), w [Cout,Cin,KS,KS]
    (pad KS // 2):  xin = nearest_x2?(relu(x A + S)?)  ->  v = conv(xin) * dscale + bias + shift  ->  relu?  ->  + nearest_x2?(res)[..., :Cout].
    pre = (A, S) [B,Cin]; dscale / shift [B,Cout]; res [B,Ho >> res_up,Wo >> res_up,>= Cout] (channel-drop skip)."""
    x, w = f64(x), f64(w)
    if pre is not None:
        x = pre_bn_relu(x, pre[0], pre[1], pre_rounding)
    if in_up:
        x = up2(x)
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))), torch.from_numpy(np.ascontiguousarray(w)),
                 padding=w.shape[2] // 2).numpy().transpose(0, 2, 3, 1)
    if dscale is not None:
        y = y * f64(dscale)[:, None, None, :]
    if bias is not None:
        y = y + f64(bias)
    if shift is not None:
        y = y + f64(shift)[:, None, None, :]
    if relu:
        y = np.maximum(y, 0.0)
    if res is not None:
        r = up2(res) if res_up else f64(res)
        y = y + r[..., :w.shape[0]]
    return np.ascontiguousarray(y)


def attn_split(T, c8, c2):
    """T [B,H,W,c8 + c8 + c2] (theta | phi | g) -> theta [B,HW,c8], phi [B,HW/4,c8] (2x2 max-pool), gT [B,c2,HW/4] (2x2 max-pool, transposed)."""
    T = f64(T)
    B, H, W, _ = T.shape
    pool = lambda a: a.reshape(B, H // 2, 2, W // 2, 2, a.shape[-1]).max(axis=(2, 4)).reshape(B, H * W // 4, a.shape[-1])
    theta = T[..., :c8].reshape(B, H * W, c8)
    return theta, pool(T[..., c8:2 * c8]), np.ascontiguousarray(pool(T[..., 2 * c8:]).transpose(0, 2, 1))


def rgb_tanh(x):
    """x [B,hw,C] -> [B,3,hw] = tanh of channels 0..2."""
    return np.tanh(f64(x)[..., :3]).transpose(0, 2, 1)


def gen_block(x, w, b3, tabs, up):
    """A GenBlock as the engine runs it: four convs, every norm folded into one of them.  x [B,r,r,cin]; w: the four conv weights;
    tabs: [(A_k, S_k)] of bn_0 .. bn_3 (S_1 .. S_3 carry the bias of the conv before them); b3: conv_3's bias.
    Returns (out, h) — h is conv_2's output, the input of conv_3 (and of the fused tail)."""
    t = conv(x, w[0], pre=tabs[0], dscale=tabs[1][0], shift=tabs[1][1], relu=True)
    t = conv(t, w[1], in_up=up, dscale=tabs[2][0], shift=tabs[2][1], relu=True)
    h = conv(t, w[2], dscale=tabs[3][0], shift=tabs[3][1], relu=True)
    return conv(h, w[3], bias=b3, res=x, res_up=up), h


def self_attn(x, w_theta, w_phi, w_g, w_o, gamma):
    """The self-attention block as the engine runs it: one 1x1 conv for theta | phi | g, split + pool, logits, softmax, values, and the
    output conv with gamma folded into its weights and x as the residual.  x [B,H,W,C]; w_* [Cout,C,1,1]."""
    c8, c2 = w_theta.shape[0], w_g.shape[0]
    T = conv(x, np.concatenate([f64(w_theta), f64(w_phi), f64(w_g)], axis=0))
    theta, phi, gT = attn_split(T, c8, c2)
    P = softmax(theta @ phi.transpose(0, 2, 1))                    # [B,HW,HW/4]
    O = (P @ gT.transpose(0, 2, 1)).reshape(x.shape[0], x.shape[1], x.shape[2], c2)
    return conv(O, f64(w_o) * float(gamma), res=x)


def final(x, A, S, rgb_w, rgb_b):
    """tanh(conv_to_rgb(relu(x A + S))[:3]) -> [B,3,H,W].  A, S [C] (the generator's last norm is unconditional)."""
    B = x.shape[0]
    y = conv(x, f64(rgb_w)[:3], pre=(np.tile(f64(A), (B, 1)), np.tile(f64(S), (B, 1))), bias=f64(rgb_b)[:3])
    return np.tanh(y).transpose(0, 3, 1, 2)


def tail(h, x0, w3, b3, A, S, rgb_w, rgb_b):
    """The last up block's conv_3 + skip, then `final` (bg_tail.hip): h [B,R,R,mid], x0 [B,R/2,R/2,cin], w3 [cout,mid(,1,1)]."""
    w3 = f64(w3).reshape(f64(w3).shape[0], -1, 1, 1)
    return final(conv(h, w3, bias=b3, res=x0, res_up=True), A, S, rgb_w, rgb_b)


# ---- counted bounds, mirrored operands and lattice inputs: bg_tail and the batched GEMMs (tests/test_biggan_bounds_ref.py, test_gpu_biggan_ops.py) ----
# Nothing below is measured on the device.  U16 / U32: the unit roundoffs of fp16 / fp32; SUB16: the rounding unit of an fp16 value below 2^-14.
U16, U32, SUB16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -24
f32 = np.float32


def r32(a):
    return np.asarray(a, np.float64).astype(f32).astype(np.float64)


def sum_odd(a, b):
    """a + b in float64 ROUNDED TO ODD: where the float64 sum is inexact (two-sum residual non-zero) and its last bit is even, the neighbour on
    the residual's side.  Rounding the result to fp32 or fp16 then gives the correctly rounded exact sum — the double rounding is not assumed
    away.  Returns (sum, the number of elements whose float64 sum was inexact)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    return np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s), int((e != 0).sum())


def fma32(a, b, c, form):
    """fp32 a b + c of fp32 values: "fma" one rounding, "sep" two.  The product of two fp32 values is exact in float64."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    return r32(sum_odd(p if form == "fma" else r32(p), c)[0])


def fma16(a, b, c, form):
    """Packed fp16 a b + c of fp16 values, the same two forms."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    return h16(sum_odd(p if form == "fma" else h16(p), c)[0])


def tanh_term(s):
    """_f32_bar's rule for a tanh of fp32 arguments: 4 x the largest error of numpy's float32 tanh against float64 on the same arguments."""
    s = np.asarray(s, np.float64).astype(f32)
    return 4.0 * float(np.abs(np.tanh(s).astype(np.float64) - np.tanh(s.astype(np.float64))).max())


TAIL_FORMS = tuple((cc, t) for cc in ("fma", "sep") for t in ("fma", "sep"))      # (Cc = b3 a + s in fp32, t = sk Ca + Cc in packed fp16)
TAIL_K1, TAIL_K2 = 32, 9 * 128


def tail_operands(w3, b3, A, S, cc_form):
    """bg_tail.hip:33-35, 50-52: Ca = fp16(a); the conv_3 fragments fp16(w3 Ca) (a packed fp16 product: one rounding); Cc = fp16(fp32(b3 a + s))."""
    Ca = h16(r32(A))
    return h16(h16(w3).reshape(128, -1) * Ca[:, None]), Ca, h16(fma32(r32(b3), r32(A), r32(S), cc_form))


def _conv3(z, w):
    """z [R,R,128] float64, w [3,128,3,3] -> [3,R,R], zero padding (halo pixels outside the image contribute exactly 0)."""
    return F.conv2d(torch.from_numpy(np.ascontiguousarray(z.transpose(2, 0, 1)))[None], torch.from_numpy(np.ascontiguousarray(w)), padding=1)[0].numpy()


def tail_ref(h, x0, w3, b3, A, S, rgb_w, rgb_b, cc_form="fma", t_form="fma"):
    """(ref, tol, s) of bg_tail_kernel, each [B,3,R,R] float64; s is the pre-tanh value.  Mirrored: the weight fragments, Ca, Cc (cc_form).
    Everything else is float64, and the kernel's roundings are COUNTED per element:
      acc    = sum_32 W3s h            first MFMA chain: (2 * 32 + 8) U32 A1, A1 = sum |W3s h|
      a16    = fp16(acc)               U16 |acc|
      t      = sk Ca + Cc  (fp16)      U16 |t| ("fma")  or  U16 |sk Ca| + U16 |t| ("sep")
      z      = relu(a16 + t)  (fp16)   U16 |acc + t|;  relu is 1-Lipschitz, and an element with acc + t < -dz is 0 on both sides: dz = 0 there
      (SUB16 per fp16 rounding; the sum times 1 + 2^-9: each rounding acts on a value already off by the earlier ones, at most 4 U16 relative.)
    dz goes through |W_rgb| over the 9 taps x 128 channels; the second chain and the 27 fp32 additions of partial sums add
    (2 * 1152 + 8 + 27) U32 (sum |W z| + |rgb_b|); tanh is 1-Lipschitz; tanh_term(s) closes it."""
    h, x0 = f64(h), f64(x0)
    W3s, Ca, Cc = tail_operands(w3, b3, A, S, cc_form)
    W, rb = h16(rgb_w)[:3], r32(rgb_b)[:3]
    B, R = h.shape[0], h.shape[1]
    s, tol = np.empty((B, 3, R, R)), np.empty((B, 3, R, R))
    nround = 3 if t_form == "fma" else 4
    for b in range(B):
        acc, A1 = h[b] @ W3s.T, np.abs(h[b]) @ np.abs(W3s).T
        p = up2(x0[b:b + 1])[0] * Ca
        t = p + Cc
        zp = acc + t
        dz = (TAIL_K1 * 2 + 8) * U32 * A1 + U16 * (np.abs(acc) + np.abs(t) + np.abs(zp) + (np.abs(p) if t_form == "sep" else 0.0)) + nround * SUB16
        dz = dz * (1 + 2.0 ** -9)
        dz[zp < -dz] = 0.0
        z = np.maximum(zp, 0.0)
        s[b] = _conv3(z, W) + rb[:, None, None]
        tol[b] = _conv3(dz, np.abs(W)) + (2 * TAIL_K2 + 8 + 27) * U32 * (_conv3(z, np.abs(W)) + np.abs(rb)[:, None, None])
    return np.tanh(s), tol + tanh_term(s), s


def tail_inputs(B, R_, seed=None):
    """The random inputs of test_gpu_biggan_ops.py::test_tail (unchanged from the 4e-3 bar's version)."""
    import math
    rng = np.random.default_rng(1200 + R_ if seed is None else seed)
    q = lambda a: np.asarray(a, np.float64).astype(np.float16).astype(f32)
    h = q(np.maximum(rng.standard_normal((B, R_, R_, 32)), 0.0))
    x0 = q(rng.standard_normal((B, R_ // 2, R_ // 2, 128)) + 0.5 * (np.arange(B)[:, None, None, None] % 3 - 1))
    w3 = q(rng.standard_normal((128, 32)) / (math.sqrt(128) + math.sqrt(32)))
    b3 = (0.2 * rng.standard_normal(128)).astype(f32)
    A = (rng.uniform(0.5, 1.5, 128) * rng.choice([-1.0, 1.0], 128)).astype(f32)
    S = (0.3 + 0.5 * rng.standard_normal(128)).astype(f32)
    rgb_w = q(rng.standard_normal((3, 128, 3, 3)) / (math.sqrt(128 * 9) + math.sqrt(128)))
    rgb_b = (0.1 * rng.standard_normal(3)).astype(f32)
    return h, x0, w3, b3, A, S, rgb_w, rgb_b


def tail_lattice(B, R_, seed=0):
    """Inputs on which every intermediate of bg_tail_kernel is exact, and the exact pre-tanh value: (inputs, s [B,3,R,R] float64).
    h >= 0 and x0 in multiples of 1/4, w3 and rgb_w in {0, +-1/4, +-1/2} (uploaded as given), bn_a in +-{1/2, 1, 2}, b3 / bn_s / rgb_b dyadic.
    The premises are asserted: W3s = w3 a and Cc exact under both forms; acc, fp16(acc), t and z fit fp16's 11 bits; the 27 partial sums and
    their sum stay below 2^24 quanta; at least half of the pre-tanh values have |s| <= 2 (tanh must not saturate the defects away)."""
    rng = np.random.default_rng([seed, B, R_])
    h = (rng.integers(0, 5, (B, R_, R_, 32)) * (rng.random((B, R_, R_, 32)) < 0.5) / 4.0).astype(f32)
    x0 = (rng.integers(-4, 5, (B, R_ // 2, R_ // 2, 128)) / 4.0).astype(f32)
    x0 += (0.25 * (np.arange(B) % 3))[:, None, None, None].astype(f32)              # candidates differ by a lattice step
    w3 = (rng.choice([0.25, -0.25, 0.5, -0.5], (128, 32)) * (rng.random((128, 32)) < 0.5)).astype(f32)
    A = (rng.choice([-1.0, 1.0], 128) * 2.0 ** rng.integers(-1, 2, 128)).astype(f32)
    b3 = (rng.integers(-8, 9, 128) / 8.0).astype(f32)
    S = (rng.integers(-40, 9, 128) / 16.0).astype(f32)                               # mostly negative: z is sparse, so rgb_w can be dense enough to use every tap
    rgb_b = (rng.integers(-8192, 8193, 3) / 16384.0).astype(f32)                     # (14 fractional bits: s does not fit fp16)
    wdraw, keep = rng.choice([0.25, -0.25, 0.5, -0.5], (3, 128, 3, 3)), rng.random((3, 128, 3, 3))

    def weights(density):
        w = (wdraw * (keep < density)).astype(f32)
        for c, j, tap in zip(*np.nonzero(np.abs(w).reshape(3, 4, 32, 9).sum(axis=2) == 0)):      # (a column the draw left empty gets one weight)
            w[c, 32 * j + (tap + c) % 32, tap // 3, tap % 3] = 0.25
        return w

    def z_of(b):
        a = f64(A)
        return np.maximum(f64(h[b]) @ (f64(w3) * a[:, None]).T + up2(x0[b:b + 1])[0] * a + (f64(b3) * a + f64(S)), 0.0)
    # the densest rgb_w of this ladder that keeps tanh unsaturated on the first candidate's image (how z's draw came out decides; asserted on all below)
    z0 = z_of(0)
    for density in (0.125, 0.09, 0.0625, 0.045, 0.03, 0.02, 0.0):
        rgb_w = weights(density)
        if (np.abs(_conv3(z0, f64(rgb_w)) + f64(rgb_b)[:, None, None]) <= 2.0).mean() >= 0.6:
            break
    inp = (h, x0, w3, b3, A, S, rgb_w, rgb_b)
    # every (tap, colour) column of the second chain carries weight in every 32-channel slice
    assert (np.abs(rgb_w).reshape(3, 4, 32, 9).sum(axis=2) > 0).all(), "tail lattice: a (colour, slice, tap) without weight"
    ops = [tail_operands(w3, b3, A, S, f) for f in ("fma", "sep")]
    for a, b in zip(*ops):
        assert np.array_equal(a, b), "tail lattice: the operands differ between the forms"
    W3s, Ca, Cc = ops[0]
    assert np.array_equal(W3s, f64(w3) * f64(A)[:, None]) and np.array_equal(Cc, f64(b3) * f64(A) + f64(S)) and np.array_equal(Ca, f64(A))
    fits11 = lambda v: np.array_equal(v, h16(v))                                     # (representable in fp16: 11 significant bits, in range)
    s = np.empty((B, 3, R_, R_))
    for b in range(B):
        hb = f64(h[b])
        A1 = np.abs(hb) @ np.abs(W3s).T
        assert A1.max() < 2.0 ** 24 / 32 and np.array_equal(hb * 4, np.round(hb * 4)) and np.array_equal(W3s * 8, np.round(W3s * 8))   # products in multiples of 1/32: any order of the first chain is exact
        acc = hb @ W3s.T
        sk = up2(x0[b:b + 1])[0]
        t = sk * Ca + Cc                      # the product and the sum both fit fp16: "fma" and "sep" round nothing (fma16 is checked on one row)
        assert fits11(sk * Ca) and fits11(t) and all(np.array_equal(fma16(sk[0], Ca, Cc, form), t[0]) for form in ("fma", "sep"))
        zp = acc + t
        assert fits11(acc) and fits11(zp), "tail lattice: acc, t or z does not fit 11 bits"
        z = np.maximum(zp, 0.0)
        assert np.array_equal(z * 32, np.round(z * 32))                              # z in multiples of 1/32, z W in multiples of 1/128, rgb_b of 2^-14
        Asum = _conv3(z, np.abs(f64(rgb_w))) + np.abs(f64(rgb_b))[:, None, None]
        assert Asum.max() < 2.0 ** 24 / 16384, "tail lattice: the partial sums leave the fp32 lattice"
        s[b] = _conv3(z, f64(rgb_w)) + f64(rgb_b)[:, None, None]
        assert np.array_equal(s[b], r32(s[b]))
    assert (np.abs(s) <= 2.0).mean() >= 0.5, "tail lattice: tanh saturates on more than half of the pixels (%.2f within 2)" % (np.abs(s) <= 2.0).mean()
    return inp, s


# ---- bg_tail in fp32 / packed fp16, tile by tile as the kernel walks the image: the faithful emulation and its planted defects ----------
TAIL_TH, TAIL_TW, TAIL_PW, TAIL_NPX = 8, 32, 34, 340


def tail_emulation(inp, cc_form="fma", t_form="fma", defect=None, grid=512):
    """fp32 accumulators (numpy float32 matmul), the packed fp16 epilogue, z zero outside the image, the 27 partial sums per halo pixel in
    fp32, their sum in the kernel's order (rgb_b first, taps row by row), float32 tanh.  defect: one of TAIL_DEFECTS."""
    h, x0, w3, b3, A, S, rgb_w, rgb_b = inp
    W3s, Ca, Cc = (a.astype(f32) for a in tail_operands(w3, b3, A, S, cc_form))
    B, R = h.shape[0], h.shape[1]
    tx_n, ty_n = R // TAIL_TW, R // TAIL_TH
    # rows n = tap * 3 + colour of the second chain, 27 used of 32
    Wn = np.zeros((32, 128), f32)
    Wn[:27] = h16(rgb_w)[:3].transpose(2, 3, 0, 1).reshape(27, 128)
    idx = np.clip(np.arange(-1, R + 1), 0, R - 1)                                    # the clamped coordinates of the halo
    inside = (np.arange(-1, R + 1) >= 0) & (np.arange(-1, R + 1) < R)
    out = np.empty((B, 3, R, R), f32)
    Pall = []
    for b in range(B):
        hb = np.asarray(h[b], f32)[idx][:, idx]                                      # [R+2,R+2,32]
        acc = hb @ W3s.T
        sidx = ((idx + 1) >> 1 if defect == "skip_round_up" else idx >> 1)
        sidx = np.minimum(sidx, R // 2 - 1)
        sk = f64(x0[b])[idx >> 1][:, sidx]
        t = fma16(sk, Ca.astype(np.float64), Cc.astype(np.float64), t_form)
        z = np.maximum(h16(h16(acc) + t), 0.0)
        inb = inside[:, None] & inside[None, :]
        if defect == "inb_right":
            inb = inside[:, None] & (inside[None, :] | (np.arange(-1, R + 1) == R)[None, :])
        z = np.where(inb[..., None], z, 0.0).astype(f32)
        if defect == "slice_dropped":
            z[..., 32:64] = 0
        Pall.append(z)
    for b in range(B):
        for ty in range(ty_n):
            for tx in range(tx_n):
                tile = (b * ty_n + ty) * tx_n + tx
                reg = Pall[b][ty * 8:ty * 8 + 10, tx * 32:tx * 32 + 34].reshape(TAIL_NPX, 128)
                if defect == "stale_prefetch" and tile >= grid:                      # the first four 32-pixel blocks from the operands prefetched for the previous tile
                    pt = tile - grid
                    pb, pr = divmod(pt, ty_n * tx_n)
                    py, px = divmod(pr, tx_n)
                    reg = reg.copy()
                    reg[:128] = Pall[pb][py * 8:py * 8 + 10, px * 32:px * 32 + 34].reshape(TAIL_NPX, 128)[:128]
                P = (reg @ Wn.T).reshape(10, 34, 32)                                 # fp32 partial sums
                sacc = np.broadcast_to(np.asarray(rgb_b, f32)[:3, None, None], (3, 8, 32)).copy()
                for dy in range(3):
                    for dx in range(3):
                        n = (dy * 3 + dx) * 3
                        sub = P[dy:dy + 8, dx:dx + 32]
                        for c in range(3):
                            col = np.full((8, 32), n + c)
                            if defect == "swizzle_key" and dy == 1 and dx == 1:      # the centre tap reads with key (pp + 1) & 7
                                pp = (np.arange(8)[:, None] + dy) * TAIL_PW + np.arange(32)[None, :] + dx
                                col = ((((n + c) >> 2) ^ (pp & 7) ^ ((pp + 1) & 7)) << 2) + ((n + c) & 3)
                            sacc[c] = sacc[c] + np.take_along_axis(sub, col[..., None], axis=2)[..., 0]
                out[b, :, ty * 8:ty * 8 + 8, tx * 32:tx * 32 + 32] = np.tanh(sacc)
    return out


TAIL_DEFECTS = ("inb_right", "skip_round_up", "stale_prefetch", "slice_dropped", "swizzle_key")


# ---- the batched GEMMs (self-attention products) ------------------------------------------------------------------------------------------
def gemm_ref(a, w, mode):
    """(ref, tol) [batch,M,N] float64 of out = a[z] w[z]^T on fp16 operands: (2 K + 8) U32 A, A = sum |a w|, + U16 |out| for the fp16 store of
    mode 0, + 2^-24 (conv_ops_ref's bound without an epilogue)."""
    a, w = f64(a), f64(w)
    K = a.shape[2]
    ref = np.einsum("bmk,bnk->bmn", a, w)
    A = np.einsum("bmk,bnk->bmn", np.abs(a), np.abs(w))
    return ref, (2 * K + 8) * U32 * A + (U16 * np.abs(ref) if mode == 0 else 0.0) + 2.0 ** -24


def gemm_inputs(M, N, K, batch=3):
    """The random operands of test_gemm_batched: O(1) apart per batch slice."""
    rng = np.random.default_rng(1100 + M + N + K)
    q = lambda v: np.asarray(v, np.float64).astype(np.float16).astype(f32)
    return (q(rng.standard_normal((batch, M, K)) + np.arange(batch)[:, None, None] - 1.0),
            q(rng.standard_normal((batch, N, K)) * K ** -0.5 * (1.0 + np.arange(batch)[:, None, None])))


def gemm_lattice(M, N, K, mode, batch=3, seed=0):
    """Both operands on the lattice (a in multiples of 1/4 up to 1, w in {0, +-1/4, +-1/2}): every partial sum in every order is exact in fp32
    (asserted: sum |a w| < 2^24 / 16).  Returns (a, w, want): want is the exact sum (mode 3) or its fp16 rounding (mode 0), as float32."""
    rng = np.random.default_rng([seed, M, N, K])
    a = (rng.integers(-4, 5, (batch, M, K)) / 4.0).astype(f32)
    w = rng.choice(np.array([0, 0.25, -0.25, 0.5, -0.5], f32), size=(batch, N, K))
    ref = np.einsum("bmk,bnk->bmn", f64(a), f64(w))
    A = np.einsum("bmk,bnk->bmn", np.abs(f64(a)), np.abs(f64(w)))
    assert A.max() < 2.0 ** 24 / 16 and np.array_equal(ref, r32(ref)) and np.array_equal(ref * 16, np.round(ref * 16))
    assert np.abs(ref).max() < 65504
    return a, w, (h16(ref) if mode == 0 else ref).astype(f32)


def gemm_emulation(a, w, mode, defect=None):
    """fp32 accumulation (numpy float32 matmul), fp16 store in mode 0.  defect "neighbour_w": slice z reads w[z + 1]; "k_step": one 64-deep
    K step (the last) is dropped."""
    a, w = np.asarray(a, f32), np.asarray(w, f32)
    if defect == "neighbour_w":
        w = np.roll(w, -1, axis=0)
    if defect == "k_step":
        a = a[..., :-64]
        w = w[..., :-64]
    out = np.einsum("bmk,bnk->bmn", a, w, dtype=f32)
    return h16(out).astype(f32) if mode == 0 else out


def gemm_instance(M, N, K, batch, cand_batch, cus=256, nominal=64):
    """The symbol launch_gemm_tiled / launch_gemm_direct pick for a batched product (gemm_tiled.hip:216-262, conv_direct.hip:260-270)."""
    if K % 64 != 0 or M < 64:
        return "gemm_direct_kernel<%d>" % (4 if N > 64 else 2 if N > 32 else 1)
    fills = -(-M // 128) * (N // 128) * (nominal if cand_batch else batch) >= cus
    return "gemm_tiled_kernel<128>" if N % 128 == 0 and fills else "gemm_tiled_kernel<64>"
