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
