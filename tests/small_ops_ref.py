"""Float64 restatements of the small fp32 kernels around StyleGAN2 and the CLIP towers, one per kernel (test infrastructure).

tests/test_gpu_small_ops.py compares each HIP kernel with the function of the same name here; tests/test_small_ops_ref.py pins these
functions to oracle/stylegan2_ref.py, oracle/clip_ref.py, oracle/fitness_ref.py and torch on the CPU, so the GPU tests do not test the
kernels against a private opinion.  Every function takes `dt`: numpy float64 (the reference) or float32 (the twin the error bars are derived
from: the same operations written the plain way in float32, sums of many terms added one term after the other as a kernel's thread adds
them).  Operands are taken as the device holds them (weights transposed [K, N] with their coefficient folded); nothing here rounds to fp16.
"""
import numpy as np

SQRT2 = np.sqrt(2.0)


def _a(x, dt):
    return np.asarray(x, dtype=dt)


def seq_sum(a, dt, axis=-1):
    """Sum along `axis`: float64 as numpy sums, float32 one term after the other."""
    a = _a(a, dt)
    if dt == np.float64:
        return a.sum(axis=axis)
    a = np.moveaxis(a, axis, 0)
    acc = np.zeros(a.shape[1:], dt)
    for k in range(a.shape[0]):
        acc = acc + a[k]
    return acc


def matmul(x, wt, dt):
    """x [P, K] @ wt [K, N]; the float32 twin adds the K products of an output one after the other."""
    x, wt = _a(x, dt), _a(wt, dt)
    if dt == np.float64:
        return x @ wt
    acc = np.zeros((x.shape[0], wt.shape[1]), dt)
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * wt[k]
    return acc


def lrelu_sqrt2(v, dt):
    v = _a(v, dt)
    return np.where(v > 0, v, dt(0.2) * v) * dt(SQRT2)


def pixelnorm(z, dt=np.float64, eps=1e-8):
    """stylegan2/models.py:625-626: z * rsqrt(mean(z^2) + eps) per row."""
    z = _a(z, dt)
    ms = seq_sum(z * z, dt) / dt(z.shape[1])
    return z * (dt(1) / np.sqrt(ms + dt(eps)))[:, None]


def dense(x, wt, bias=None, in_sq=False, mode=0, eps_row=None, dt=np.float64):
    """dense_kernel / dense_splitk_kernel / dense_multi_kernel: epi(f(x) @ wt + bias), f = square with in_sq; mode 0 none, 1 lrelu * sqrt2,
    2 rsqrt(v + eps_row[p])."""
    x = _a(x, dt)
    v = matmul(x * x if in_sq else x, wt, dt)
    if bias is not None:
        v = v + _a(bias, dt)
    if mode == 1:
        v = lrelu_sqrt2(v, dt)
    elif mode == 2:
        with np.errstate(divide="ignore", over="ignore"):
            v = dt(1) / np.sqrt(v + _a(eps_row, dt).reshape(-1, 1))
    return v


def mapping(z, wt, b, dt=np.float64):
    """stylegan2/models.py:590-627: pixel norm, then per layer dense + bias + lrelu * sqrt2.  wt [n, L(k), L(n)] and b [n, L] carry their
    coefficients (lr_mul / sqrt(L), lr_mul)."""
    x = pixelnorm(z, dt)
    for w_, b_ in zip(wt, b):
        x = dense(x, w_, b_, mode=1, dt=dt)
    return x


def style_norm(s, segments, dt=np.float64, eps=1e-8):
    """Per (row, segment): smax = max(max|s|, 1e-20), s <- s * (1 / smax), eps_row = eps * (1 / smax)^2 (csrc/kernels_misc.hip
    style_norm_kernel; the algebra of util.style_tables).  The float32 twin multiplies by the rounded reciprocal, as the kernel does."""
    s = _a(s, dt).copy()
    P = s.shape[0]
    smax, eps_row = np.empty((P, len(segments)), dt), np.empty((P, len(segments)), dt)
    with np.errstate(over="ignore"):
        for l, (o, n) in enumerate(segments):
            m = np.maximum(np.abs(s[:, o:o + n]).max(axis=1), dt(1e-20))
            inv = dt(1) / m
            s[:, o:o + n] = s[:, o:o + n] * inv[:, None]
            smax[:, l] = m
            eps_row[:, l] = dt(eps) * inv * inv
    return s, smax, eps_row


def d_head(dfin, w0, b0, w1, b1, dt=np.float64):
    """stylegan2/models.py:1339-1350 on the flattened final map: dense (16 CL -> CL) + bias + lrelu * sqrt2, dense (CL -> 1) + bias.
    dfin [P, 16 CL], w0 [CL, 16 CL] (the values the device multiplies: already rounded to fp16), w1 [CL] -> dis [P]."""
    h = lrelu_sqrt2(matmul(dfin, _a(w0, dt).T, dt) + _a(b0, dt), dt)
    return matmul(h, _a(w1, dt).reshape(-1, 1), dt)[:, 0] + _a(b1, dt)[0]


def mbstd(x, batch_size, group, dt=np.float64, eps=1e-8):
    """stylegan2/modules.py:701-747 per D call of batch_size samples, x [B, hw, C] -> (group-mean-subtracted features [B, hw, C], the
    std value of each sample [B]): sample s of a call belongs to sub-group s % (batch_size / group)."""
    x = _a(x, dt)
    B, hw, C = x.shape
    nsub = batch_size // group
    d = np.empty_like(x)
    std = np.empty(B, dt)
    for mb in range(B // batch_size):
        for j in range(nsub):
            idx = [mb * batch_size + j + g * nsub for g in range(group)]
            v = x[idx]
            mean = seq_sum(v, dt, axis=0) / dt(group)
            dv = v - mean
            var = seq_sum(dv * dv, dt, axis=0) / dt(group)
            d[idx] = dv
            sd = np.sqrt(var + dt(eps)).reshape(-1)
            std[idx] = seq_sum(sd, dt) / dt(sd.size)
    return d, std


def finalize_image(y, dt=np.float64):
    """utils.py:14-17 biggan_norm: clip((y + 1) / 2, 0, 1)."""
    return np.clip((_a(y, dt) + dt(1)) * dt(0.5), dt(0), dt(1))


def layernorm(x, g, b, dt=np.float64, eps=1e-5):
    """clip/model.py:152-158: two-pass mean / variance over the last axis."""
    x = _a(x, dt)
    D = x.shape[-1]
    mean = seq_sum(x, dt) / dt(D)
    d = x - mean[..., None]
    var = seq_sum(d * d, dt) / dt(D)
    return d * (dt(1) / np.sqrt(var + dt(eps)))[..., None] * _a(g, dt) + _a(b, dt)


def embed_lnpre(patch_emb, cls, pos, g, b, dt=np.float64):
    """clip/model.py:221-225: [class_embedding ; patch embeddings] + positional_embedding, then ln_pre.  patch_emb [P, T - 1, D]."""
    pe = _a(patch_emb, dt)
    tok = np.concatenate([np.broadcast_to(_a(cls, dt), (pe.shape[0], 1, pe.shape[2])), pe], axis=1) + _a(pos, dt)
    return layernorm(tok, g, b, dt)


def embed_text(tokens, tok_emb, pos, dt=np.float64):
    """clip/model.py:308-310: token_embedding[tokens] + positional_embedding -> [n * ctx, D]."""
    tokens = np.asarray(tokens)
    x = _a(tok_emb, dt)[tokens] + _a(pos, dt)
    return x.reshape(-1, x.shape[-1])


def cosine(feat, target, dt=np.float64, eps=1e-8):
    """torch.cosine_similarity(feat [P, D], target [1, D]) as the kernel writes it: x.y / max(|x| |y|, eps)."""
    f, t = _a(feat, dt), _a(target, dt).reshape(1, -1)
    xy, xx, yy = seq_sum(f * t, dt), seq_sum(f * f, dt), seq_sum(t * t, dt)
    return xy / np.maximum(np.sqrt(xx) * np.sqrt(yy), dt(eps))


def cosine_views(feat, target, dt=np.float64):
    """feat [P, V, D] -> (per-view cosines [P, V], their mean summed in the order v = 0 .. V - 1)."""
    f = _a(feat, dt)
    P, V, D = f.shape
    vs = cosine(f.reshape(P * V, D), target, dt).reshape(P, V)
    acc = np.zeros(P, dt)
    for v in range(V):
        acc = acc + vs[:, v]
    return vs, acc / dt(V)


def assemble_F(sim, dis=None, dt=np.float64):
    """problem.py:23-27: F = -sim, or column_stack(-sim, relu(1 - dis))."""
    sim = _a(sim, dt)
    if dis is None:
        return -sim[:, None]
    return np.stack([-sim, np.maximum(dt(1) - _a(dis, dt), dt(0))], axis=1)


def image_patches(img, ps):
    """img [n, 3, S, S] -> the patch-embedding operand [n G G, 3 ps ps]: row (b, gy, gx), column (c, iy, ix) (clip/model.py:206, 219)."""
    img = np.asarray(img)
    n, _, S, _ = img.shape
    G = S // ps
    return img.reshape(n, 3, G, ps, G, ps).transpose(0, 2, 4, 1, 3, 5).reshape(n * G * G, 3 * ps * ps)
