"""References of the perceptual objective (test infrastructure): LPIPS on VGG16 as include/glass.h states it
(stylegan2/external_models/lpips.py:34-78 fed as stylegan2/project.py:113-122,263 feeds it), in float64.

* lpips(sd, x0, x1): the semantics restated in float64 — (v - shift) / scale, the five VGG16 slices, unit-normalisation over channels with
  eps 1e-8, squared difference averaged over H x W, weighted by the slice's lin vector, summed.
* lpips(..., storage16=True): the same arithmetic in float64 with the input of the first convolution, the convolution weights and every stored
  activation rounded to fp16 — what the engine's storage format alone costs (its sums are fp32; this emulation keeps them exact).

Weights: clip_glass_amd.synth.lpips_state(seed) — a dict under the engine's keys.  Images are NCHW in [-1, 1]."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from clip_glass_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_modules.npz")
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
SLICE_END = (2, 7, 14, 21, 28)          # features index of the last convolution of each slice
POOL_BEFORE = (5, 10, 17, 24)           # a MaxPool2d(2) stands in front of these convolutions
FIXTURE_SEED = 11


def _r16(t):
    return t.to(torch.float16).to(torch.float64)


def area(y, S):
    """F.interpolate(mode="area") of [n, 3, R, R] to S for R % S == 0: the exact box mean, float64."""
    y = torch.as_tensor(np.asarray(y), dtype=torch.float64)
    n, c, R, _ = y.shape
    assert R % S == 0
    b = R // S
    return y.reshape(n, c, S, b, S, b).mean(dim=(3, 5))


def scale_input(x, storage16=False):
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    v = (x - torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    return _r16(v) if storage16 else v


def slices(sd, x, storage16=False, trace=None):
    """The five slice outputs [n, C_k, S / 2^k, S / 2^k] (float64) of the scaled input x.  trace: a list that receives every conv output."""
    rnd = _r16 if storage16 else (lambda t: t)
    out = []
    for idx, cin, cout in synth.VGG16_CONVS:
        if idx in POOL_BEFORE:
            x = F.max_pool2d(x, 2)
        w = rnd(torch.as_tensor(sd["lpips.features.%d.weight" % idx], dtype=torch.float64))
        b = torch.as_tensor(sd["lpips.features.%d.bias" % idx], dtype=torch.float64)
        x = rnd(torch.relu(F.conv2d(x, w, b, padding=1)))
        if trace is not None:
            trace.append(x)
        if idx in SLICE_END:
            out.append(x)
    return out


def head_term(f0, f1, lin):
    """One slice's term: sum_c lin_c mean_hw (f0 rsqrt(sum_c f0^2 + 1e-8) - f1 rsqrt(...))^2; f0, f1 [n, C, H, W] -> [n]."""
    f0, f1 = torch.as_tensor(f0, dtype=torch.float64), torch.as_tensor(f1, dtype=torch.float64)
    n0 = f0 * torch.rsqrt((f0 ** 2).sum(1, keepdim=True) + 1e-8)
    n1 = f1 * torch.rsqrt((f1 ** 2).sum(1, keepdim=True) + 1e-8)
    return (((n0 - n1) ** 2).mean(dim=(2, 3)) * torch.as_tensor(lin, dtype=torch.float64).view(1, -1)).sum(1)


def lpips(sd, x0, x1, storage16=False):
    """float64 [n]: LPIPS_VGG16(pixel_min=-1, pixel_max=1).forward(x0, x1); x1 may hold one image for all of x0."""
    a = slices(sd, scale_input(x0, storage16), storage16)
    b = slices(sd, scale_input(x1, storage16), storage16)
    d = 0
    for k in range(5):
        d = d + head_term(a[k], b[k].expand_as(a[k]), sd["lpips.lin.%d.weight" % k])
    return d.numpy()


def max_activation(sd, x):
    """Largest |activation| any layer holds on the images x (float64 reference)."""
    tr = []
    xin = scale_input(x)
    slices(sd, xin, trace=tr)
    return max([float(xin.abs().max())] + [float(t.abs().max()) for t in tr])


def images(seed, n, S, name="img"):
    """Seeded images [n, 3, S, S] in [-1, 1]: smooth structure plus noise, so neighbouring pixels correlate as in a picture."""
    lo = synth.normal(seed, name + ".lo", (n, 3, S // 4, S // 4), std=0.5)
    hi = synth.normal(seed, name + ".hi", (n, 3, S, S), std=0.15)
    x = np.repeat(np.repeat(lo, 4, axis=2), 4, axis=3) + hi
    return np.clip(x, -1.0, 1.0).astype(np.float32)
