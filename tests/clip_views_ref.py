"""Crop views (include/glass.h, glass_engine_set_clip_views): the definition in torch float64, and index-level fp32 emulations of the two
kernels' arithmetic (view_patches_kernel, resize_patches_kernel) in numpy.  Test infrastructure, no GPU."""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073], dtype=torch.float64)[None, :, None, None]     # clip/clip.py:73
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711], dtype=torch.float64)[None, :, None, None]


def torch_views(img01, S, boxes, normalize=0):
    """The definition: img01 = biggan_norm(y) [B,3,R,R] in [0, 1], boxes [V,4] = (x0, y0, s, flip) -> float64 [B,V,3,S,S]: the reference's
    resize (generator.py:45) of the crop, then the mirror."""
    x = torch.as_tensor(img01).double()
    out = []
    for x0, y0, s, flip in np.asarray(boxes).reshape(-1, 4).tolist():
        v = F.interpolate(x[:, :, y0:y0 + s, x0:x0 + s], (S, S), mode="bilinear", align_corners=False)
        if flip:
            v = torch.flip(v, dims=[3])
        out.append((v - MEAN) / STD if normalize else v)
    return torch.stack(out, dim=1)


def as_patch_rows(v, ps):
    """[B,V,3,S,S] -> the patch operand [(b V + v) G G + g][3 ps ps] (column = (c ps + iy) ps + ix)."""
    v = torch.as_tensor(v)
    B, V, _, S, _ = v.shape
    G = S // ps
    return v.reshape(B * V, 3, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * V * G * G, 3 * ps * ps).numpy()


def _f(v):
    return np.float32(v)


def _axis(n_src, S, out_index):
    """One axis of the kernels' coordinate arithmetic in fp32: (i0, i1, l) per output index, in the source's own coordinates."""
    scale = _f(n_src) / _f(S)
    s = scale * (out_index.astype(np.float32) + _f(0.5)) - _f(0.5)
    s = np.maximum(s, _f(0)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int32), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, (s - i0.astype(np.float32)).astype(np.float32)


def _blend(yc, iy0, iy1, ly, ix0, ix1, lx):
    nrm = lambda v: np.minimum(np.maximum((v + _f(1)) * _f(0.5), _f(0)), _f(1)).astype(np.float32)
    v00, v01 = nrm(yc[..., iy0[:, None], ix0[None, :]]), nrm(yc[..., iy0[:, None], ix1[None, :]])
    v10, v11 = nrm(yc[..., iy1[:, None], ix0[None, :]]), nrm(yc[..., iy1[:, None], ix1[None, :]])
    ly, lx, one = ly[:, None], lx[None, :], _f(1)
    return ((one - ly) * ((one - lx) * v00 + lx * v01) + ly * ((one - lx) * v10 + lx * v11)).astype(np.float32)


def emulate_resize(y, S):
    """resize_patches_kernel's formula on y [B,3,R,R] in (-1, 1): fp32 [B,3,S,S] (before the fp16 store)."""
    y = np.ascontiguousarray(y, np.float32)
    R = y.shape[-1]
    i0, i1, l = _axis(R, S, np.arange(S))
    return _blend(y, i0, i1, l, i0, i1, l)


def emulate_views(y, S, boxes, normalize=0):
    """view_patches_kernel's formula: fp32 [B,V,3,S,S] (before the fp16 store).  The coordinates are the crop's own; the box offsets are
    added to the integer taps; a flipped view computes output column X from column S - 1 - X."""
    y = np.ascontiguousarray(y, np.float32)
    out = []
    for x0, y0, s, flip in np.asarray(boxes).reshape(-1, 4).tolist():
        X = np.arange(S)
        iy0, iy1, ly = _axis(s, S, np.arange(S))
        ix0, ix1, lx = _axis(s, S, S - 1 - X if flip else X)
        v = _blend(y, y0 + iy0, y0 + iy1, ly, x0 + ix0, x0 + ix1, lx)
        if normalize:
            v = ((v - MEAN.numpy()[0].astype(np.float32)) / STD.numpy()[0].astype(np.float32)).astype(np.float32)
        out.append(v)
    return np.stack(out, axis=1)


def edge_boxes(R):
    """Four boxes that touch every edge of an R x R image between them: the whole image, a flipped 2 x 2 crop in the far corner, one that
    touches the top and right edges, one that touches the left and bottom edges."""
    a, b = max(2, (2 * R) // 3), max(2, R // 2 + 1)
    return np.array([(0, 0, R, 0), (R - 2, R - 2, 2, 1), (R - a, 0, a, 0), (0, R - b, b, 1)], np.int32)


def mean_sims(view_sims):
    """[P,V] -> the pass's score: the fp32 sum in the order v = 0 .. V - 1, divided by V."""
    vs = np.asarray(view_sims, np.float32)
    acc = np.zeros(vs.shape[0], np.float32)
    for v in range(vs.shape[1]):
        acc = (acc + vs[:, v]).astype(np.float32)
    return (acc / np.float32(vs.shape[1])).astype(np.float32)
