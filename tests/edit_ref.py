"""Float64 restatements of the image-editing kernels (csrc/edit.hip; include/glass.h "Image editing"), each with its float32 twin in the
kernel's documented summation order (test infrastructure).

The directional cosine is the section's formula written with torch.nn.functional.cosine_similarity on float64 differences; the views' mean,
the weighted combination and the sign rule are prompt_set_ref's.  The twins add as a wave does: lane-strided partial sums (i = lane; i < D;
i += 64), then the butterfly over offsets 32, 16, .. 1, every product and sum rounded to float32 on its own.  tests/test_edit_ref.py pins both.

The inputs and the bar of tests/test_gpu_edit_ops.py live here too, so that the CPU test can show that the bar bites at those shapes."""
import numpy as np
import torch

import prompt_set_ref as PR

F32, F64 = np.float32, np.float64
EPS = 1e-8


def lane_sum(a):
    """float32 [..., D] -> [...]: a wave's sum of a row — lane l adds elements l, l + 64, ... in that order, then lanes combine by
    v[l] += v[l ^ o] for o = 32, 16, .. 1 (every lane ends with the same bits)."""
    a = np.asarray(a, F32)
    D = a.shape[-1]
    K = (D + 63) // 64
    pad = np.zeros(a.shape[:-1] + (K * 64,), F32)
    pad[..., :D] = a                                    # (adding +0.0 to a partial sum that starts at +0.0 changes nothing)
    pad = pad.reshape(a.shape[:-1] + (K, 64))
    v = np.zeros(a.shape[:-1] + (64,), F32)
    for k in range(K):
        v = v + pad[..., k, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def unit_rows(f, dt=F64):
    """f / max(|f|, 1e-8) per row: how a source feature becomes a source row, and what the kernel does to a feature row."""
    f = np.asarray(f, dt)
    n = np.sqrt(lane_sum(f * f)) if dt == F32 else np.sqrt((f * f).sum(-1))
    return f / np.maximum(n, dt(EPS))[..., None]


def directional_cosines(feat, targets, src, dt=F64):
    """c [P, V, T]: the cosine between x = f / max(|f|, 1e-8) - src[v] and g_t, x.g / max(|x| |g|, 1e-8); x = 0 gives 0."""
    f, g, s = np.asarray(feat, dt), np.asarray(targets, dt), np.asarray(src, dt)
    P, V, D = f.shape
    T = g.shape[0]
    x = unit_rows(f, dt) - s[None]
    if dt == F64:
        xt = torch.from_numpy(np.ascontiguousarray(x)).reshape(P * V, 1, D)
        c = torch.nn.functional.cosine_similarity(xt, torch.from_numpy(np.ascontiguousarray(g)).reshape(1, T, D), dim=-1, eps=EPS)
        return c.numpy().reshape(P, V, T)
    nx = np.sqrt(lane_sum(x * x))
    c = np.empty((P, V, T), F32)
    for t in range(T):
        xy, yy = lane_sum(x * g[t]), lane_sum(g[t] * g[t])
        c[:, :, t] = xy / np.maximum(nx * np.sqrt(yy), F32(EPS))
    return c


def cosine_set_dir(feat, targets, weights, src, dt=F64):
    """feat [P, V, D], targets [T, D], weights [T], src [V, D] -> (view_sim [P, V]: entry 0 per view, set_sim [P, T]: per entry the mean
    over the views summed in the order v = 0 .. V - 1 (the cosine itself for V = 1), sim [P]: prompt_set_ref.combine)."""
    c = directional_cosines(feat, targets, src, dt)
    V = c.shape[1]
    if V == 1:
        set_sim = c[:, 0]
    else:
        acc = np.zeros(c[:, 0].shape, dt)
        for v in range(V):
            acc = acc + c[:, v]
        set_sim = acc / dt(V)
    return c[:, :, 0], set_sim, PR.combine(set_sim, weights, dt)


def latent_anchor(w, a, dt=F64):
    """w [P, n_lat, L] — or [P, L]: one row for every layer —, a [n_lat, L] -> d [P] = sum_l sum_i (w - a)^2 / (n_lat L); the twin sums the
    flattened (l, i) index as a wave does and divides once."""
    a = np.asarray(a, dt)
    w = np.asarray(w, dt)
    if w.ndim == 2:
        w = np.broadcast_to(w[:, None, :], (w.shape[0],) + a.shape)
    x = (w - a[None]).reshape(w.shape[0], -1)
    if dt == F64:
        return (x * x).sum(-1) / dt(x.shape[1])
    return lane_sum(x * x) / F32(x.shape[1])


def assemble_F_edit(sim, anchor, anchor_lambda=0.0, dis=None, lp=None, lp_lambda=0.0, set_sim=None, weights=None, dt=F64):
    """F with the anchor distance ("Image editing"): the similarity columns (-sim with the folds, or the pareto columns of set_sim), the hinge,
    the LPIPS distance as its own column, the anchor as its own last column (anchor_lambda == 0) or folded: F0 + anchor_lambda * d behind the
    LPIPS fold.  (The kernel's folds are fused multiply-adds: one rounding; this float64 form is the value they round.)"""
    d = np.asarray(anchor, dt)
    if set_sim is not None:
        cols = [PR.assemble_F_set(set_sim, weights, dt=dt)]
    else:
        f0 = -np.asarray(sim, dt)
        if lp is not None and lp_lambda > 0:
            f0 = dt(lp_lambda) * np.asarray(lp, dt) + f0
        if anchor_lambda > 0:
            f0 = dt(anchor_lambda) * d + f0
        cols = [f0[:, None]]
    if dis is not None:
        cols.append(np.maximum(dt(1) - np.asarray(dis, dt), dt(0))[:, None])
    if lp is not None and not lp_lambda > 0:
        cols.append(np.asarray(lp, dt)[:, None])
    if not anchor_lambda > 0:
        cols.append(d[:, None])
    return np.concatenate(cols, axis=1)


# ---- what tests/test_gpu_edit_ops.py runs, shared with tests/test_edit_ref.py ----
def bar(ref64, ref32):
    """The project's general bar: 4 * max|ref32 - ref64|, or one spacing of max|ref64| where the twin is exact."""
    ref64 = np.asarray(ref64, F64)
    e32 = float(np.abs(np.asarray(ref32, F64) - ref64).max())
    return float(np.spacing(F32(np.abs(ref64).max()))) if e32 == 0.0 else 4 * e32


def dir_inputs(P, V, T, D, seed=5):
    """Independent normal feature, source and entry rows (so |x| is of order 1), the sources of unit length; weights of mixed sign."""
    rng = np.random.default_rng(seed + 100000 * P + 1000 * V + 10 * T + D)
    feat = (rng.standard_normal((P, V, D)) * rng.uniform(0.5, 20.0, (P, V, 1))).astype(F32)
    src = unit_rows(rng.standard_normal((V, D)).astype(F32), F32)
    targets = rng.standard_normal((T, D)).astype(F32)
    mags = np.array([1.0, 1e-3, 1e3, 0.37, 12.5, 2.0, 0.05, 300.0, 1.5, 0.9, 7.0, 0.011, 45.0, 3.0, 0.6, 1.0])[:T]
    weights = (mags * np.where(np.arange(T) % 3 == 1, -1.0, 1.0)).astype(F32)
    return feat, targets, weights, src


def dyadic_unit_rows(V, D, seed=9):
    """Rows of length exactly 1 in any summation order: min(D, 16) entries of +-2^-k with 4^-k * count = 1, zeros elsewhere."""
    rng = np.random.default_rng(seed + D)
    n = 16 if D >= 16 else 4 if D >= 4 else 1
    rows = np.zeros((V, D), F32)
    for v in range(V):
        idx = rng.choice(D, n, replace=False)
        rows[v, idx] = rng.choice([-1.0, 1.0], n) / np.sqrt(n)
    return rows


def anchor_inputs(P, n_lat, L, layered=True, seed=3):
    """Anchor rows like dlatents (a common offset, unit spread), candidates at distances from 1e-3 to 1 of them."""
    rng = np.random.default_rng(seed + 1000 * n_lat + L + P)
    a = (rng.standard_normal((n_lat, L)) + 0.3).astype(F32)
    step = np.logspace(-3, 0, P)[:, None, None]
    if layered:
        w = (a[None] + step * rng.standard_normal((P, n_lat, L))).astype(F32)
    else:
        w = (a[0][None] + step[:, 0] * rng.standard_normal((P, L))).astype(F32)
    return w, a
