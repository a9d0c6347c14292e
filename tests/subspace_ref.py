"""float64 restatement of latent space "sub" (include/glass.h "Subspace latent space"), with layer_psi applied after it, and the
elementwise error bar of the fp32 kernels against it.

    acc[p][g][j]  = sum_k c[p][g][k] B[k][j]
    dlat[p][l][j] = base[l][j] + acc[p][layer_group[l]][j]        (base[l][j] alone on a frozen layer, layer_group[l] = -1)
    out           = lerp(avg, dlat, layer_psi[l])                  (the truncation trick; psi = 1 on a layer: dlat itself)

The bar.  u = 2^-24.  An output of a layer with a group is K FMAs and one add, K + 1 roundings, so the standard gamma bound gives
    bar[p][l][j] = (K + 2) u (|base[l][j]| + sum_k |c[p][g][k] B[k][j]|),
evaluated in float64; a frozen layer is a copy and its bar is 0.  Inputs are O(1) normals: no subnormals are involved.
With a truncated layer (psi = w != 1) the kernel computes d = b - a (one rounding) and then fma(coeff, d, t) (one rounding) with (coeff, t)
= (w, a) for w < 0.5 and (w - 1, b) otherwise (torch.lerp's rule; w - 1 is exact for w in [0.5, 1]).  To first order an error e of b comes
out as w e in both branches, and the two roundings are bounded the same way as above — (2 + 1) u times the sum of the magnitudes of the
terms — so
    bar_psi = w bar (1 + 3 u) + 3 u (|coeff| |b - a| + |t|).
"""
import numpy as np

U = 2.0 ** -24
F32, F64 = np.float32, np.float64


def layer_psi(n_lat, psi, cutoff):
    """float64 [n_lat]: psi (as the fp32 value the engine holds) below the cutoff, 1 elsewhere; cutoff None: every layer."""
    out = np.ones(n_lat, F64)
    out[:n_lat if cutoff is None or cutoff < 0 else cutoff] = F64(F32(psi))
    return out


def _groups(c, layer_group, basis, base):
    c, basis, base = np.asarray(c), np.asarray(basis), np.asarray(base)
    lg = np.asarray(layer_group, np.int64)
    P, G, K = c.shape
    n_lat, L = base.shape
    assert basis.shape == (K, L) and lg.shape == (n_lat,) and lg.min() >= -1 and lg.max() < G
    return c, lg, basis, base


def expand(c, layer_group, basis, base, psi=1.0, cutoff=None, avg=None):
    """(dlat, bar), float64 [P][n_lat][L] each: the rule and its error bar for c [P][G][K], layer_group [n_lat], basis [K][L], base
    [n_lat][L]; psi / cutoff / avg [L]: the truncation trick on top (needed only where psi != 1)."""
    c, lg, basis, base = _groups(c, layer_group, basis, base)
    c64, B64, b64 = c.astype(F64), basis.astype(F64), base.astype(F64)
    K = c.shape[2]
    acc = np.einsum("pgk,kj->pgj", c64, B64)
    mag = np.einsum("pgk,kj->pgj", np.abs(c64), np.abs(B64))
    live = (lg >= 0)[None, :, None]
    dlat = b64[None] + np.where(live, acc[:, np.maximum(lg, 0)], 0.0)
    bar = np.where(live, (K + 2) * U * (np.abs(b64)[None] + mag[:, np.maximum(lg, 0)]), 0.0)
    w = layer_psi(len(lg), psi, cutoff)
    if np.all(w == 1.0):
        return dlat, bar
    a = np.asarray(avg, F64)[None, None, :]
    wl = w[None, :, None]
    low = wl < 0.5
    coeff = np.where(low, wl, wl - 1.0)
    t = np.where(low, a, dlat)
    out = np.where(wl == 1.0, dlat, t + coeff * (dlat - a))
    bar_psi = wl * bar * (1 + 3 * U) + 3 * U * (np.abs(coeff) * np.abs(dlat - a) + np.abs(t))
    return out, np.where(wl == 1.0, bar, bar_psi)


def _fma32(a, b, c):
    """round_fp32(a b + c) for fp32 arrays: the product of two fp32 values is exact in float64; the sum is rounded to float64 and then to
    fp32 (a double rounding that can differ from a hardware FMA in the last bit, rarely — far inside any bar here)."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def expand_f32(c, layer_group, basis, base, fault=None):
    """numpy fp32 emulation of the kernel's chain: acc = fma(c[k], B[k], acc) for k = 0 .. K - 1 from 0, then base + acc in fp32; frozen
    layers are copies.  float32 [P][n_lat][L].  fault: one of FAULTS, planted on purpose (tests/test_subspace_ref.py)."""
    c, lg, basis, base = _groups(c, layer_group, basis, base)
    c, basis, base = c.astype(F32), basis.astype(F32), base.astype(F32)
    P, G, K = c.shape
    n_lat, L = base.shape
    B = basis
    if fault == "basis_stride_K":                   # B[k][j] read at k * K + j instead of k * L + j (wrapped into the array)
        flat = basis.reshape(-1)
        B = flat[(np.arange(K)[:, None] * K + np.arange(L)[None, :]) % flat.size]
    acc = np.zeros((P, G, L), F32)
    for k in range(K - 1 if fault == "dropped_last_component" else K):
        acc = _fma32(c[:, :, k, None], B[None, None, k, :], acc)
    out = np.empty((P, n_lat, L), F32)
    for l in range(n_lat):
        g, b = int(lg[l]), base[l]
        if fault == "reversed_group_index" and g >= 0:
            g = G - 1 - g
        if fault == "group1_reads_group0" and g == 1:
            g = 0
        if fault == "base_of_wrong_layer":
            b = base[(l + 1) % n_lat]
        if fault == "frozen_layer_gets_acc" and g < 0:
            g = 0
        out[:, l] = (b[None] + acc[:, g]) if g >= 0 else np.broadcast_to(b, (P, L))
    return out


FAULTS = ("reversed_group_index", "group1_reads_group0", "frozen_layer_gets_acc", "base_of_wrong_layer", "dropped_last_component",
          "basis_stride_K")


def within(got, ref, bar):
    """(ok, worst ratio |got - ref| / bar over the elements with a positive bar, count of elements outside): elements with bar 0 must be
    equal exactly."""
    err = np.abs(np.asarray(got, F64) - ref)
    bad = err > bar
    pos = bar > 0
    return not bad.any(), float((err[pos] / bar[pos]).max()) if pos.any() else 0.0, int(bad.sum())


def case(seed, L, n_lat, K, layer_group, P):
    """O(1) normal operands of one shape: c [P][G][K], basis [K][L], base [n_lat][L], float32."""
    rng = np.random.RandomState(seed)
    G = int(np.max(layer_group)) + 1
    return (rng.normal(size=(P, G, K)).astype(F32), rng.normal(size=(K, L)).astype(F32) / F32(np.sqrt(K)),
            rng.normal(size=(n_lat, L)).astype(F32))


def layer_groups(n_lat):
    """The four assignments the op test runs: one group of all layers; one group per layer; two groups with layers 0 and n_lat - 1 frozen;
    a non-contiguous group {0, n_lat - 1} together with a frozen middle layer (the rest is a second group)."""
    two = np.full(n_lat, -1, np.int32)
    two[1:n_lat // 2] = 0
    two[n_lat // 2:n_lat - 1] = 1
    split = np.ones(n_lat, np.int32)
    split[[0, n_lat - 1]] = 0
    split[n_lat // 2] = -1
    return {"one": np.zeros(n_lat, np.int32), "per_layer": np.arange(n_lat, dtype=np.int32), "two_frozen_ends": two, "split_frozen_middle": split}
