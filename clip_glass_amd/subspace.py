"""Latent space "sub" on the host (include/glass.h "Subspace latent space"): which style layers form which group, the principal directions
of W (GANSpace, Härkönen et al. 2020), and the npz file both travel in.  Host only, float64 numpy: the engine gets float32 copies.

A population row is [G][K] coefficients; the engine turns it into dlatents[l] = base[l] + c[layer_group[l]] . basis.  build() probes the
mapping network with z ~ N(0, 1), takes the PCA of the mapped rows and scales every component by its standard deviation, so that a
coefficient is unit-variance, as a variable of z is; base is the mean dlatent on every layer."""
import numpy as np

DEFAULT_COMPONENTS = 64
MAX_COMPONENTS = 512                     # glass_subspace_supported: 16 candidates' coefficients are staged in 32 KB of LDS
SUBSPACE_KEYS = ("subspace_components", "subspace_layers", "subspace_samples", "subspace_basis")
NPZ_KEYS = ("mean", "components", "stdev", "layer_group")


def parse_layer_groups(spec, n_lat):
    """layer_group int32 [n_lat] of a spec like "0-3,4-7,8-17": comma-separated inclusive ranges of style layers ("5": one layer), one
    group per range in the order given, every layer not named frozen (-1).  None or "": one group of every layer.  ValueError that names
    the range for an empty or malformed one, a layer outside [0, n_lat) and a layer named twice."""
    n_lat = int(n_lat)
    if n_lat < 1:
        raise ValueError("subspace_layers: the generator has no style layers (n_lat = %d)" % n_lat)
    out = np.full(n_lat, -1, dtype=np.int32)
    if spec is None or not str(spec).strip():
        out[:] = 0
        return out
    for g, part in enumerate(str(spec).split(",")):
        text = part.strip()
        ends = text.split("-")
        if not text or len(ends) > 2 or not all(e.strip().isdigit() for e in ends):
            raise ValueError("subspace_layers: range %r of %r is not LAYER or FIRST-LAST (inclusive, decimal)" % (text, spec))
        lo, hi = int(ends[0]), int(ends[-1])
        if hi < lo:
            raise ValueError("subspace_layers: range %r is empty (FIRST-LAST is inclusive and needs FIRST <= LAST)" % text)
        if hi >= n_lat:
            raise ValueError("subspace_layers: range %r leaves the generator's style layers 0 .. %d" % (text, n_lat - 1))
        taken = [l for l in range(lo, hi + 1) if out[l] >= 0]
        if taken:
            raise ValueError("subspace_layers: range %r overlaps an earlier range at layer %d" % (text, taken[0]))
        out[lo:hi + 1] = g
    return out


def n_groups(layer_group):
    """Number of groups of a layer_group array (its largest index + 1)."""
    return int(np.max(layer_group)) + 1


def pca_basis(samples, K):
    """(mean [L], components [K][L], stdev [K]) of samples [N][L] in float64: eigh of the sample covariance (N - 1 in the denominator), the K
    directions of largest variance in descending order, each with the sign that makes its largest-magnitude entry positive (the first such
    entry on a tie) — so the result is deterministic.  K <= min(L, N - 1)."""
    x = np.asarray(samples, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 2:
        raise ValueError("pca_basis: samples must be [N >= 2, L], got %r" % (x.shape,))
    N, L = x.shape
    K = int(K)
    if not 1 <= K <= min(L, N - 1):
        raise ValueError("pca_basis: K must be in [1, min(L, N - 1) = %d], got %d" % (min(L, N - 1), K))
    mean = x.mean(axis=0)
    d = x - mean
    vals, vecs = np.linalg.eigh(d.T @ d / (N - 1))
    order = np.argsort(-vals, kind="stable")[:K]
    comp = np.ascontiguousarray(vecs[:, order].T)
    big = np.argmax(np.abs(comp), axis=1)
    comp *= np.where(comp[np.arange(K), big] < 0, -1.0, 1.0)[:, None]
    return mean, comp, np.sqrt(np.maximum(vals[order], 0.0))


def operands(mean, components, stdev, n_lat, base=None):
    """(basis float32 [K][L], base float32 [n_lat][L]) as Engine.set_subspace takes them: basis = stdev[:, None] * components, base = the
    mean on every layer unless a base is given ([L], or [n_lat][L]: an edit's source dlatents)."""
    basis = np.asarray(stdev, np.float64)[:, None] * np.asarray(components, np.float64)
    L = basis.shape[1]
    b = np.asarray(mean if base is None else base, np.float64)
    if b.size == L:
        b = np.broadcast_to(b.reshape(1, L), (int(n_lat), L))
    elif b.size == int(n_lat) * L:
        b = b.reshape(int(n_lat), L)
    else:
        raise ValueError("subspace base must hold L = %d floats (a w row) or n_lat * L = %d (a w+ row), got %d" % (L, int(n_lat) * L, b.size))
    return np.ascontiguousarray(basis, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)


def save(path, mean, components, stdev, layer_group):
    """One npz with mean [L], components [K][L], stdev [K] (float64) and layer_group int32 [n_lat]: the shape GANSpace exports, plus the
    groups."""
    with open(path, "wb") as f:          # (a file object: np.savez would append ".npz" to a bare name)
        np.savez(f, mean=np.asarray(mean, np.float64), components=np.asarray(components, np.float64), stdev=np.asarray(stdev, np.float64),
                 layer_group=np.asarray(layer_group, np.int32))


def load(path, latent_size=None):
    """dict(mean, components, stdev, layer_group) of a file save() wrote (layer_group None when the file has none: a plain GANSpace export).
    ValueError by name for a missing array, inconsistent shapes, and — with latent_size — a basis of another network's L."""
    with np.load(path) as f:
        missing = [k for k in NPZ_KEYS[:3] if k not in f.files]
        if missing:
            raise ValueError("subspace_basis %r: missing array(s) %s (expected mean [L], components [K][L], stdev [K])" % (str(path), ", ".join(missing)))
        mean, comp, std = (np.asarray(f[k], np.float64) for k in NPZ_KEYS[:3])
        lg = np.asarray(f["layer_group"], np.int32) if "layer_group" in f.files else None
    if comp.ndim != 2 or mean.shape != (comp.shape[1],) or std.shape != (comp.shape[0],):
        raise ValueError("subspace_basis %r: mean %r, components %r and stdev %r do not fit [L], [K][L], [K]" % (str(path), mean.shape, comp.shape, std.shape))
    if latent_size is not None and comp.shape[1] != int(latent_size):
        raise ValueError("subspace_basis %r: its directions have L = %d entries and the network's dlatents %d: it belongs to another network"
                         % (str(path), comp.shape[1], int(latent_size)))
    return dict(mean=mean, components=comp, stdev=std, layer_group=lg)


def probe(generator, seed, rows, dim_z):
    """`rows` dlatents of z ~ N(0, 1) drawn from `seed`, through the generator's mapping network (map_latents slices them by the engine's
    capacity): float64 [rows][L]."""
    z = np.random.RandomState(int(seed or 0)).normal(size=(int(rows), int(dim_z))).astype(np.float32)
    return np.asarray(generator.map_latents(z), dtype=np.float64)


def build(generator, config):
    """(mean, components, stdev) for the config: subspace_samples (default problem.PROBE_ROWS = 4096) rows of z from config.seed through
    generator.map_latents, then pca_basis with subspace_components (default 64, capped at dim_z)."""
    from .problem import PROBE_ROWS
    N = getattr(config, "subspace_samples", None)
    K = components_of(config)
    return pca_basis(probe(generator, getattr(config, "seed", 0), PROBE_ROWS if N is None else int(N), config.dim_z), K)


def row_width(config):
    """Floats per population row of latent space "sub" for a config: G * K of config.subspace_shape — what the Generator settled on — or,
    before a Generator exists, of the config's own keys (the spec's groups over the channel table's style layers, components_of)."""
    shape = getattr(config, "subspace_shape", None)
    if shape is not None:
        return int(shape[0]) * int(shape[1])
    from .latent import stylegan2_n_lat
    return n_groups(parse_layer_groups(getattr(config, "subspace_layers", None), stylegan2_n_lat(config))) * components_of(config)


def components_of(config):
    """K of a config: subspace_components, default 64, capped at dim_z."""
    K = getattr(config, "subspace_components", None)
    return min(DEFAULT_COMPONENTS if K is None else int(K), int(config.dim_z))
