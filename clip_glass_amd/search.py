"""Native search driver: GA (single objective) and NSGA-II (two objectives) with the operator
set the reference configures through pymoo 0.4.2.1 (run.py:59-76, operators.py:37-81):
simulated binary crossover (eta 3, prob 1.0), polynomial mutation (eta 3, per-variable prob 0.5),
binary tournament mating, duplicate elimination, fitness / rank-and-crowding survival.

pymoo is not vendored by the reference and is not installable here (its 0.4.2.1 release breaks
on numpy >= 1.24), so this is a restatement of the published algorithms (Deb et al. 2002; Deb &
Agrawal 1995), statistically — not bit — equivalent to pymoo's (parity unpinned).
It lets `python -m clip_glass_amd.run` work end-to-end without pymoo and gives every rank of a
multi-GPU job the same population (same seed => identical GA state, no broadcast needed).
"""
import numpy as np


# ----------------------------- variation operators --------------------------------------
def sbx(rng, pa, pb, xl, xu, eta=3.0, prob=1.0, prob_var=0.5):
    """Bounded simulated binary crossover of parent matrices pa, pb [n, n_var] -> two children each."""
    n, nv = pa.shape
    ca, cb = pa.copy(), pb.copy()
    do_cross = rng.random(n) < prob
    for i in np.nonzero(do_cross)[0]:
        for j in range(nv):
            if rng.random() > prob_var or abs(pa[i, j] - pb[i, j]) < 1e-14:
                continue
            y1, y2 = min(pa[i, j], pb[i, j]), max(pa[i, j], pb[i, j])
            u = rng.random()

            def child(beta_bound):
                alpha = 2.0 - beta_bound ** -(eta + 1.0)
                if u <= 1.0 / alpha:
                    return (u * alpha) ** (1.0 / (eta + 1.0))
                return (1.0 / (2.0 - u * alpha)) ** (1.0 / (eta + 1.0))
            b1 = child(1.0 + 2.0 * (y1 - xl[j]) / (y2 - y1))
            b2 = child(1.0 + 2.0 * (xu[j] - y2) / (y2 - y1))
            c1 = min(max(0.5 * ((y1 + y2) - b1 * (y2 - y1)), xl[j]), xu[j])
            c2 = min(max(0.5 * ((y1 + y2) + b2 * (y2 - y1)), xl[j]), xu[j])
            if rng.random() < 0.5:
                c1, c2 = c2, c1
            ca[i, j], cb[i, j] = c1, c2
    return ca, cb


def sbx_vectorised(rng, pa, pb, xl, xu, eta=3.0, prob=1.0, prob_var=0.5):
    """Same operator, whole-population numpy form (used by the driver)."""
    n, nv = pa.shape
    y1, y2 = np.minimum(pa, pb), np.maximum(pa, pb)
    d = np.maximum(y2 - y1, 1e-300)
    u = rng.random((n, nv))

    def betaq(bound):
        alpha = 2.0 - bound ** -(eta + 1.0)
        return np.where(u <= 1.0 / alpha, (u * alpha) ** (1.0 / (eta + 1.0)),
                        (1.0 / np.maximum(2.0 - u * alpha, 1e-300)) ** (1.0 / (eta + 1.0)))
    c1 = np.clip(0.5 * ((y1 + y2) - betaq(1.0 + 2.0 * (y1 - xl) / d) * d), xl, xu)
    c2 = np.clip(0.5 * ((y1 + y2) + betaq(1.0 + 2.0 * (xu - y2) / d) * d), xl, xu)
    swap = rng.random((n, nv)) < 0.5
    c1, c2 = np.where(swap, c2, c1), np.where(swap, c1, c2)
    active = (rng.random((n, 1)) < prob) & (rng.random((n, nv)) < prob_var) & ((y2 - y1) > 1e-14)
    return np.where(active, c1, pa), np.where(active, c2, pb)


def polynomial_mutation(rng, x, xl, xu, eta=3.0, prob=0.5):
    """Bounded polynomial mutation, per-variable probability `prob`."""
    n, nv = x.shape
    span = xu - xl
    d1, d2 = (x - xl) / span, (xu - x) / span
    u = rng.random((n, nv))
    mpow = 1.0 / (eta + 1.0)
    lo = (2.0 * u + (1.0 - 2.0 * u) * (1.0 - d1) ** (eta + 1.0)) ** mpow - 1.0
    hi = 1.0 - (2.0 * (1.0 - u) + 2.0 * (u - 0.5) * (1.0 - d2) ** (eta + 1.0)) ** mpow
    y = np.clip(x + np.where(u <= 0.5, lo, hi) * span, xl, xu)
    return np.where(rng.random((n, nv)) < prob, y, x)


def hux(rng, pa, pb, prob=0.2, prob_hux=0.5):
    """Half-uniform crossover on boolean matrices (pymoo "bin_hux"): with probability `prob` per mating,
    exchange ceil(prob_hux * #differing) randomly chosen differing bits."""
    ca, cb = pa.copy(), pb.copy()
    for i in np.nonzero(rng.random(pa.shape[0]) < prob)[0]:
        diff = np.nonzero(pa[i] != pb[i])[0]
        n = int(np.ceil(len(diff) * prob_hux))
        if n:
            sw = rng.permutation(diff)[:n]
            ca[i, sw], cb[i, sw] = pb[i, sw], pa[i, sw]
    return ca, cb


def bitflip(rng, x, prob=0.01):
    """pymoo "bin_bitflip": flip every bit independently with probability `prob`."""
    flip = rng.random(x.shape) < prob
    return np.where(flip, 1.0 - x, x)


def vary(rng, A, B, xl, xu, mask, eta_c, eta_m, prob_m, n_off):
    """Crossover + mutation for a (possibly mixed-variable) population: real / int columns get SBX + polynomial
    mutation (int: rounded, as pymoo's int_sbx / int_pm do), bool columns HUX + bit-flip
    (operators.py:38-63 MixedVariable* with the reference's probabilities)."""
    mask = np.asarray(mask)
    num = mask != "bool"
    ca, cb = A.copy(), B.copy()
    if num.any():
        ca[:, num], cb[:, num] = sbx_vectorised(rng, A[:, num], B[:, num], xl[num], xu[num], eta_c)
    if (~num).any():
        ca[:, ~num], cb[:, ~num] = hux(rng, A[:, ~num], B[:, ~num], 0.2)
    off = np.concatenate([ca, cb])[rng.permutation(2 * A.shape[0])[:n_off]]
    if num.any():
        off[:, num] = polynomial_mutation(rng, off[:, num], xl[num], xu[num], eta_m, prob_m)
    if (~num).any():
        off[:, ~num] = bitflip(rng, off[:, ~num], 10 / 1000)
    ints = mask == "int"
    if ints.any():
        off[:, ints] = np.clip(np.rint(off[:, ints]), xl[ints], xu[ints])
    return off


# ----------------------------- NSGA-II machinery ------------------------------------------
def fast_non_dominated_sort(F):
    n = F.shape[0]
    dom = (np.all(F[:, None, :] <= F[None, :, :], axis=2) & np.any(F[:, None, :] < F[None, :, :], axis=2))
    n_dominating = dom.sum(axis=0)          # how many dominate j
    rank = np.full(n, -1)
    fronts, current, r = [], np.nonzero(n_dominating == 0)[0], 0
    while current.size:
        rank[current] = r
        fronts.append(current)
        n_dominating = n_dominating - dom[current].sum(axis=0)
        n_dominating[rank >= 0] = -1
        current = np.nonzero(n_dominating == 0)[0]
        r += 1
    return fronts, rank


def crowding_distance(F):
    n, m = F.shape
    if n <= 2:
        return np.full(n, np.inf)
    cd = np.zeros(n)
    for k in range(m):
        order = np.argsort(F[:, k], kind="mergesort")
        f = F[order, k]
        span = f[-1] - f[0]
        cd[order[0]] = cd[order[-1]] = np.inf
        if span > 0:
            cd[order[1:-1]] += (f[2:] - f[:-2]) / span
    return cd


def _eliminate_duplicates(X, ref=None, eps=1e-16):
    keep = np.ones(X.shape[0], bool)
    for i in range(X.shape[0]):
        if not keep[i]:
            continue
        d = np.abs(X[i + 1:] - X[i]).max(axis=1) if i + 1 < X.shape[0] else np.zeros(0)
        keep[i + 1:] &= d > eps
    if ref is not None and ref.size:
        keep &= np.abs(X[:, None, :] - ref[None, :, :]).max(axis=2).min(axis=1) > eps
    return keep


class Individual:
    def __init__(self, X, F):
        self.X, self.F = X, F


class Result:
    pass


DEVICE_MAX_POP = 1024      # include/glass.h "Device search": survival ranks 2 pop merged rows in one workgroup
DEVICE_PROB_HUX, DEVICE_PROB_FLIP = 0.2, 10 / 1000      # what vary() above gives hux and bitflip (operators.py:50-58), for a mixed device search


class _DeviceAlgorithm:
    """What a callback sees of a device search: `pop` is read back from the device only when something asks for it."""

    def __init__(self, problem, engine, nsga):
        self.problem, self._engine, self._nsga, self.n_gen = problem, engine, nsga, 0

    @property
    def pop(self):
        r = self._engine.search_read("X", "F")
        return _individuals(r["X"].astype(float), r["F"].astype(float), self._nsga)


def _individuals(X, F, nsga):
    return [Individual(x, f if nsga else f[0]) for x, f in zip(X, F)]


def _result(X, F, nsga):
    res = Result()
    res.pop = _individuals(X, F, nsga)
    if nsga:
        front = fast_non_dominated_sort(F)[0][0]
        res.X, res.F = X[front], F[front]
    else:
        best = int(np.argmin(F[:, 0]))
        res.X, res.F = X[best], F[best]
    res.G = np.zeros(np.atleast_2d(res.X).shape[0])
    res.CV = np.zeros(np.atleast_2d(res.X).shape[0])
    return res


def _device_initial(problem, sampling, pop_size, seed):
    """Generation 0 of a device search under `seed`: sampled, de-duplicated and refilled to exactly pop_size rows."""
    np.random.seed(seed)   # the reference's Sampling classes draw from numpy's global RNG (operators.py:24-25)
    X = np.asarray(sampling._do(problem, pop_size), dtype=float)
    X = X[_eliminate_duplicates(X)]
    for _ in range(16):    # exactly pop_size rows: refill from the sampler where elimination shrank the population
        if X.shape[0] >= pop_size:
            break
        X = np.concatenate([X, np.asarray(sampling._do(problem, pop_size - X.shape[0]), dtype=float)])
        X = X[_eliminate_duplicates(X)]
    if X.shape[0] != pop_size:
        raise ValueError("device search: the sampler keeps returning duplicate rows: %d distinct of %d" % (X.shape[0], pop_size))
    return X


def _island_result(X, F, nsga, islands, pop_size, own_prompts):
    """The Result of an island search from its rows, island-major: islands[i] is island i's Result; X / F / pop are the best row (GA) or the
    non-dominated front (NSGA-II) of the union where the islands share one objective, and island 0's where each has its own prompt."""
    per = [_result(X[i * pop_size:(i + 1) * pop_size], F[i * pop_size:(i + 1) * pop_size], nsga) for i in range(islands)]
    res = _result(X[:pop_size], F[:pop_size], nsga) if own_prompts else _result(X, F, nsga)
    res.islands = per
    return res


def _minimize_device(problem, algorithm, pop_size, n_gen, sampling, seed, callback, eta_c, eta_m, prob_m, verbose, mask, islands=1,
                     migrate_every=0, migrants=1):
    """The generation step on the device (include/glass.h "Device search"): generation 0 is sampled, de-duplicated and refilled on the host
    as below, then every generation is one engine.search_step and a read of F.  Refusals come first and name their reason.
    islands > 1 ("Device search: islands"): generation 0 of island i is what this function samples under seed + i; the engine must have been
    set up for the same islands, migrate_every and migrants (Engine.set_search_islands before finalize)."""
    mask = np.asarray(["real"] * problem.n_var if mask is None else list(mask))
    n_real = None      # a mixed search: the real columns in front of the bits
    if (mask != "real").any():
        others = sorted(set(mask[mask != "real"].tolist()))
        if others != ["bool"]:
            raise ValueError("device search: the variables must be real, or real followed by bool, and this mask has %s ones (GPT2's int tokens "
                             "use the integer operators and are scored through the host tokenizer): they keep the host search" % " / ".join(others))
        n_real = int((mask == "real").sum())
        if n_real == 0 or (mask[:n_real] != "real").any():
            raise ValueError("device search: a mixed row is its real columns followed only by its bool columns (a BigGAN row: [z | class "
                             "bits]); this mask has a bool column in front of a real one: it keeps the host search")
        have = getattr(getattr(problem, "engine", None), "search_n_real", None)
        if have != n_real:
            raise ValueError("device search: this mask has %d real columns followed by %d bool ones, and the engine's search was set up for %s: "
                             "Engine.set_search_mixed(..., n_real=%d, ...) before finalize (config.device_search = True on a BigGAN config does it)"
                             % (n_real, mask.size - n_real, "all-real rows" if have is None else "%d real columns" % have, n_real))
    ranks = int(getattr(problem, "ranks", 1) or 1)
    if ranks > 1:
        raise ValueError("device search: %d ranks (--dist): the multi-rank wiring is not built yet; run one rank, or the host search" % ranks)
    bs = int(getattr(getattr(problem, "config", None), "batch_size", 1))
    if pop_size > DEVICE_MAX_POP:
        raise ValueError("device search: pop_size %d is over %d, the most the survival kernel ranks" % (pop_size, DEVICE_MAX_POP))
    if pop_size < 2 or pop_size % bs:
        raise ValueError("device search: pop_size %d must be a multiple of batch_size %d (the shapes on the device are static)" % (pop_size, bs))
    engine = getattr(problem, "engine", None)
    if engine is None:
        raise ValueError("device search: this problem has no engine to keep the population on (GenerationProblem has one)")
    xl, xu = np.unique(np.asarray(problem.xl, float)), np.unique(np.asarray(problem.xu, float))
    if xl.size != 1 or xu.size != 1:
        raise ValueError("device search: the bounds must be scalar (one xl and one xu for every variable), as the reference's are")
    if algorithm not in ("ga", "nsga2"):
        raise ValueError("device search: unknown algorithm %r" % (algorithm,))
    if getattr(engine, "search_pop", None) != pop_size:
        raise ValueError("device search: the engine was built without it, or for another pop_size (its buffers are sized in finalize): set "
                         "config.device_search = True (run.py --device-search) before the problem is constructed")
    nsga = algorithm == "nsga2"
    have_islands = getattr(engine, "search_islands", None)
    if islands != (have_islands or 1) or (islands > 1 and have_islands is None):
        raise ValueError("device search: islands=%d, and the engine's search was set up %s (its buffers are sized in finalize): "
                         "Engine.set_search_islands(%d, migrate_every, migrants) before finalize (config.islands does it)"
                         % (islands, "without islands" if have_islands is None else "for %d" % have_islands, islands))
    if have_islands is None:
        X = _device_initial(problem, sampling, pop_size, seed)
    else:
        X = np.concatenate([_device_initial(problem, sampling, pop_size, seed + i) for i in range(islands)])
    if n_real is None:
        engine.set_search_operators(float(xl[0]), float(xu[0]), eta_c, eta_m, prob_m, seed)
    else:
        engine.set_search_operators_mixed(float(xl[0]), float(xu[0]), eta_c, eta_m, prob_m, DEVICE_PROB_HUX, DEVICE_PROB_FLIP, seed)
    engine.search_init(X)
    generator = getattr(problem, "generator", None)
    algo = _DeviceAlgorithm(problem, engine, nsga)
    for gen in range(1, n_gen + 1):
        engine.search_step(gen)
        if generator is not None:
            generator.generation = gen + 1      # what the host search's evaluate() calls leave behind: the save callback's noise stream
        algo.n_gen = gen
        if verbose:
            F = engine.search_read("F")["F"]
            print("gen %4d | n_eval %6d | best %s" % (gen, gen * pop_size * islands, np.array2string(F.min(axis=0), precision=5)))
        if callback is not None:
            callback(algo)
    r = engine.search_read("X", "F")
    if have_islands is None:
        return _result(r["X"].astype(float), r["F"].astype(float), nsga)
    own = getattr(getattr(problem, "generator", None), "island_weights", None) is not None
    return _island_result(r["X"].astype(float), r["F"].astype(float), nsga, islands, pop_size, own)


# ----------------------------- separable CMA-ES --------------------------------------------
# include/glass.h "Device search: sep-CMA-ES" is the rule; this is its float64 host form, and csrc/cmaes.hip its device form.
CMA_MIN_POP, CMA_BLOCK, CMA_INIT_ROWS, DEFAULT_CMA_SIGMA = 4, 256, 4096, 1.0


def cma_constants(lam, n):
    """The weights and constants of the header's "Setup" for lam rows of n variables."""
    mu = lam // 2
    w = np.log(mu + 0.5) - np.log(np.arange(1, mu + 1, dtype=float))
    w = w / w.sum()
    me = 1.0 / (w * w).sum()
    c_sigma = (me + 2.0) / (n + me + 5.0)
    d_sigma = 1.0 + 2.0 * max(0.0, np.sqrt((me - 1.0) / (n + 1.0)) - 1.0) + c_sigma
    c_c = (4.0 + me / n) / (n + 4.0 + 2.0 * me / n)
    c_1 = 2.0 / ((n + 1.3) ** 2 + me)
    c_mu = min(1.0 - c_1, 2.0 * (me - 2.0 + 1.0 / me) / ((n + 2.0) ** 2 + me))
    c_1 = min(1.0, c_1 * (n + 2.0) / 3.0)
    c_mu = min(1.0 - c_1, c_mu * (n + 2.0) / 3.0)
    chi = np.sqrt(float(n)) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n))
    return dict(mu=mu, w=w, mu_eff=me, c_sigma=c_sigma, d_sigma=d_sigma, c_c=c_c, c_1=c_1, c_mu=c_mu, chi=chi)


def cma_rank(F):
    """(order, finite): the rows by (F, index) — -0.0 ties 0.0, a non-finite F goes last by index — and how many are finite."""
    F = np.asarray(F, float).reshape(-1) + 0.0
    fin = np.nonzero(np.isfinite(F))[0]
    return np.concatenate([fin[np.argsort(F[fin], kind="stable")], np.nonzero(~np.isfinite(F))[0]]), fin.size


class CMAState:
    """m, d, p_sigma, p_c float64 [n], sigma, and the best row seen with its F; `skipped` counts generations with fewer than mu finite rows."""

    def __init__(self, mean, diag, sigma):
        self.m, self.d = np.array(mean, dtype=float), np.array(diag, dtype=float)
        self.ps, self.pc = np.zeros_like(self.m), np.zeros_like(self.m)
        self.sigma, self.ps_norm, self.h, self.skipped, self.updates = float(sigma), 0.0, 0, 0, 0
        self.best_X, self.best_F = np.zeros(self.m.size, np.float32), np.inf


def cma_sample(state, lam, xl, xu, seed, generation):
    """The generation's rows, float32 [lam, n]: clip(m + (sigma sqrt(d)) z) in double, rounded once."""
    from .synth import search_normals
    z = search_normals(seed, generation, np.arange(lam)[:, None], np.arange(state.m.size)[None, :])
    return np.minimum(np.maximum(state.m + (state.sigma * np.sqrt(state.d)) * z, xl), xu).astype(np.float32)


def cma_update(state, c, X, F, xl, xu, generation):
    """Rank and update from the rows as they were evaluated (X float32 [lam, n], F [lam]); False: fewer than mu finite rows, nothing moved."""
    order, finite = cma_rank(F)
    if finite < c["mu"]:
        state.skipped += 1
        return False
    state.updates += 1
    if F[order[0]] < state.best_F:
        state.best_X, state.best_F = X[order[0]].copy(), float(F[order[0]])
    n, w = state.m.size, c["w"]
    yw, s2 = np.zeros(n), np.zeros(n)
    for i in range(c["mu"]):                     # the order i = 1 .. mu, one writer per variable
        y = (X[order[i]].astype(float) - state.m) / state.sigma
        yw = yw + w[i] * y
        s2 = s2 + w[i] * (y * y)
    state.m = state.m + state.sigma * yw
    state.ps = (1.0 - c["c_sigma"]) * state.ps + np.sqrt(c["c_sigma"] * (2.0 - c["c_sigma"]) * c["mu_eff"]) * yw / np.sqrt(state.d)
    sq, acc = state.ps * state.ps, 0.0
    for b in range(0, n, CMA_BLOCK):             # parts of 256 variables in index order (cumsum adds sequentially), then the parts in order
        acc = acc + np.cumsum(sq[b:b + CMA_BLOCK])[-1]
    norm = np.sqrt(acc)
    h = 1.0 if norm / np.sqrt(1.0 - np.power(1.0 - c["c_sigma"], 2.0 * (generation + 1.0))) < (1.4 + 2.0 / (n + 1.0)) * c["chi"] else 0.0
    state.pc = (1.0 - c["c_c"]) * state.pc + (h * np.sqrt(c["c_c"] * (2.0 - c["c_c"]) * c["mu_eff"])) * yw
    state.d = (((1.0 - c["c_1"]) - c["c_mu"]) * state.d + c["c_1"] * (state.pc * state.pc + (((1.0 - h) * c["c_c"]) * (2.0 - c["c_c"])) * state.d)
               + c["c_mu"] * s2)
    sigma = state.sigma * np.exp(min(1.0, (c["c_sigma"] / c["d_sigma"]) * (norm / c["chi"] - 1.0)))
    state.sigma, state.ps_norm, state.h = float(min(max(sigma, 1e-10), xu - xl)), float(norm), int(h)
    return True


def _cma_checks(problem, pop_size, mask):
    """What "cmaes" refuses, by name, on the host and on the device; returns the scalar bounds."""
    if int(problem.n_obj) != 1:
        raise ValueError("cmaes: minimises one objective and this problem has n_obj = %d: use nsga2 (or a _nod config, or the LPIPS / anchor "
                         "distance folded in with lambda > 0)" % problem.n_obj)
    if mask is not None and (np.asarray(list(mask)) != "real").any():
        others = sorted(set(np.asarray(list(mask))[np.asarray(list(mask)) != "real"].tolist()))
        raise ValueError("cmaes: samples real-valued rows and this mask has %s columns (BigGAN's class bits, GPT2's tokens): use ga" % " / ".join(others))
    if pop_size < CMA_MIN_POP:
        raise ValueError("cmaes: pop_size %d is under %d (mu = pop / 2 >= 2 rows recombine)" % (pop_size, CMA_MIN_POP))
    xl, xu = np.unique(np.asarray(problem.xl, float)), np.unique(np.asarray(problem.xu, float))
    if xl.size != 1 or xu.size != 1:
        raise ValueError("cmaes: the bounds must be scalar (one xl and one xu for every variable), as the reference's are")
    return float(xl[0]), float(xu[0])


def cma_initial(problem, sampling, seed, mean=None, diag=None, sigma=None):
    """(m0, d0, sigma0): what is not given comes from CMA_INIT_ROWS rows of the search's own sampling under np.random.seed(seed) — their column
    mean and variance — and sigma0 from the problem's config (cma_sigma, default 1): in z, generation 0 is then the reference's distribution."""
    if mean is None or diag is None:
        np.random.seed(seed)
        S = np.asarray(sampling._do(problem, CMA_INIT_ROWS), dtype=float)
        mean = S.mean(axis=0) if mean is None else mean
        diag = S.var(axis=0) if diag is None else diag
    mean, diag = np.broadcast_to(np.asarray(mean, float), (problem.n_var,)).copy(), np.broadcast_to(np.asarray(diag, float), (problem.n_var,)).copy()
    if not (np.isfinite(mean).all() and np.isfinite(diag).all() and (diag > 0).all()):
        raise ValueError("cmaes: the initial mean must be finite and the initial variances finite and positive (a sampling that never moves a "
                         "column gives it no scale)")
    if sigma is None:
        sigma = getattr(getattr(problem, "config", None), "cma_sigma", None)
    sigma = DEFAULT_CMA_SIGMA if sigma is None else float(sigma)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("cmaes: cma_sigma must be finite and positive, got %r" % (sigma,))
    return mean, diag, sigma


def _cma_result(X, F, best_X, best_F, mean, sigma):
    res = Result()
    res.pop = _individuals(np.asarray(X, float), np.asarray(F, float).reshape(-1, 1), False)
    res.X, res.F = np.asarray(best_X, float), np.array([best_F], float)
    res.mean, res.sigma = np.asarray(mean, float), float(sigma)
    res.G, res.CV = np.zeros(1), np.zeros(1)
    return res


def _minimize_cmaes(problem, pop_size, n_gen, sampling, seed, callback, verbose, mask, init):
    """Generations 0 .. n_gen of the rule on the host: (n_gen + 1) pop_size evaluations, the GA's count."""
    xl, xu = _cma_checks(problem, pop_size, mask)
    state = CMAState(*cma_initial(problem, sampling, seed, *init))
    c = cma_constants(pop_size, problem.n_var)
    algo = Result()
    algo.problem, algo.state = problem, state
    for gen in range(n_gen + 1):
        X = cma_sample(state, pop_size, xl, xu, seed, gen)
        out = {}
        problem._evaluate(X.astype(float), out)
        F = np.asarray(out["F"], dtype=float).reshape(pop_size, -1)[:, 0]
        cma_update(state, c, X, F, xl, xu, gen)
        algo.pop, algo.n_gen = _individuals(X.astype(float), F.reshape(-1, 1), False), gen
        if verbose:
            print("gen %4d | n_eval %6d | best %.5g | sigma %.3g" % (gen, (gen + 1) * pop_size, state.best_F, state.sigma))
        if callback is not None and gen >= 1:
            callback(algo)
    res = _cma_result(X, F, state.best_X, state.best_F, state.m, state.sigma)
    res.state = state
    return res


class _DeviceCMA:
    """What a callback sees of a device CMA search: `pop` is the generation's rows and F, read back only when something asks for it."""

    def __init__(self, problem, engine):
        self.problem, self._engine, self.n_gen = problem, engine, 0

    @property
    def pop(self):
        r = self._engine.search_read("off_X", "off_F")
        return _individuals(r["off_X"].astype(float), r["off_F"].astype(float), False)


def _minimize_cmaes_device(problem, pop_size, n_gen, sampling, seed, callback, verbose, mask, init):
    """The same generations on the problem's engine: every generation is one engine.search_step (sample, the pass, rank, update)."""
    xl, xu = _cma_checks(problem, pop_size, mask)
    ranks = int(getattr(problem, "ranks", 1) or 1)
    if ranks > 1:
        raise ValueError("device search: %d ranks (--dist): the multi-rank wiring is not built yet; run one rank, or the host search" % ranks)
    bs = int(getattr(getattr(problem, "config", None), "batch_size", 1))
    if pop_size > DEVICE_MAX_POP or pop_size % bs:
        raise ValueError("device search: pop_size %d must be a multiple of batch_size %d and at most %d" % (pop_size, bs, DEVICE_MAX_POP))
    engine = getattr(problem, "engine", None)
    if engine is None:
        raise ValueError("device search: this problem has no engine to keep the distribution on (GenerationProblem has one)")
    if getattr(engine, "search_pop", None) != pop_size or getattr(engine, "search_algorithm", None) != "cmaes":
        raise ValueError("device search: the engine was built without it, for another pop_size or for another algorithm (its buffers are sized in "
                         "finalize): set config.device_search = True and config.algorithm = \"cmaes\" before the problem is constructed")
    m0, d0, s0 = cma_initial(problem, sampling, seed, *init)
    engine.set_search_operators(xl, xu, seed=seed)
    engine.search_init_cma(m0, d0, s0)
    generator = getattr(problem, "generator", None)
    algo = _DeviceCMA(problem, engine)
    for gen in range(n_gen + 1):
        engine.search_step(gen)
        if generator is not None:
            generator.generation = gen + 1      # what the host search's evaluate() calls leave behind: the save callback's noise stream
        algo.n_gen = gen
        if verbose:
            c = engine.search_read_cma()
            print("gen %4d | n_eval %6d | best %.5g | sigma %.3g" % (gen, (gen + 1) * pop_size, c["best_F"], c["sigma"]))
        if callback is not None and gen >= 1:
            callback(algo)
    r, c = engine.search_read("off_X", "off_F"), engine.search_read_cma()
    res = _cma_result(r["off_X"], r["off_F"][:, 0], c["best_X"], c["best_F"], c["mean"], c["sigma"])
    res.state = c
    return res


def minimize(problem, algorithm, pop_size, n_gen, sampling, seed=1, callback=None, eta_c=3.0, eta_m=3.0,
             prob_m=0.5, verbose=False, mask=None, device=False, cma_mean=None, cma_diag=None, cma_sigma=None, islands=1, migrate_every=0,
             migrants=1):
    """pymoo.optimize.minimize(problem, algorithm, ("n_gen", n_gen)) stand-in.

    problem: has n_var, n_obj, xl, xu and _evaluate(x, out) (GenerationProblem);
    algorithm: "ga" | "nsga2" | "cmaes"; sampling: object with _do(problem, n) (operators.get_operators);
    mask: per-variable type "real" | "int" | "bool" (None = all real) — the BigGAN configs mix real z with
    boolean class bits (operators.py:39), the GPT2 config is all-int.
    device=True (opt-in; real-valued StyleGAN2 searches and the BigGAN configs' [real | bool] rows, on one rank): selection, variation, duplicate flags and survival run on the
    problem's engine between the passes (include/glass.h "Device search"); the result has the same shapes.
    algorithm "cmaes" (opt-in): separable CMA-ES (include/glass.h "Device search: sep-CMA-ES") — one objective, real variables, scalar bounds;
    generations 0 .. n_gen of pop_size rows, the callback after generations 1 .. n_gen.  cma_mean / cma_diag / cma_sigma: the initial
    distribution (default: cma_initial).  The Result has X / F = the best row seen, pop = the last generation, and mean and sigma.
    islands=K (opt-in, device=True and "ga" / "nsga2" only; include/glass.h "Device search: islands"): K populations of pop_size rows in the
    problem's engine, island i under seed + i, with ring migration of `migrants` rows every `migrate_every` generations (0: never).
    res.islands[i] is island i's Result; res.X / res.F / res.pop are the best row (GA) or the non-dominated front (NSGA-II) of the union —
    or island 0's, where each island has its own prompt."""
    islands = int(islands)
    if islands < 1:
        raise ValueError("islands must be >= 1, got %d" % islands)
    if islands > 1 and algorithm == "cmaes":
        raise ValueError("islands=%d with algorithm cmaes: it keeps one distribution, not populations; islands of distributions are a "
                         "different feature: use ga or nsga2" % islands)
    if islands > 1 and not device:
        raise ValueError("islands=%d without device=True: the host search has no islands (they are populations of the device search)" % islands)
    if algorithm == "cmaes":
        run = _minimize_cmaes_device if device else _minimize_cmaes
        return run(problem, pop_size, n_gen, sampling, seed, callback, verbose, mask, (cma_mean, cma_diag, cma_sigma))
    if device:
        return _minimize_device(problem, algorithm, pop_size, n_gen, sampling, seed, callback, eta_c, eta_m, prob_m, verbose, mask, islands,
                                migrate_every, migrants)
    rng = np.random.default_rng(seed)
    np.random.seed(seed)   # the reference's Sampling classes draw from numpy's global RNG (operators.py:24-25)
    xl = np.broadcast_to(np.asarray(problem.xl, float), (problem.n_var,))
    xu = np.broadcast_to(np.asarray(problem.xu, float), (problem.n_var,))
    nsga = algorithm == "nsga2"
    mask = np.asarray(["real"] * problem.n_var if mask is None else list(mask))

    def evaluate(X):
        out = {}
        problem._evaluate(X, out)
        F = np.asarray(out["F"], dtype=float)
        return F.reshape(X.shape[0], -1)

    def survive(X, F, n):
        if not nsga:
            order = np.argsort(F[:, 0], kind="mergesort")[:n]
            return X[order], F[order], np.zeros(len(order), int), -F[order, 0]
        fronts, rank = fast_non_dominated_sort(F)
        chosen, cds = [], []
        for fr in fronts:
            cd = crowding_distance(F[fr])
            if len(chosen) + len(fr) > n:
                order = np.argsort(-cd, kind="mergesort")[: n - len(chosen)]
                fr, cd = fr[order], cd[order]
            chosen.extend(fr.tolist())
            cds.extend(cd.tolist())
            if len(chosen) >= n:
                break
        chosen = np.array(chosen)
        return X[chosen], F[chosen], rank[chosen], np.array(cds)

    X = np.asarray(sampling._do(problem, pop_size), dtype=float)
    X = X[_eliminate_duplicates(X)]
    pad = (-X.shape[0]) % getattr(getattr(problem, "config", None), "batch_size", 1)
    if pad:   # SURVEY 8a note 8: the engine needs whole minibatches; refill instead of asserting
        X = np.concatenate([X, np.asarray(sampling._do(problem, pad), dtype=float)])
    F = evaluate(X)
    X, F, rank, cd = survive(X, F, pop_size)
    algo = Result()
    algo.problem = problem
    for gen in range(1, n_gen + 1):
        n = X.shape[0]
        # binary tournament: lower rank wins, then larger crowding distance (GA: better fitness)
        a, b = rng.integers(0, n, (2, pop_size)), rng.integers(0, n, (2, pop_size))
        better = (rank[a] < rank[b]) | ((rank[a] == rank[b]) & (cd[a] >= cd[b]))
        parents = np.where(better, a, b)
        off = vary(rng, X[parents[0]], X[parents[1]], xl, xu, mask, eta_c, eta_m, prob_m, pop_size)
        off = off[_eliminate_duplicates(off, X)]
        bs = getattr(getattr(problem, "config", None), "batch_size", 1)
        if off.shape[0] % bs:
            extra = bs - off.shape[0] % bs
            pick = rng.integers(0, n, (2, extra))
            off = np.concatenate([off, vary(rng, X[pick[0]], X[pick[1]], xl, xu, mask, eta_c, eta_m, 1.0, extra)])
        Fo = evaluate(off)
        X, F, rank, cd = survive(np.concatenate([X, off]), np.concatenate([F, Fo]), pop_size)
        algo.pop = [Individual(x, f if nsga else f[0]) for x, f in zip(X, F)]
        algo.n_gen = gen
        if verbose:
            print("gen %4d | n_eval %6d | best %s" % (gen, gen * pop_size, np.array2string(F.min(axis=0), precision=5)))
        if callback is not None:
            callback(algo)
    res = Result()
    res.pop = [Individual(x, f if nsga else f[0]) for x, f in zip(X, F)]
    if nsga:
        front = fast_non_dominated_sort(F)[0][0]
        res.X, res.F = X[front], F[front]
    else:
        best = int(np.argmin(F[:, 0]))
        res.X, res.F = X[best], F[best]
    res.G = np.zeros(np.atleast_2d(res.X).shape[0])
    res.CV = np.zeros(np.atleast_2d(res.X).shape[0])
    return res


def pseudo_weights_choice(F, weights=(0.0, 1.0)):
    """pymoo get_decision_making("pseudo-weights", w).do(F): index of the point whose pseudo-weight vector is closest to w."""
    F = np.asarray(F, float)
    span = F.max(axis=0) - F.min(axis=0)
    span[span == 0] = 1.0
    pw = (F.max(axis=0) - F) / span
    pw = pw / np.maximum(pw.sum(axis=1, keepdims=True), 1e-300)
    return int(np.argmin(np.linalg.norm(pw - np.asarray(weights, float), axis=1)))
