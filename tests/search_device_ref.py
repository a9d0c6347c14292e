"""Float64 mirror of the device search's rule (include/glass.h "Device search"; csrc/search.hip), driven by synth.search_uniforms.

Not a test module: tests/test_search_device_ref.py pins it to search.py's own operators, the GPU tests compare the kernels with it."""
import numpy as np

from clip_glass_amd import synth
from util import diag


def tournament(seed, generation, pop, rank, cd):
    """parents int [2, n_matings] and the contestants int [4, n_matings] of every mating of a generation (n_matings = ceil(pop / 2))."""
    m = np.arange((pop + 1) // 2, dtype=np.uint32)
    u = synth.search_uniforms(seed, generation, m, 0, synth.SEARCH_DRAW_TOURNAMENT)
    c = np.stack([np.minimum(np.floor(x * float(pop)).astype(np.int64), pop - 1) for x in u])
    rank, cd = np.asarray(rank), np.asarray(cd, np.float64)

    def better(a, b):
        return np.where((rank[a] < rank[b]) | ((rank[a] == rank[b]) & (cd[a] >= cd[b])), a, b)
    return np.stack([better(c[0], c[1]), better(c[2], c[3])]), c


def sbx_uniforms(seed, generation, n_matings, n_var):
    """(u, swap, gate) float64 [n_matings, n_var] each."""
    m = np.arange(n_matings, dtype=np.uint32)[:, None]
    j = np.arange(n_var, dtype=np.uint32)[None, :]
    u = synth.search_uniforms(seed, generation, m, j, synth.SEARCH_DRAW_SBX)
    return u[0], u[1], u[2]


def mutation_uniforms(seed, generation, rows, n_var):
    """(u, gate) float64 [len(rows), n_var] each, for the offspring rows `rows`."""
    r = np.asarray(rows, dtype=np.uint32)[:, None]
    j = np.arange(n_var, dtype=np.uint32)[None, :]
    u = synth.search_uniforms(seed, generation, r, j, synth.SEARCH_DRAW_MUTATION)
    return u[0], u[1]


def sbx(pa, pb, xl, xu, eta, u, swap_u, gate_u):
    """Both children of every mating (float64), and the decisions (active, swap)."""
    y1, y2 = np.minimum(pa, pb), np.maximum(pa, pb)
    d = np.maximum(y2 - y1, 1e-300)

    def betaq(bound):
        alpha = 2.0 - bound ** -(eta + 1.0)
        with np.errstate(all="ignore"):
            return np.where(u <= 1.0 / alpha, (u * alpha) ** (1.0 / (eta + 1.0)),
                            (1.0 / np.maximum(2.0 - u * alpha, 1e-300)) ** (1.0 / (eta + 1.0)))
    c1 = np.clip(0.5 * ((y1 + y2) - betaq(1.0 + 2.0 * (y1 - xl) / d) * d), xl, xu)
    c2 = np.clip(0.5 * ((y1 + y2) + betaq(1.0 + 2.0 * (xu - y2) / d) * d), xl, xu)
    swap = swap_u < 0.5
    active = (gate_u < 0.5) & ((y2 - y1) > 1e-14)
    ca = np.where(active, np.where(swap, c2, c1), pa)
    cb = np.where(active, np.where(swap, c1, c2), pb)
    return ca, cb, active, swap


def mutate(x, xl, xu, eta, prob, u, gate_u):
    span = xu - xl
    d1, d2 = (x - xl) / span, (xu - x) / span
    mpow = 1.0 / (eta + 1.0)
    with np.errstate(all="ignore"):
        lo = (2.0 * u + (1.0 - 2.0 * u) * (1.0 - d1) ** (eta + 1.0)) ** mpow - 1.0
        hi = 1.0 - (2.0 * (1.0 - u) + 2.0 * (u - 0.5) * (1.0 - d2) ** (eta + 1.0)) ** mpow
    y = np.clip(x + np.where(u <= 0.5, lo, hi) * span, xl, xu)
    do = gate_u < prob
    return np.where(do, y, x), do


def vary(X, rank, cd, xl, xu, eta_c, eta_m, prob_m, seed, generation):
    """The offspring of the fp32 population X [pop, n_var]: dict(off float64 [pop, n_var] BEFORE the rounding to fp32, off32 the rounded rows,
    parents [2, n_matings], contestants [4, n_matings], active / swap [n_matings, n_var], mutated [pop, n_var])."""
    X = np.asarray(X, np.float32).astype(np.float64)
    pop, nv = X.shape
    xl, xu = float(xl), float(xu)
    parents, contestants = tournament(seed, generation, pop, rank, cd)
    nm = parents.shape[1]
    u, su, gu = sbx_uniforms(seed, generation, nm, nv)
    ca, cb, active, swap = sbx(X[parents[0]], X[parents[1]], xl, xu, float(eta_c), u, su, gu)
    off = np.empty((2 * nm, nv))
    off[0::2], off[1::2] = ca, cb
    off = off[:pop]
    mu, mg = mutation_uniforms(seed, generation, np.arange(pop), nv)
    off, mutated = mutate(off, xl, xu, float(eta_m), float(prob_m), mu, mg)
    return dict(off=off, off32=off.astype(np.float32), parents=parents, contestants=contestants, active=active, swap=swap, mutated=mutated)


def duplicates(X, Xoff):
    """flags int32 [n_off]: the offspring row equals (by value) a population row or an offspring row below it."""
    X, Xoff = np.asarray(X, np.float32), np.asarray(Xoff, np.float32)
    flags = np.zeros(Xoff.shape[0], np.int32)
    for r in range(Xoff.shape[0]):
        hit = bool((X == Xoff[r]).all(axis=1).any()) if X.shape[0] else False
        if not hit and r:
            hit = bool((Xoff[:r] == Xoff[r]).all(axis=1).any())
        flags[r] = int(hit)
    return flags


def eligible(F, n_pop, flags=None):
    """(valid bool [N], counts (flagged, non-finite)) of the merged rows F float32 [N, n_obj]."""
    F = np.asarray(F, np.float32)
    N = F.shape[0]
    fin = np.isfinite(F).all(axis=1)
    flg = np.zeros(N, bool)
    if flags is not None and N > n_pop:
        flg[n_pop:] = np.asarray(flags) != 0
    valid = np.ones(N, bool)
    valid[n_pop:] = ~flg[n_pop:] & fin[n_pop:]
    return valid, (int(flg.sum()), int((~fin).sum()))


def survive(F, n_pop, pop_out, nsga=True, flags=None):
    """dict(chosen merged indices in survival order, rank, cd float64, counts) — written from the rule's text, not from search.py."""
    F32 = np.asarray(F, np.float32)
    Fd = F32.astype(np.float64)
    N, M = Fd.shape
    valid, counts = eligible(F32, n_pop, flags)
    idx = np.nonzero(valid)[0]
    if not nsga:
        order = idx[np.lexsort((idx, Fd[idx, 0]))][:pop_out]
        return dict(chosen=order.astype(np.int32), rank=np.zeros(len(order), np.int32), cd=-Fd[order, 0], counts=counts)
    rank = np.full(N, -1)
    left = list(idx)
    r, ranked = 0, 0
    fronts = []
    while left and ranked < pop_out:
        sub = Fd[left]
        dominated = np.zeros(len(left), bool)
        for a in range(len(left)):
            dominated |= (sub[a] <= sub).all(axis=1) & (sub[a] < sub).any(axis=1)
        front = [i for i, dm in zip(left, dominated) if not dm]
        for i in front:
            rank[i] = r
        fronts.append(np.array(front))
        left = [i for i, dm in zip(left, dominated) if dm]
        ranked += len(front)
        r += 1
    cd = np.zeros(N)
    for fr in fronts:
        if len(fr) <= 2:
            cd[fr] = np.inf
            continue
        for k in range(M):
            o = fr[np.lexsort((fr, Fd[fr, k]))]
            span = Fd[o[-1], k] - Fd[o[0], k]
            cd[o[0]] = cd[o[-1]] = np.inf
            if span > 0:
                cd[o[1:-1]] += (Fd[o[2:], k] - Fd[o[:-2], k]) / span
    chosen = []
    for fr in fronts:
        room = pop_out - len(chosen)
        if len(fr) > room:
            fr = fr[np.lexsort((fr, -cd[fr]))][:room]
        chosen.extend(int(i) for i in fr)
    chosen = np.array(chosen, np.int32)
    return dict(chosen=chosen, rank=rank[chosen].astype(np.int32), cd=cd[chosen], counts=counts)


def ulp32(v):
    """One fp32 ulp at magnitude v."""
    return float(np.spacing(np.float32(abs(v))))


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------------
def population_case(pop, nv, xl, xu, seed=3):
    """X float32 [pop, n_var] in [xl, xu] with a pair of equal rows (the 1e-14 gate) and rows on the bounds, rank int32, cd with infinities."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(xl, xu, (pop, nv)).astype(np.float32)
    X[1] = X[0]                      # equal parents: the 1e-14 gate
    X[2, ::2] = xl                   # parents on the bounds
    X[3, 1::2] = xu
    rank = rng.integers(0, 3, pop).astype(np.int32)
    cd = rng.uniform(0, 2, pop)
    cd[::3] = np.inf
    return X, rank, cd


def survive_cases(N, M, seed=0):
    """name -> (F float32 [N, M], flags or None): the cases of the issue at one merged size."""
    rng = np.random.default_rng(seed + 31 * N + M)
    n_pop = N // 2
    out = {}
    F = rng.standard_normal((N, M)).astype(np.float32)
    out["random"] = (F, None)
    if M >= 2:      # one front: column 0 rising, column 1 falling
        F1 = rng.standard_normal((N, M)).astype(np.float32)
        F1[:, 0] = np.arange(N)
        F1[:, 1] = -np.arange(N)
        out["one_front"] = (F1[rng.permutation(N)], None)
    chain = np.repeat(np.arange(N, dtype=np.float32)[:, None], M, axis=1)
    out["chain"] = (chain[rng.permutation(N)], None)          # every row dominates the next: N fronts (M = 1: a plain order)
    rep = rng.integers(0, 4, (N, M)).astype(np.float32)      # repeated F rows, tied values, zeros of both signs
    rep[rep == 0] *= np.where(rng.random((rep == 0).sum()) < 0.5, -1.0, 1.0)
    out["repeated"] = (rep, None)
    small = rng.standard_normal((N, M)).astype(np.float32) + 10
    small[0] = -5                                              # a front of one row
    if M >= 2:
        small[1], small[2] = 0, 0                              # then a front of two
        small[1, 0], small[2, 1] = -1, -1
    out["small_fronts"] = (small, None)
    bad = rng.standard_normal((N, M)).astype(np.float32)
    flags = np.zeros(N - n_pop, np.int32)
    flags[[0, 3]] = 1
    bad[n_pop + 1, 0] = np.nan
    bad[n_pop + 2, M - 1] = np.inf
    bad[n_pop + 3] = -100                                      # flagged AND the best row: still left out
    out["left_out"] = (bad, flags)
    if M >= 2:      # a last front that must be cut, with tied distances: an evenly spaced line behind a dominating block
        cut = np.zeros((N, M), np.float32)
        k = n_pop - 3
        cut[:k] = -50 - rng.random((k, M)).astype(np.float32)
        t = np.arange(N - k, dtype=np.float32)
        cut[k:, 0], cut[k:, 1] = t, -t
        out["cut_ties"] = (cut, None)
    return out


# ---- the comparisons both GPU test files make ---------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_offspring(name, got, X, m, xl, xu):
    """got float32 [rows, n_var] against the mirror's dict m (rows = every offspring row)."""
    ref = m["off32"]
    assert got.shape == ref.shape
    pop = got.shape[0]
    Xd = np.asarray(X, np.float32)
    untouched = ~np.repeat(m["active"], 2, axis=0)[:pop] & ~m["mutated"]
    parent = np.empty_like(ref)
    parent[0::2] = Xd[m["parents"][0]][: (pop + 1) // 2]
    parent[1::2] = Xd[m["parents"][1]][: pop // 2]
    wrong = int((bits(got)[untouched] != bits(parent)[untouched]).sum())
    ulp = ulp32(max(abs(xl), abs(xu)))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    worst = np.unravel_index(int(err.argmax()), err.shape)
    diag("%s: untouched variables %d (wrong bits %d), differing values %d of %d, worst %.3g = %.2f ulp at row %d var %d (mirror %r)"
         % (name, int(untouched.sum()), wrong, int((bits(got) != bits(ref)).sum()), ref.size, err.max(), err.max() / ulp, worst[0], worst[1],
            float(m["off"][worst])))
    assert untouched.any() and (~untouched).any()
    assert wrong == 0, "%s: %d variables the mirror leaves alone do not carry their parent's bits" % (name, wrong)
    assert err.max() <= 2 * ulp, "%s: worst |device - mirror| %.3g = %.2f ulp at row %d var %d" % (name, err.max(), err.max() / ulp, worst[0], worst[1])
    assert (got >= np.float32(xl)).all() and (got <= np.float32(xu)).all()


def check_survival(name, got, F, n_pop, pop_out, nsga, flags, X=None):
    ref = survive(F, n_pop, pop_out, nsga, flags)
    assert np.array_equal(got["chosen"], ref["chosen"]), "%s: chosen\n%r\n%r" % (name, got["chosen"], ref["chosen"])
    assert np.array_equal(got["rank"], ref["rank"]), name
    assert np.array_equal(got["cd"].view(np.uint64), ref["cd"].view(np.uint64)), "%s: distances\n%r\n%r" % (name, got["cd"], ref["cd"])
    assert tuple(got["counts"]) == ref["counts"], name
    assert np.array_equal(bits(got["F"]), bits(np.asarray(F, np.float32)[ref["chosen"]])), name
    if X is not None:
        assert np.array_equal(bits(got["X"]), bits(X[ref["chosen"]])), name
