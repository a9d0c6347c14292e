"""Numpy mirror of the island rule (include/glass.h "Device search: islands"; csrc/search.hip ga_migrate_kernel and the island dimension of every phase's kernel), built on
search_device_ref.py and search_mixed_ref.py: island i is the single search under seed + i on its own rows, and migrate() is the ring.

Not a test module: tests/test_search_islands_ref.py pins it to known answers and shows that its checker fails on planted faults; the GPU
tests compare the kernels with it."""
import numpy as np

import search_device_ref as SR
import search_mixed_ref as MR

FAULTS = ("reversed_ring", "reversed_order", "keep_duplicates", "no_rerank", "read_after_write")


def island_seed(seed, i):
    """Island i's Philox seed: seed + i, uint64, wrapping."""
    return (int(seed) + int(i)) & 0xFFFFFFFFFFFFFFFF


def order(rank, cd):
    """The rows of one island in the tournament's order (rank, -cd, index), best first."""
    rank, cd = np.asarray(rank), np.asarray(cd, np.float64)
    idx = np.arange(rank.shape[0])
    return idx[np.lexsort((idx, -cd, rank))]


def rows_equal(a, b):
    """By value in every variable: -0.0 equals 0.0 (and a NaN nothing)."""
    return bool((np.asarray(a, np.float32) == np.asarray(b, np.float32)).all())


def migrate(X, F, rank, cd, n, nsga=True, fault=None):
    """One ring migration of the islands X float32 [K, pop, n_var], F float32 [K, pop, n_obj], rank int [K, pop], cd float64 [K, pop] as
    survival left them -> dict(X, F, rank int32, cd, accepted int32 [K]) after it.  fault: one of FAULTS, a deliberately wrong rule (for the
    tests of the checker)."""
    assert fault is None or fault in FAULTS
    X0, F0 = np.array(X, np.float32), np.array(F, np.float32)
    K, pop, _ = X0.shape
    assert 1 <= n <= pop // 2
    r0, c0 = np.array(rank, np.int32), np.array(cd, np.float64)
    Xn, Fn, rn, cn = X0.copy(), F0.copy(), r0.copy(), c0.copy()
    accepted = np.zeros(K, np.int32)

    def rerank(i):
        s = SR.survive(Fn[i], pop, pop, nsga, None)
        ch = s["chosen"]
        Xn[i], Fn[i], rn[i], cn[i] = Xn[i][ch], Fn[i][ch], s["rank"], s["cd"]
    for i in range(K):
        src = (i + 1) % K if fault == "reversed_ring" else (i - 1 + K) % K
        # the rule reads every source as survival left it; the fault takes island by island what the islands before it have become
        SX, SF, Sr, Sc = (Xn, Fn, rn, cn) if fault == "read_after_write" else (X0, F0, r0, c0)
        best = order(Sr[src], Sc[src])[:n]
        if fault == "reversed_order":
            best = best[::-1]
        worst = order(r0[i], c0[i])[::-1][:n]
        cand = [SX[src, b].copy() for b in best]
        candF = [SF[src, b].copy() for b in best]
        for k in range(n):
            dup = any(rows_equal(cand[k], X0[i, c]) for c in range(pop)) or any(rows_equal(cand[k], cand[q]) for q in range(k))
            if dup and fault != "keep_duplicates":
                continue
            Xn[i, worst[k]], Fn[i, worst[k]] = cand[k], candF[k]
            accepted[i] += 1
        if fault == "read_after_write" and accepted[i]:
            rerank(i)
    for i in range(K):
        if accepted[i] and fault not in ("no_rerank", "read_after_write"):
            rerank(i)
    return dict(X=Xn, F=Fn, rank=rn, cd=cn, accepted=accepted)


def check_migration(name, got, X, F, rank, cd, n, nsga=True):
    """got: dict(X, F, rank, cd, accepted) against the mirror applied to the pre-state: exact, distances bitwise."""
    ref = migrate(X, F, rank, cd, n, nsga)
    assert np.array_equal(np.asarray(got["accepted"]).reshape(-1), ref["accepted"]), "%s: accepted %r, mirror %r" % (name, got["accepted"], ref["accepted"])
    assert np.array_equal(SR.bits(got["X"]), SR.bits(ref["X"])), "%s: X" % name
    assert np.array_equal(SR.bits(got["F"]), SR.bits(ref["F"])), "%s: F" % name
    assert np.array_equal(np.asarray(got["rank"], np.int32), ref["rank"]), "%s: rank\n%r\n%r" % (name, got["rank"], ref["rank"])
    assert np.array_equal(np.asarray(got["cd"], np.float64).view(np.uint64), ref["cd"].view(np.uint64)), "%s: cd\n%r\n%r" % (name, got["cd"], ref["cd"])
    return ref


def migration_due(generation, K, migrate_every):
    return K > 1 and migrate_every > 0 and generation >= 1 and generation % migrate_every == 0


def vary(X, rank, cd, xl, xu, eta_c, eta_m, prob_m, seed, generation, n_real=None, prob_x=0.2, prob_flip=0.01):
    """The offspring of every island of X [K, pop, n_var]: a list of K mirror dicts — search_device_ref.vary's (n_real None: all-real rows) or
    search_mixed_ref.vary_mixed's — island i under seed + i with local indices."""
    out = []
    for i in range(np.asarray(X).shape[0]):
        s = island_seed(seed, i)
        if n_real is None:
            out.append(SR.vary(X[i], rank[i], cd[i], xl, xu, eta_c, eta_m, prob_m, s, generation))
        else:
            out.append(MR.vary_mixed(X[i], n_real, rank[i], cd[i], xl, xu, eta_c, eta_m, prob_m, prob_x, prob_flip, s, generation))
    return out


def generation(state, evaluate, nsga, xl, xu, eta_c, eta_m, prob_m, seed, gen, migrate_every=0, migrants=1, n_real=None, prob_x=0.2,
               prob_flip=0.01):
    """One K-island generation of state = dict(X [K, pop, n_var] float32, F, rank, cd) under evaluate(rows float32 [R, n_var]) -> F float32
    [R, n_obj]: vary, ONE evaluation of all K pop offspring, survival per island, migration where due.  Returns (state after, dict(off_X,
    off_F, flags, counts [K, 2], accepted [K] or None))."""
    X, F, rank, cd = (np.asarray(state[k]) for k in ("X", "F", "rank", "cd"))
    K, pop, nv = X.shape
    ms = vary(X, rank, cd, xl, xu, eta_c, eta_m, prob_m, seed, gen, n_real, prob_x, prob_flip)
    off = np.stack([m["off32"] for m in ms]).astype(np.float32)
    off_F = np.asarray(evaluate(off.reshape(K * pop, nv)), np.float32).reshape(K, pop, -1)
    flags = np.stack([SR.duplicates(X[i], off[i]) for i in range(K)])
    nX, nF, nr, nc, counts = X.copy(), F.copy(), np.array(rank, np.int32), np.array(cd, np.float64), np.zeros((K, 2), np.int32)
    for i in range(K):
        Fm, Xm = np.concatenate([F[i], off_F[i]]), np.concatenate([X[i], off[i]])
        s = SR.survive(Fm, pop, pop, nsga, flags[i])
        assert len(s["chosen"]) == pop
        nX[i], nF[i], nr[i], nc[i], counts[i] = Xm[s["chosen"]], Fm[s["chosen"]], s["rank"], s["cd"], s["counts"]
    new = dict(X=nX, F=nF, rank=nr, cd=nc)
    accepted = None
    if migration_due(gen, K, migrate_every):
        m = migrate(nX, nF, nr, nc, migrants, nsga)
        accepted = m.pop("accepted")
        new = m
    return new, dict(off_X=off, off_F=off_F, flags=flags, counts=counts, accepted=accepted)


# ---- hand-made migration cases shared by the CPU and the GPU tests -----------------------------------------------------------------
def ranked(X, F, nsga):
    """Islands X [K, pop, n_var] with F [K, pop, n_obj] -> (X, F, rank, cd) as a survival leaves them (each island ranked and ordered)."""
    X, F = np.array(X, np.float32), np.array(F, np.float32)
    K, pop = F.shape[:2]
    rank, cd = np.zeros((K, pop), np.int32), np.zeros((K, pop))
    for i in range(K):
        s = SR.survive(F[i], pop, pop, nsga, None)
        X[i], F[i], rank[i], cd[i] = X[i][s["chosen"]], F[i][s["chosen"]], s["rank"], s["cd"]
    return X, F, rank, cd


def migration_cases(n_var=5):
    """name -> (X, F, rank, cd, n, nsga).  Rows are told apart by their first variable: island i's row with F = f holds 100 i + f."""
    out = {}

    def ga(K, pop, shift=0.0):
        F = np.stack([np.arange(pop, dtype=np.float32)[::-1] * (i + 1) + shift + 0.25 * i for i in range(K)])[..., None]
        X = np.repeat((100.0 * np.arange(K)[:, None] + F[..., 0])[..., None], n_var, axis=2).astype(np.float32)
        X[..., 1:] += np.arange(1, n_var, dtype=np.float32)
        return X, F
    for K, n, name in ((2, 1, "ring_k2"), (3, 1, "ring_k3"), (3, 2, "two_migrants"), (2, 3, "half_pop")):
        X, F = ga(K, 6)
        out[name] = ranked(X, F, False) + (n, False)
    # a migrant equal to a receiver row (island 1 already holds island 0's best row), and two equal migrants (island 1's rows with F = 0.25)
    X, F = ga(3, 6)
    X[1, 2], F[1, 2] = X[0, 5], F[0, 5]
    X[1, 4], F[1, 4] = X[1, 5], F[1, 5]
    out["duplicates"] = ranked(X, F, False) + (3, False)
    # -0.0 against 0.0: island 1's row with F = 4.25 is island 0's best row up to the sign of a zero
    X, F = ga(2, 6)
    X[0, 5, 1:] = 0.0
    X[1, 3] = X[0, 5]
    X[1, 3, 1] = -0.0
    out["negative_zero"] = ranked(X, F, False) + (1, False)
    # NSGA-II, two objectives: a first front of four rows whose ends have an infinite distance and come first, then a front of two
    FA = np.array([(1, 2.5), (0, 4), (2, 1), (4, 0), (5, 5), (6, 4.5)], np.float32)
    F2 = np.stack([FA, FA + 10])
    X2 = np.concatenate([F2, np.zeros((2, 6, n_var - 2), np.float32)], axis=2)
    X2[..., 2:] = np.arange(2, n_var, dtype=np.float32)
    out["nsga_infinite"] = ranked(X2, F2, True) + (3, True)
    rng = np.random.default_rng(5)
    F3 = rng.standard_normal((3, 8, 2)).astype(np.float32)
    X3 = rng.standard_normal((3, 8, n_var)).astype(np.float32)
    out["nsga_random"] = ranked(X3, F3, True) + (2, True)
    return out
