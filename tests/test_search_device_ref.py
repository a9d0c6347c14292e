"""tests/search_device_ref.py (the float64 mirror of the device search, include/glass.h "Device search") pinned on the CPU to the project's
own host operators: search.sbx_vectorised / polynomial_mutation, fed the mirror's uniforms through a stub rng, give the mirror's children
bit for bit; the mirror's survival equals minimize's survive() restated from fast_non_dominated_sort / crowding_distance in indices, order,
rank and distance; and minimize(device=True) refuses what the device search does not do, by name, before it touches an engine."""
import types

import numpy as np
import pytest

import search_device_ref as SR
from clip_glass_amd import search, synth


class StubRng:
    """Hands out queued arrays in the order the operator asks for them, checking the shapes."""

    def __init__(self, *arrays):
        self.q = list(arrays)

    def random(self, shape=None):
        a = self.q.pop(0)
        assert tuple(np.shape(a)) == tuple(np.atleast_1d(shape)), (np.shape(a), shape)
        return a


def test_uniforms_are_the_philox_words():
    u = synth.search_uniforms(0x1234567800000005, 7, np.arange(3, dtype=np.uint32), 2, synth.SEARCH_DRAW_SBX)
    w = synth.philox4x32(np.arange(3, dtype=np.uint32), 2, 7, 1, 5, 0x12345678 ^ synth.SEARCH_TAG)
    for a, b in zip(u, w):
        assert np.array_equal(a, (b.astype(np.float64) + 0.5) * 2.0 ** -32)
        assert (a > 0).all() and (a < 1).all()
    # another purpose, generation or variable is another block
    v = synth.search_uniforms(0x1234567800000005, 7, np.arange(3, dtype=np.uint32), 2, synth.SEARCH_DRAW_MUTATION)
    assert not np.array_equal(u[0], v[0])


@pytest.mark.parametrize("pop,nv,xl,xu", [(8, 20, -10.0, 10.0), (7, 33, -2.5, 6.0)])
def test_mirror_children_equal_the_host_operators_bit_for_bit(pop, nv, xl, xu):
    X, rank, cd = SR.population_case(pop, nv, xl, xu)
    seed, gen, eta_c, eta_m, prob_m = 11, 4, 3.0, 3.0, 0.5
    m = SR.vary(X, rank, cd, xl, xu, eta_c, eta_m, prob_m, seed, gen)
    Xd = X.astype(np.float64)
    nm = (pop + 1) // 2
    u, su, gu = SR.sbx_uniforms(seed, gen, nm, nv)
    bl, bu = np.full(nv, xl), np.full(nv, xu)
    ca, cb = search.sbx_vectorised(StubRng(u, su, np.zeros((nm, 1)), gu), Xd[m["parents"][0]], Xd[m["parents"][1]], bl, bu, eta_c)
    off = np.empty((2 * nm, nv))
    off[0::2], off[1::2] = ca, cb
    off = off[:pop]
    mu, mg = SR.mutation_uniforms(seed, gen, np.arange(pop), nv)
    off = search.polynomial_mutation(StubRng(mu, mg), off, bl, bu, eta_m, prob_m)
    assert np.array_equal(off.view(np.uint64), m["off"].view(np.uint64))
    assert (m["off"] >= xl).all() and (m["off"] <= xu).all()
    # the cases the shapes are there for: equal parents are never crossed, and some variables are, some are mutated
    same = (Xd[m["parents"][0]] == Xd[m["parents"][1]])
    assert not m["active"][same].any()
    assert m["active"].any() and (~m["active"]).any() and m["mutated"].any() and (~m["mutated"]).any()


def test_tournament_rule():
    pop = 16
    rank = np.array([0, 1] * 8)
    cd = np.linspace(0, 1, pop)
    parents, c = SR.tournament(5, 2, pop, rank, cd)
    assert parents.shape == (2, 8) and c.min() >= 0 and c.max() < pop
    for p, (a, b) in zip(parents.reshape(-1), np.concatenate([c[:2].T, c[2:].T])):
        want = a if (rank[a] < rank[b] or (rank[a] == rank[b] and cd[a] >= cd[b])) else b
        assert p == want
    # `>=` goes to the first contestant
    assert (SR.tournament(5, 2, pop, np.zeros(pop, int), np.zeros(pop))[0] == np.stack([c[0], c[2]])).all()


def host_survive(F, n_pop, pop_out, nsga, flags=None):
    """minimize's survive() closure over the eligible merged rows, restated from search.py's functions; indices are merged indices."""
    valid, _ = SR.eligible(F, n_pop, flags)
    idx = np.nonzero(valid)[0]
    Fv = np.asarray(F, np.float32).astype(np.float64)[idx]
    if not nsga:
        order = np.argsort(Fv[:, 0], kind="mergesort")[:pop_out]
        return idx[order], np.zeros(len(order), int), -Fv[order, 0]
    fronts, rank = search.fast_non_dominated_sort(Fv)
    chosen, cds = [], []
    for fr in fronts:
        cd = search.crowding_distance(Fv[fr])
        if len(chosen) + len(fr) > pop_out:
            order = np.argsort(-cd, kind="mergesort")[: pop_out - len(chosen)]
            fr, cd = fr[order], cd[order]
        chosen.extend(fr.tolist())
        cds.extend(cd.tolist())
        if len(chosen) >= pop_out:
            break
    chosen = np.array(chosen)
    return idx[chosen], rank[chosen], np.array(cds)


@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_mirror_survival_equals_minimize_survive(N, M):
    n_pop = N // 2
    for name, (F, flags) in SR.survive_cases(N, M).items():
        for nsga in ([False, True] if M == 1 else [True]):
            got = SR.survive(F, n_pop, n_pop, nsga, flags)
            idx, rank, cd = host_survive(F, n_pop, n_pop, nsga, flags)
            assert np.array_equal(got["chosen"], idx), (name, nsga)
            assert np.array_equal(got["rank"], rank), (name, nsga)
            assert np.array_equal(got["cd"].view(np.uint64), np.asarray(cd, np.float64).view(np.uint64)), (name, nsga)
            assert len(idx) == n_pop
    F, flags = SR.survive_cases(N, M)["left_out"]
    got = SR.survive(F, n_pop, n_pop, True, flags)
    assert got["counts"] == (2, 2) and not set(got["chosen"]) & {n_pop, n_pop + 1, n_pop + 2, n_pop + 3}


def test_mirror_duplicates():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((8, 20)).astype(np.float32)
    off = rng.standard_normal((8, 20)).astype(np.float32)
    off[1] = X[5]
    off[2] = X[5]
    off[2, -1] += 1
    off[4] = off[3]
    X[0, 0], off[6] = 0.0, X[0]
    off[6, 0] = -0.0
    assert SR.duplicates(X, off).tolist() == [0, 1, 0, 0, 1, 0, 1, 0]


# ---- minimize(device=True): what it refuses, before it touches an engine ---------------------------------------------------------
class _Sampling:
    def _do(self, problem, n):
        return np.random.normal(size=(n, problem.n_var))


def _problem(**kw):
    p = types.SimpleNamespace(n_var=16, n_obj=2, xl=-10.0, xu=10.0, config=types.SimpleNamespace(batch_size=4), engine=object(), ranks=1)
    p.__dict__.update(kw)
    p._evaluate = lambda x, out: out.__setitem__("F", np.zeros((x.shape[0], p.n_obj)))
    return p


@pytest.mark.parametrize("kw,mask,pop,word", [
    (dict(), ["real"] * 8 + ["bool"] * 8, 8, "real"),
    (dict(ranks=2), None, 8, "rank"),
    (dict(), None, 2048, "1024"),
    (dict(), None, 6, "batch_size"),
    (dict(engine=None), None, 8, "engine"),
    (dict(xl=np.full(16, -10.0) + np.arange(16)), None, 8, "scalar"),
])
def test_minimize_device_refusals(kw, mask, pop, word):
    with pytest.raises(ValueError, match=word):
        search.minimize(_problem(**kw), "nsga2", pop, 2, _Sampling(), device=True, mask=mask)
