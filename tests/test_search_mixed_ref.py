"""tests/search_mixed_ref.py (the numpy mirror of the device search's mixed rows, include/glass.h "Mixed rows") pinned without a GPU: known
answers by hand, invariants of half-uniform crossover over random matings, the real columns against search_device_ref.vary, what
minimize(device=True) takes and refuses of a mask with bool columns, and the edges of the host-only rule."""
import types

import numpy as np
import pytest

import search_device_ref as SR
import search_mixed_ref as MR
from clip_glass_amd import search, synth

SEED = (5 << 32) | 11


def test_purpose_words():
    assert (synth.SEARCH_DRAW_BIT_GATE, synth.SEARCH_DRAW_BIT_KEY, synth.SEARCH_DRAW_BIT_FLIP) == (3, 4, 5)
    # a key is the raw word behind u0
    k = MR.hux_keys(9, 2, 3, 16, 24)
    u0 = synth.search_uniforms(9, 2, np.arange(3, dtype=np.uint32)[:, None], (16 + np.arange(24, dtype=np.uint32))[None, :], synth.SEARCH_DRAW_BIT_KEY)[0]
    assert k.dtype == np.uint32 and np.array_equal((k.astype(np.float64) + 0.5) * 2.0 ** -32, u0)
    assert len(np.unique(k)) > 60


def test_hux_known_answers():
    """The case of test_search.py::test_hux_and_bitflip_known_answers: D = {0, 2, 3, 5, 6} ranked [5, 0, 6, 2, 3] by the injected keys."""
    a = np.array([1, 1, 0, 0, 1, 1, 0, 1], np.float32)
    b = np.array([0, 1, 1, 1, 1, 0, 1, 1], np.float32)
    keys = np.zeros(8, np.uint32)
    keys[[5, 0, 6, 2, 3]] = [10, 20, 30, 40, 50]
    keys[[1, 4, 7]] = 0      # the smallest keys of all, on columns outside D: they take no part
    D, sel = MR.hux_select(a, b, keys)
    assert D.tolist() == [0, 2, 3, 5, 6] and sel.tolist() == [0, 5, 6]
    c0, c1 = MR.hux_children(a, b, sel)
    assert c0.tolist() == [0, 1, 0, 0, 1, 0, 1, 1] and c1.tolist() == [1, 1, 1, 1, 1, 1, 0, 1]
    # a closed gate copies
    D, sel = MR.hux_select(a, b, keys, gate=False)
    assert D.tolist() == [0, 2, 3, 5, 6] and sel.size == 0
    c0, c1 = MR.hux_children(a, b, sel)
    assert np.array_equal(c0, a) and np.array_equal(c1, b)
    # |D| = 0 and |D| = 1
    D, sel = MR.hux_select(a, a, keys)
    assert D.size == 0 and sel.size == 0
    one = a.copy()
    one[4] = 0
    D, sel = MR.hux_select(a, one, keys)
    assert D.tolist() == [4] and sel.tolist() == [4]
    # equal keys break by index: n = 3 of D = {0, 2, 3, 5, 6} with one key everywhere
    D, sel = MR.hux_select(a, b, np.full(8, 7, np.uint32))
    assert sel.tolist() == [0, 2, 3]
    # ... and only among equals: a smaller key on a later column comes first
    keys = np.full(8, 7, np.uint32)
    keys[6] = 1
    assert MR.hux_select(a, b, keys)[1].tolist() == [0, 2, 6]
    # the top bit of a key counts (unsigned order)
    keys = np.full(8, 0x80000000, np.uint32)
    keys[[5, 6, 3]] = [1, 2, 0x7FFFFFFF]
    assert MR.hux_select(a, b, keys)[1].tolist() == [3, 5, 6]


def test_bitflip_gate():
    f = MR.bitflip(5, 1, np.arange(8), 16, 1000, 0.01)
    assert f.shape == (8, 1000) and 20 <= int(f.sum()) <= 160
    assert not MR.bitflip(5, 1, np.arange(8), 16, 1000, 0.0).any() and MR.bitflip(5, 1, np.arange(8), 16, 1000, 1.0).all()
    # a function of the row, not of the slice
    assert np.array_equal(MR.bitflip(5, 1, [3, 6], 16, 1000, 0.01), f[[3, 6]])


def test_hux_invariants_over_random_matings():
    n_bits, n_real = 70, 6
    rng = np.random.default_rng(0)
    keys = MR.hux_keys(12, 3, 200, n_real, n_bits)
    sizes = set()
    for m in range(200):
        a = (rng.random(n_bits) < 0.3).astype(np.float32)
        b = (rng.random(n_bits) < (0.3 if m % 4 else 0.01 * (m % 7))).astype(np.float32)
        if m % 50 == 0:
            b = a.copy()
        D, sel = MR.hux_select(a, b, keys[m])
        assert set(sel.tolist()) <= set(D.tolist())
        assert sel.size == (D.size + 1) // 2
        c0, c1 = MR.hux_children(a, b, sel)
        ai, bi, c0i, c1i = (v.astype(np.int64) for v in (a, b, c0, c1))
        assert np.array_equal(c0i | c1i, ai | bi) and np.array_equal(c0i & c1i, ai & bi)
        sizes.add(int(D.size))
    assert 0 in sizes and len(sizes) > 10


@pytest.mark.parametrize("pop,n_real,n_bits", [(8, 16, 24), (7, 6, 70)])
def test_real_columns_are_the_all_real_search(pop, n_real, n_bits):
    X, rank, cd = MR.population_case(pop, n_real, n_bits, "bernoulli")
    seed, gen = (5 << 32) | 11, 4
    m = MR.vary_mixed(X, n_real, rank, cd, -2.0, 2.0, 3.0, 3.0, 0.5, 0.2, 0.01, seed, gen)
    r = SR.vary(X[:, :n_real], rank, cd, -2.0, 2.0, 3.0, 3.0, 0.5, seed, gen)
    assert m["off32"].shape == (pop, n_real + n_bits)
    assert np.array_equal(SR.bits(m["off32"][:, :n_real]), SR.bits(r["off32"]))
    assert np.array_equal(m["off32"][:, n_real:], m["bits"]) and np.isin(m["bits"], (0.0, 1.0)).all()
    assert len(m["D"]) == len(m["selected"]) == (pop + 1) // 2 and m["flips"].shape == (pop, n_bits)


def test_vary_mixed_decisions():
    """prob_x 1 / prob_flip 0: every child is its mating's exchange; prob_x 0 / prob_flip 1: the complement of a copy."""
    pop, n_real, n_bits = 8, 16, 24
    X, rank, cd = MR.population_case(pop, n_real, n_bits, "all_differ")
    m = MR.vary_mixed(X, n_real, rank, cd, -2.0, 2.0, 3.0, 3.0, 0.5, 1.0, 0.0, SEED, 4)
    assert m["gate"].all() and not m["flips"].any()
    pa, pb = X[m["parents"][0], n_real:], X[m["parents"][1], n_real:]
    differing = [i for i in range(pop // 2) if m["D"][i].size]
    assert differing and all(m["D"][i].size == n_bits and m["selected"][i].size == n_bits // 2 for i in differing)
    for i in range(pop // 2):
        swapped = np.zeros(n_bits, bool)
        swapped[m["selected"][i]] = True
        assert np.array_equal(m["bits"][2 * i], np.where(swapped, pb[i], pa[i])) and np.array_equal(m["bits"][2 * i + 1], np.where(swapped, pa[i], pb[i]))
    c = MR.vary_mixed(X, n_real, rank, cd, -2.0, 2.0, 3.0, 3.0, 0.5, 0.0, 1.0, SEED, 4)
    assert not c["gate"].any() and c["flips"].all()
    assert np.array_equal(c["bits"][0::2], 1 - pa) and np.array_equal(c["bits"][1::2], 1 - pb)


# ---- minimize(device=True) with a mask that has bool columns ---------------------------------------------------------------------
class _Stop(Exception):
    pass


class _Engine:
    """Carries what _minimize_device reads before it touches the device; the first device call ends the test."""

    def __init__(self, pop, n_real=None):
        self.search_pop = pop
        if n_real is not None:
            self.search_n_real = n_real
        self.calls = []

    def set_search_operators_mixed(self, *a):
        self.calls.append(("mixed",) + a)

    def set_search_operators(self, *a):
        self.calls.append(("real",) + a)

    def search_init(self, X):
        self.calls.append(("init", np.asarray(X)))
        raise _Stop()


class _Sampling:
    def _do(self, problem, n):
        z = np.random.normal(size=(n, 8))
        return np.concatenate([np.clip(z, -2, 2), (np.random.random((n, 8)) < 0.3).astype(float)], axis=1)


def _problem(engine):
    return types.SimpleNamespace(n_var=16, n_obj=1, xl=-2.0, xu=2.0, config=types.SimpleNamespace(batch_size=4), engine=engine, ranks=1)


def test_minimize_device_takes_a_real_then_bool_mask():
    e = _Engine(8, n_real=8)
    with pytest.raises(_Stop):
        search.minimize(_problem(e), "ga", 8, 2, _Sampling(), seed=3, device=True, mask=["real"] * 8 + ["bool"] * 8)
    assert [c[0] for c in e.calls] == ["mixed", "init"]
    assert e.calls[0][1:] == (-2.0, 2.0, 3.0, 3.0, 0.5, 0.2, 10 / 1000, 3)
    X0 = e.calls[1][1]
    assert X0.shape == (8, 16) and np.isin(X0[:, 8:], (0.0, 1.0)).all()


def test_minimize_device_all_real_goes_the_old_way():
    e = _Engine(8)
    with pytest.raises(_Stop):
        search.minimize(_problem(e), "ga", 8, 2, _Sampling(), seed=3, device=True, mask=None)
    assert [c[0] for c in e.calls] == ["real", "init"]


@pytest.mark.parametrize("engine,mask,words", [
    (_Engine(8, n_real=4), ["real"] * 8 + ["bool"] * 8, ["real", "4 real columns", "set_search_mixed"]),      # set up for another real count
    (_Engine(8), ["real"] * 8 + ["bool"] * 8, ["all-real rows", "set_search_mixed"]),                          # set up by set_search
    (_Engine(8, n_real=8), ["bool"] * 8 + ["real"] * 8, ["bool column in front of a real one"]),
    (_Engine(8, n_real=8), ["real"] * 4 + ["bool"] * 4 + ["real"] * 4 + ["bool"] * 4, ["bool column in front of a real one"]),
    (_Engine(8, n_real=8), ["bool"] * 16, ["real"]),
    (_Engine(8, n_real=8), ["real"] * 8 + ["int"] * 8, ["int"]),
    (_Engine(8, n_real=8), ["real"] * 8 + ["bool"] * 4 + ["int"] * 4, ["bool / int"]),
])
def test_minimize_device_mask_refusals(engine, mask, words):
    with pytest.raises(ValueError) as ex:
        search.minimize(_problem(engine), "ga", 8, 2, _Sampling(), device=True, mask=mask)
    assert all(w in str(ex.value) for w in words), str(ex.value)
    assert not engine.calls


def test_mixed_search_supported_edges():
    from clip_glass_amd.engine import mixed_search_supported, search_supported
    assert mixed_search_supported(64, 128, 1000, 1, "ga") == (True, "")
    assert mixed_search_supported(8, 4, 4096, 1, "ga")[0] and mixed_search_supported(8, 4, 1, 2, "nsga2")[0]
    for n_bits in (0, 4097):
        ok, msg = mixed_search_supported(8, 4, n_bits, 1, "ga")
        assert not ok and "n_bits" in msg and "4096" in msg
    ok, msg = mixed_search_supported(8, 0, 24, 1, "ga")
    assert not ok and "n_real" in msg
    # everything search_supported says for n_var = n_real + n_bits
    for pop, n_obj, algo in [(1025, 1, "ga"), (8, 2, "ga"), (8, 7, "nsga2"), (1, 1, "ga")]:
        assert mixed_search_supported(pop, 16, 24, n_obj, algo) == search_supported(pop, 40, n_obj, algo)
        assert not mixed_search_supported(pop, 16, 24, n_obj, algo)[0]
    assert not mixed_search_supported(8, 16, 24, 1, "sa")[0]
