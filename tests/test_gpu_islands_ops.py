"""The island kernels of csrc/search.hip and the noise period in isolation, through the diagnostic ops (include/glass_ops.h "The island
kernels"), against the numpy mirror tests/search_islands_ref.py.  Everything is exact: rows, F, ranks and the accepted counts as they are,
distances and noise planes bit for bit.

glass_op_ga_migrate runs what the engine launches behind a due migration — ga_migrate_kernel, the gated ga_survive_kernel and ga_gather_kernel
over the islands — on the hand-made cases of tests/test_search_islands_ref.py (ring direction at K = 2 and 3, n = pop / 2, duplicates, -0.0,
the NSGA-II order through infinite distances) and on K = 3, pop 8 at n_var 513 (rows off the 16-byte vector) and 512 (on it).  The rows that
are no multiple of 4 wide are the only place where the VEC = 1 instances run with more than one island: the mini models' rows are."""
import os

import numpy as np
import pytest

import search_islands_ref as IR
from score_tail_golden import golden, pack

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
CASES = IR.migration_cases()


@pytest.fixture(scope="module")
def ops():
    from clip_glass_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("name", sorted(CASES))
def test_migrate_hand_made_cases(ops, name):
    X, F, rank, cd, n, nsga = CASES[name]
    got = ops.ga_migrate(X, F, rank, cd, n, nsga=nsga)
    ref = IR.check_migration(name, got, X, F, rank, cd, n, nsga)
    assert ref["accepted"].sum() > 0


@pytest.mark.parametrize("nv", [513, 512])
@pytest.mark.parametrize("nsga,n", [(True, 2), (False, 4), (True, 1)])
def test_migrate_wide_rows(ops, nv, nsga, n):
    K, pop = 3, 8
    rng = np.random.default_rng(nv + n)
    X = rng.standard_normal((K, pop, nv)).astype(np.float32)
    F = rng.standard_normal((K, pop, 2 if nsga else 1)).astype(np.float32)
    X, F, rank, cd = IR.ranked(X, F, nsga)
    best = IR.order(rank[0], cd[0])
    X[1, 5] = X[0, best[0]]                 # island 1 holds island 0's best row already ...
    X[1, 5, nv - 1] = X[0, best[0], nv - 1] if n > 1 else np.float32(7.0)      # ... or a row that differs from it in the LAST variable only
    got = ops.ga_migrate(X, F, rank, cd, n, nsga=nsga)
    ref = IR.check_migration("wide n_var %d nsga %d n %d" % (nv, nsga, n), got, X, F, rank, cd, n, nsga)
    assert ref["accepted"][1] == (n - 1 if n > 1 else 1) and ref["accepted"][0] == n


def test_migrate_refusals(ops):
    X, F, rank, cd, n, nsga = CASES["ring_k3"]
    with pytest.raises(RuntimeError, match=r"migrants must be in \[1, pop / 2 = 3\]"):
        ops.ga_migrate(X, F, rank, cd, 4, nsga=nsga)
    with pytest.raises(RuntimeError, match="at least two islands"):
        ops.ga_migrate(X[:1], F[:1], rank[:1], cd[:1], 1, nsga=nsga)


def test_noise_period(ops):
    """Period 2: the planes of a launch of four minibatches are glass_op_noise's planes of minibatches 0, 1, 0, 1; from minibatch 1 on they are
    those of 1, 0, 1; period 0 is glass_op_noise."""
    hw, layer, gen, seed = 8 * 8 + 3, 2, 5, (7 << 32) | 9
    plain = ops.noise(4, hw, layer, 0, gen, seed)
    assert not np.array_equal(plain[0], plain[1]) and np.isfinite(plain).all()
    got = ops.noise_period(4, hw, layer, 0, gen, seed, 2)
    assert np.array_equal(got.view(np.uint32), plain[[0, 1, 0, 1]].view(np.uint32))
    got = ops.noise_period(3, hw, layer, 1, gen, seed, 2)
    assert np.array_equal(got.view(np.uint32), plain[[1, 0, 1]].view(np.uint32))
    assert np.array_equal(ops.noise_period(4, hw, layer, 0, gen, seed, 0).view(np.uint32), plain.view(np.uint32))


ISLAND_V = [1, 3]


def _island_cosine_case(V):
    K, pop, T, D = 3, 4, 3, 70
    rng = np.random.default_rng(V)
    feat = rng.standard_normal((K * pop, V, D)).astype(np.float32)
    targets = rng.standard_normal((T, D)).astype(np.float32)
    table = np.array([[1, 0, 0], [0, 0, 1], [0.5, -2, 0.25]], np.float32)
    return feat, targets, table, pop


@pytest.mark.parametrize("V", ISLAND_V)
def test_island_cosine(ops, V):
    """Every island's rows equal glass_op_cosine_set on those rows with the island's own weights, by value; an island with a single weight of 1
    equals the set that holds that entry alone; a launch that starts inside the table (row0 > 0) finds its islands; the whole launch has the
    bits of the commit before csrc/score.hip (tests/score_tail_golden.py)."""
    feat, targets, table, pop = _island_cosine_case(V)
    K = table.shape[0]
    vs, ss, sim = ops.cosine_set_islands(feat, targets, table, pop)
    got, want = pack(vs, ss, sim), golden("island_cosine_V%d" % V)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(sim).all() and (sim != sim[0]).any()
    for i in range(K):
        rows = slice(i * pop, (i + 1) * pop)
        v1, s1, m1 = ops.cosine_set(feat[rows], targets, table[i])
        assert np.array_equal(vs[rows], v1) and np.array_equal(ss[rows], s1) and np.array_equal(sim[rows], m1), i
    for i, t in ((0, 0), (1, 2)):
        rows = slice(i * pop, (i + 1) * pop)
        assert np.array_equal(sim[rows], ops.cosine_set(feat[rows], targets[t:t + 1], np.ones(1, np.float32))[2]), i
    tail = ops.cosine_set_islands(feat[pop:], targets, table, pop, row0=pop)
    assert np.array_equal(tail[2], sim[pop:]) and np.array_equal(tail[1], ss[pop:])
    with pytest.raises(RuntimeError, match="must lie inside the islands"):
        ops.cosine_set_islands(feat, targets, table, pop, row0=1)
