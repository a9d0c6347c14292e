"""ga_vary_kernel, ga_duplicates_kernel and ga_survive_kernel (csrc/search.hip) in isolation, through the diagnostic ops, against the float64
mirror tests/search_device_ref.py (pinned to search.py's own operators by tests/test_search_device_ref.py).

Vary.  Every discrete outcome is the mirror's: a variable the mirror neither crosses nor mutates must carry its parent's bits, which pins the
tournament winners, the per-variable gate and the 1e-14 gate; the swap and the mutation gate decide between values that are far apart, so a
wrong one fails the value bar.  Values: |device - fp32(mirror)| <= 2 fp32 ulps at max(|xl|, |xu|) — one for the final rounding, one for a
last-bit difference between the device's and numpy's double pow().  The figures are printed before they are asserted.
Duplicates and survival are exact: flags, chosen indices, their order, ranks, and the distances' float64 bits.

Shapes (the issue's): vary (8, 20), (7, 513), (16, 512) — odd pop, rows off the vector width, one full-width case — with bounds -10 / 10 and
an asymmetric pair, rows with equal parents and parents on the bounds; duplicates (8, 20), (64, 513); survival at 16 and 64 merged rows with
1, 2 and 3 objectives, and one run at 2048 merged rows.

Measured on an MI355X (logged through util.diag): in all seven vary cases 0 of up to 8192 values differ from the rounded mirror — worst
0.00 ulp against the bar of 2 — and 0 of the 55 to 2333 variables the mirror leaves alone have wrong bits; duplicates and survival: exact."""
import os

import numpy as np
import pytest

import search_device_ref as SR

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]


@pytest.fixture(scope="module")
def ops():
    from clip_glass_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("pop,nv", [(8, 20), (7, 513), (16, 512)])
@pytest.mark.parametrize("xl,xu", [(-10.0, 10.0), (-2.5, 6.0)])
def test_vary_against_mirror(ops, pop, nv, xl, xu):
    X, rank, cd = SR.population_case(pop, nv, xl, xu)
    seed, gen = (5 << 32) | 11, 4
    m = SR.vary(X, rank, cd, xl, xu, 3.0, 3.0, 0.5, seed, gen)
    got = ops.ga_vary(X, rank, cd, xl, xu, seed=seed, generation=gen)
    SR.check_offspring("vary pop %d n_var %d [%g, %g]" % (pop, nv, xl, xu), got, X, m, xl, xu)
    # the same (seed, generation) at two launch sizes: equal bits
    h = (pop // 2) | 1
    two = np.concatenate([ops.ga_vary(X, rank, cd, xl, xu, seed=seed, generation=gen, row0=0, rows=h),
                          ops.ga_vary(X, rank, cd, xl, xu, seed=seed, generation=gen, row0=h, rows=pop - h)])
    assert np.array_equal(SR.bits(two), SR.bits(got))
    # another generation or seed is another offspring
    assert not np.array_equal(SR.bits(ops.ga_vary(X, rank, cd, xl, xu, seed=seed, generation=gen + 1)), SR.bits(got))
    assert not np.array_equal(SR.bits(ops.ga_vary(X, rank, cd, xl, xu, seed=seed + 1, generation=gen)), SR.bits(got))


def test_vary_ga_ranks(ops):
    """GA: rank 0 and distance -F — the tournament is then on fitness alone."""
    X, _, _ = SR.population_case(8, 20, -10.0, 10.0)
    F0 = np.random.default_rng(2).standard_normal(8)
    m = SR.vary(X, np.zeros(8, np.int32), -F0, -10.0, 10.0, 3.0, 3.0, 0.5, 7, 1)
    SR.check_offspring("vary ga", ops.ga_vary(X, np.zeros(8, np.int32), -F0, -10.0, 10.0, seed=7, generation=1), X, m, -10.0, 10.0)


@pytest.mark.parametrize("pop,nv", [(8, 20), (64, 513)])
def test_duplicates(ops, pop, nv):
    rng = np.random.default_rng(pop)
    X = rng.standard_normal((pop, nv)).astype(np.float32)
    off = rng.standard_normal((pop, nv)).astype(np.float32)
    assert not ops.ga_duplicates(X, off).any(), "false flags on random rows"
    off[1] = X[5]                      # copied from a population row
    off[2] = X[5]
    off[2, -1] += 1                    # differs in the last variable only
    off[4] = off[3]                    # two equal offspring: the first is kept
    X[0, 0] = 0.0
    off[6] = X[0]
    off[6, 0] = -0.0                   # -0.0 against 0.0: equal by value
    off[7] = X[pop - 1]                # the last population row
    off[7, 0] += 1                     # ... differing in the first variable only
    flags = ops.ga_duplicates(X, off)
    want = SR.duplicates(X, off)
    assert want[:8].tolist() == [0, 1, 0, 0, 1, 0, 1, 0] and not want[8:].any()
    assert np.array_equal(flags, want)


@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_survive_cases(ops, N, M):
    n_pop = N // 2
    X = np.random.default_rng(N + M).standard_normal((N, 21)).astype(np.float32)
    for name, (F, flags) in SR.survive_cases(N, M).items():
        for nsga in ([False, True] if M == 1 else [True]):
            got = ops.ga_survive(F, n_pop, n_pop, nsga=nsga, flags=flags, X=X)
            SR.check_survival("%s N %d M %d nsga %d" % (name, N, M, nsga), got, F, n_pop, n_pop, nsga, flags, X)
    # the population alone (search_init's ranking): no offspring rows
    F = SR.survive_cases(N, M)["random"][0][:n_pop]
    SR.check_survival("init N %d M %d" % (N, M), ops.ga_survive(F, n_pop, n_pop, nsga=True), F, n_pop, n_pop, True, None)


def test_survive_largest(ops):
    """2048 merged rows, 2 objectives: the largest supported size (80 KB of LDS: past the 64 KB a kernel gets without opting in), and the same
    rows with 6 objectives (112 KB)."""
    rng = np.random.default_rng(9)
    for M in (2, 6):
        F = rng.standard_normal((2048, M)).astype(np.float32)
        flags = (rng.random(1024) < 0.02).astype(np.int32)
        got = ops.ga_survive(F, 1024, 1024, nsga=True, flags=flags)
        SR.check_survival("largest M %d" % M, got, F, 1024, 1024, True, flags)


def test_refusals(ops):
    F = np.zeros((4098, 2), np.float32)
    with pytest.raises(RuntimeError, match="2048 merged rows"):
        ops.ga_survive(F, 2049, 1024)
    with pytest.raises(RuntimeError, match="6 objectives"):
        ops.ga_survive(np.zeros((16, 7), np.float32), 8, 8)
    from clip_glass_amd.engine import search_supported
    assert search_supported(1024, 9216, 6, "nsga2")[0]
    assert "1024" in search_supported(1025, 512, 2, "nsga2")[1]
    assert "n_obj = 1" in search_supported(64, 512, 2, "ga")[1]
