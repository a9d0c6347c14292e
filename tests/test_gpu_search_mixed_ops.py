"""ga_vary_bits_kernel and the strided ga_vary_kernel (csrc/search.hip) in isolation, through glass_op_ga_vary_mixed, against the numpy
mirror tests/search_mixed_ref.py (pinned by tests/test_search_mixed_ref.py).

Bit columns: exactly the mirror's — the gate, the set D, the exchanged subset and every flip are discrete outcomes.  Real columns: through
search_device_ref.check_offspring (discrete outcomes exact, values within 2 fp32 ulps at the bound), and bit for bit what glass_op_ga_vary
gives for X[:, :n_real] — the all-real search of that width.

Shapes: (pop 8, n_real 16, n_bits 24) the mini BigGAN's row, vector path; (8, 128, 1000) the real row — more than one 256-thread pass over
the bits, a tail that is no multiple of 64; (7, 6, 70) odd pop, scalar path; (8, 4, 4096) the cap.  Bit patterns: Bernoulli(0.005) parents,
parents that differ in every bit (|D| = n_bits) and in every bit but one (the other parity of |D|), identical sections, exactly one
differing bit — each with prob_x 1, 0 and 0.2 and prob_flip 0, 10 / 1000 and 1.

Measured on an MI355X (the real columns' figures are logged through util.diag): in all 180 cases every bit equals the mirror's and 0 real
values differ from the rounded mirror (worst 0.00 ulp against the bar of 2)."""
import os

import numpy as np
import pytest

import search_device_ref as SR
import search_mixed_ref as MR

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
SHAPES = [(8, 16, 24), (8, 128, 1000), (7, 6, 70), (8, 4, 4096)]
XL, XU = -2.0, 2.0
SEED, GEN = (5 << 32) | 11, 4
# |D| of the matings that must occur in a pattern's case (the tournament decides which rows meet: the mirror says whether they did)
EXPECT_D = {"all_differ": lambda nb: nb, "all_but_one_differ": lambda nb: nb - 1, "one_differs": lambda nb: 1}


@pytest.fixture(scope="module")
def ops():
    from clip_glass_amd import ops as _ops
    return _ops


def vary(ops, X, n_real, rank, cd, prob_x, prob_flip, **kw):
    return ops.ga_vary_mixed(X, n_real, rank, cd, XL, XU, prob_x=prob_x, prob_flip=prob_flip, seed=SEED, generation=GEN, **kw)


@pytest.mark.parametrize("pattern", MR.BIT_PATTERNS)
@pytest.mark.parametrize("pop,n_real,n_bits", SHAPES)
def test_vary_mixed_against_mirror(ops, pop, n_real, n_bits, pattern):
    X, rank, cd = MR.population_case(pop, n_real, n_bits, pattern)
    exchanged = flipped = 0
    for prob_x in (1.0, 0.0, 0.2):
        for prob_flip in (0.0, 10 / 1000, 1.0):
            name = "mixed (%d, %d, %d) %s prob_x %g prob_flip %g" % (pop, n_real, n_bits, pattern, prob_x, prob_flip)
            m = MR.vary_mixed(X, n_real, rank, cd, XL, XU, 3.0, 3.0, 0.5, prob_x, prob_flip, SEED, GEN)
            got = vary(ops, X, n_real, rank, cd, prob_x, prob_flip)
            assert got.shape == X.shape
            MR.check_bits(name, got[:, n_real:], m)
            SR.check_offspring(name, got[:, :n_real], X[:, :n_real], m["real"], XL, XU)
            if prob_x == 1.0 and pattern in EXPECT_D:
                assert EXPECT_D[pattern](n_bits) in [d.size for d in m["D"]], "%s: no mating pairs rows that differ" % name
            exchanged += sum(s.size for s in m["selected"])
            flipped += int(m["flips"].sum())
    assert flipped > 0 and (exchanged > 0 if pattern in EXPECT_D else exchanged == 0 or pattern == "bernoulli")


@pytest.mark.parametrize("pop,n_real,n_bits", SHAPES)
def test_slices_and_single_rows_equal_the_whole_launch(ops, pop, n_real, n_bits):
    X, rank, cd = MR.population_case(pop, n_real, n_bits, "all_but_one_differ")
    whole = vary(ops, X, n_real, rank, cd, 1.0, 10 / 1000)
    h = (pop // 2) | 1      # an odd cut: the two children of a mating land in different launches
    two = np.concatenate([vary(ops, X, n_real, rank, cd, 1.0, 10 / 1000, row0=0, rows=h), vary(ops, X, n_real, rank, cd, 1.0, 10 / 1000, row0=h, rows=pop - h)])
    assert np.array_equal(SR.bits(two), SR.bits(whole))
    rows = np.concatenate([vary(ops, X, n_real, rank, cd, 1.0, 10 / 1000, row0=r, rows=1) for r in range(pop)])
    assert np.array_equal(SR.bits(rows), SR.bits(whole))
    # another generation or seed is another offspring, in the bits too
    other = ops.ga_vary_mixed(X, n_real, rank, cd, XL, XU, prob_x=1.0, prob_flip=10 / 1000, seed=SEED, generation=GEN + 1)
    assert not np.array_equal(other[:, n_real:], whole[:, n_real:]) and not np.array_equal(SR.bits(other[:, :n_real]), SR.bits(whole[:, :n_real]))


@pytest.mark.parametrize("pop,n_real,n_bits", SHAPES)
def test_real_columns_are_the_all_real_search(ops, pop, n_real, n_bits):
    X, rank, cd = MR.population_case(pop, n_real, n_bits, "bernoulli")
    got = vary(ops, X, n_real, rank, cd, 0.2, 10 / 1000)
    real = ops.ga_vary(np.ascontiguousarray(X[:, :n_real]), rank, cd, XL, XU, seed=SEED, generation=GEN)
    assert np.array_equal(SR.bits(got[:, :n_real]), SR.bits(real))


def test_refused_shapes(ops):
    rank, cd = np.zeros(8, np.int32), np.zeros(8)
    with pytest.raises(RuntimeError, match="ga_vary_mixed refused the shape"):
        ops.ga_vary_mixed(np.zeros((8, 4 + 4097), np.float32), 4, rank, cd, XL, XU)
    with pytest.raises(RuntimeError, match="ga_vary_mixed refused the shape"):
        ops.ga_vary_mixed(np.zeros((8, 24), np.float32), 0, rank, cd, XL, XU)
    with pytest.raises(RuntimeError, match="ga_vary_mixed refused the shape"):
        ops.ga_vary_mixed(np.zeros((8, 16), np.float32), 16, rank, cd, XL, XU)      # no bit column
    with pytest.raises(RuntimeError, match="inside the pop offspring rows"):
        ops.ga_vary_mixed(np.zeros((8, 40), np.float32), 16, rank, cd, XL, XU, row0=4, rows=5)
