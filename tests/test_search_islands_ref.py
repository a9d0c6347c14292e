"""The island mirror (tests/search_islands_ref.py) against the text of include/glass.h "Device search: islands": the seed rule, migration known
answers worked out by hand, and the checker shown to fail on planted faults.  No GPU."""
import numpy as np
import pytest

import search_device_ref as SR
import search_islands_ref as IR

XL, XU = -4.0, 4.0
CASES = IR.migration_cases()


def toy(rows):
    """Two objectives of a row, float32."""
    r = np.asarray(rows, np.float64)
    return np.stack([(r ** 2).sum(axis=1), ((r - 1.0) ** 2).sum(axis=1)], axis=1).astype(np.float32)


def start(K, pop, nv, nsga, seed=2):
    X = np.random.default_rng(seed).uniform(XL, XU, (K, pop, nv)).astype(np.float32)
    F = toy(X.reshape(K * pop, nv)).reshape(K, pop, 2)[..., : 2 if nsga else 1]
    return dict(zip(("X", "F", "rank", "cd"), IR.ranked(X, F, nsga)))


def test_island_seed_wraps():
    assert IR.island_seed(5, 0) == 5 and IR.island_seed(5, 3) == 8
    assert IR.island_seed(2 ** 64 - 1, 1) == 0 and IR.island_seed(2 ** 64 - 1, 2) == 1


@pytest.mark.parametrize("nsga", [True, False])
def test_without_migration_islands_are_single_searches(nsga):
    """M = 0: after three generations island i is the single-search mirror under seed + i on its own rows, written out here with
    search_device_ref alone."""
    K, pop, nv, seed = 3, 8, 6, 2 ** 64 - 2      # (island 2's seed wraps to 0)
    ev = (lambda rows: toy(rows)) if nsga else (lambda rows: toy(rows)[:, :1])
    st = start(K, pop, nv, nsga)
    single = [dict(X=st["X"][i].copy(), F=st["F"][i].copy(), rank=st["rank"][i].copy(), cd=st["cd"][i].copy()) for i in range(K)]
    for gen in (1, 2, 3):
        st, info = IR.generation(st, ev, nsga, XL, XU, 3.0, 3.0, 0.5, seed, gen)
        assert info["accepted"] is None
        for i, s in enumerate(single):
            m = SR.vary(s["X"], s["rank"], s["cd"], XL, XU, 3.0, 3.0, 0.5, (seed + i) % 2 ** 64, gen)
            off = m["off32"]
            assert np.array_equal(SR.bits(off), SR.bits(info["off_X"][i]))
            flags = SR.duplicates(s["X"], off)
            Fm, Xm = np.concatenate([s["F"], ev(off)]), np.concatenate([s["X"], off])
            r = SR.survive(Fm, pop, pop, nsga, flags)
            s.update(X=Xm[r["chosen"]], F=Fm[r["chosen"]], rank=r["rank"], cd=r["cd"])
            for k in s:
                assert np.array_equal(np.asarray(s[k]).view(np.uint8), np.asarray(st[k][i]).view(np.uint8)), (gen, i, k)
        # the islands are different searches: the same operators under another seed
        assert not np.array_equal(SR.bits(info["off_X"][0]), SR.bits(info["off_X"][1]))


def test_generation_migrates_when_due():
    st = start(3, 8, 6, True)
    for gen, due in ((1, False), (2, True), (3, False), (4, True)):
        st, info = IR.generation(st, toy, True, XL, XU, 3.0, 3.0, 0.5, 7, gen, migrate_every=2, migrants=2)
        assert (info["accepted"] is not None) == due
    assert not IR.migration_due(0, 3, 1) and not IR.migration_due(2, 1, 1) and not IR.migration_due(2, 3, 0) and IR.migration_due(3, 3, 1)


def first_var(m, i):
    return [float(v) for v in m["X"][i, :, 0]]


def f0(m, i):
    return [float(v) for v in m["F"][i, :, 0]]


def run(name):
    X, F, rank, cd, n, nsga = CASES[name]
    return IR.migrate(X, F, rank, cd, n, nsga)


def test_ring_direction_two_islands():
    """K = 2: predecessor and successor coincide; each island's best row (F 0 and 0.25) replaces the other's worst."""
    m = run("ring_k2")
    assert f0(m, 0) == [0, 0.25, 1, 2, 3, 4] and first_var(m, 0) == [0, 100.25, 1, 2, 3, 4]
    assert f0(m, 1) == [0, 0.25, 2.25, 4.25, 6.25, 8.25] and first_var(m, 1) == [0, 100.25, 102.25, 104.25, 106.25, 108.25]
    assert list(m["accepted"]) == [1, 1] and (m["rank"] == 0).all() and np.array_equal(m["cd"], -m["F"][..., 0].astype(np.float64))


def test_ring_direction_three_islands():
    """Island i receives from island i - 1: 0 from 2, 1 from 0, 2 from 1."""
    m = run("ring_k3")
    assert first_var(m, 0) == [0, 200.5, 1, 2, 3, 4]
    assert first_var(m, 1) == [0, 100.25, 102.25, 104.25, 106.25, 108.25]
    assert first_var(m, 2) == [100.25, 200.5, 203.5, 206.5, 209.5, 212.5]
    assert list(m["accepted"]) == [1, 1, 1]


def test_two_migrants_and_half_the_population():
    m = run("two_migrants")
    assert first_var(m, 0) == [0, 200.5, 1, 2, 3, 203.5] and f0(m, 0) == [0, 0.5, 1, 2, 3, 3.5]
    assert first_var(m, 1) == [0, 100.25, 1, 102.25, 104.25, 106.25]
    m = run("half_pop")      # n = pop / 2: the three best of each island replace the three worst of the other
    assert f0(m, 0) == [0, 0.25, 1, 2, 2.25, 4.25] and first_var(m, 0) == [0, 100.25, 1, 2, 102.25, 104.25]
    assert f0(m, 1) == [0, 0.25, 1, 2, 2.25, 4.25] and first_var(m, 1) == [0, 100.25, 1, 2, 102.25, 104.25]
    assert list(m["accepted"]) == [3, 3]


def test_duplicates_are_dropped_and_their_slots_keep_their_rows():
    """n = 3.  Island 1 (F 0, .25, .25, 4.25, 8.25, 10.25) holds island 0's best row already: migrant 0 is dropped and the worst row (10.25)
    stays, migrants 1 and 2 (F 1, 2) replace the second and third worst.  Island 2 receives island 1's F 0 and .25 rows and drops the second
    .25 row, equal to the migrant before it: its third worst (9.5) stays."""
    m = run("duplicates")
    assert f0(m, 1) == [0, 0.25, 0.25, 1, 2, 10.25] and list(m["accepted"]) == [3, 2, 2]
    assert f0(m, 2) == [0, 0.25, 0.5, 3.5, 6.5, 9.5] and first_var(m, 2) == [0, 100.25, 200.5, 203.5, 206.5, 209.5]
    assert f0(m, 0) == [0, 0.5, 1, 2, 3.5, 6.5]


def test_negative_zero_equals_zero():
    X, F, rank, cd, n, nsga = CASES["negative_zero"]
    assert np.signbit(X[1]).any() and not np.array_equal(SR.bits(X[1, 2]), SR.bits(X[0, 0])) and IR.rows_equal(X[1, 2], X[0, 0])
    m = run("negative_zero")
    assert list(m["accepted"]) == [1, 0]
    for k, pre in (("X", X), ("F", F), ("rank", rank), ("cd", cd)):      # island 1 keeps every bit
        assert np.array_equal(np.asarray(m[k][1]).view(np.uint8), np.asarray(pre[1]).view(np.uint8)), k


def test_nsga_order_runs_through_infinite_distances():
    """Island A: front 0 = (1, 2.5), (0, 4), (2, 1), (4, 0) with distances 1.25, inf, 1.375, inf, front 1 = (5, 5), (6, 4.5); island B is A + 10.
    The three best of A in the order (rank, -cd, index) are (0, 4), (4, 0), (2, 1) — not its first three rows — and they go to B's worst
    rows (16, 14.5), (15, 15), (11, 12.5), worst first."""
    X, F, rank, cd, n, nsga = CASES["nsga_infinite"]
    assert list(rank[0]) == [0, 0, 0, 0, 1, 1] and list(cd[0]) == [1.25, np.inf, 1.375, np.inf, np.inf, np.inf]
    assert list(IR.order(rank[0], cd[0])) == [1, 3, 2, 0, 4, 5]
    m = IR.migrate(X, F, rank, cd, n, nsga)
    pairs = lambda i: [tuple(float(v) for v in r) for r in m["F"][i]]
    assert pairs(1) == [(2, 1), (4, 0), (0, 4), (10, 14), (12, 11), (14, 10)]
    assert list(m["rank"][1]) == [0, 0, 0, 1, 1, 1] and list(m["cd"][1]) == [2, np.inf, np.inf, np.inf, 2, np.inf]
    assert pairs(0) == [(0, 4), (2, 1), (4, 0), (12, 11), (14, 10), (10, 14)]
    assert list(m["rank"][0]) == [0, 0, 0, 1, 1, 1] and list(m["cd"][0]) == [np.inf, 2, np.inf, 2, np.inf, np.inf]
    assert np.array_equal(SR.bits(m["X"][..., :2]), SR.bits(m["F"])) and list(m["accepted"]) == [3, 3]


# which hand-made case exposes which planted fault
EXPOSES = dict(reversed_ring="ring_k3", reversed_order="duplicates", keep_duplicates="duplicates", no_rerank="ring_k3",
               read_after_write="two_migrants")


@pytest.mark.parametrize("fault", IR.FAULTS)
def test_checker_fails_on_planted_faults(fault):
    X, F, rank, cd, n, nsga = CASES[EXPOSES[fault]]
    IR.check_migration("right", IR.migrate(X, F, rank, cd, n, nsga), X, F, rank, cd, n, nsga)
    with pytest.raises(AssertionError):
        IR.check_migration(fault, IR.migrate(X, F, rank, cd, n, nsga, fault=fault), X, F, rank, cd, n, nsga)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_are_well_formed(name):
    """Every shared case is a state a survival leaves (ranking it again changes nothing for the GA; NSGA-II: the same fronts), n <= pop / 2, and
    the migration moves something."""
    X, F, rank, cd, n, nsga = CASES[name]
    assert 1 <= n <= X.shape[1] // 2
    m = IR.migrate(X, F, rank, cd, n, nsga)
    assert m["accepted"].sum() > 0 and not np.array_equal(SR.bits(m["X"]), SR.bits(X))
    for i in range(X.shape[0]):      # a migration keeps what it does not replace: the multiset of F rows changes by the accepted rows only
        kept = sum(1 for r in F[i] if any(np.array_equal(r, q) for q in m["F"][i]))
        assert kept >= X.shape[1] - m["accepted"][i]
