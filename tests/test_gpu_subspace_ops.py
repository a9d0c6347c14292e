"""dlatent_subspace_kernel (csrc/dlatent.hip) in isolation, through glass_op_dlatent_subspace: every element against the float64 rule under
its bar (tests/subspace_ref.py), and the identities that hold bit for bit — frozen layers, the zero row, a candidate wherever it sits in a
launch, the layers of one group."""
import numpy as np
import pytest

import subspace_ref as S
from clip_glass_amd import ops as O
from util import diag

pytestmark = pytest.mark.gpu
F32 = np.float32
NETS = [(32, 8), (64, 10), (512, 18)]
PMAX = 17


def _ks(L):
    return [1, 3, 32, L]


@pytest.fixture(scope="module")
def ops():
    return O


@pytest.mark.parametrize("L,n_lat", NETS)
@pytest.mark.parametrize("groups", ["one", "per_layer", "two_frozen_ends", "split_frozen_middle"])
def test_matches_the_rule_under_the_bar(ops, L, n_lat, groups):
    """K in {1, 3, 32, L} x P in {1, 5, 16, 17} (around the 16-candidate tile): the reference of the 17 rows is computed once per K, a launch
    of P rows is checked against its first P."""
    lg = S.layer_groups(n_lat)[groups]
    frozen = lg < 0
    for K in sorted(set(_ks(L))):
        c, B, base = S.case(100 + K, L, n_lat, K, lg, PMAX)
        ref, bar = S.expand(c, lg, B, base)
        for P in (1, 5, 16, 17):
            out = ops.dlatent_subspace(c[:P], lg, B, base)
            assert out.shape == (P, n_lat, L) and out.dtype == F32
            ok, worst, n_bad = S.within(out, ref[:P], bar[:P])
            diag("[subspace op] L%d n_lat%d K%d %s P%d: worst err / bar %.3f" % (L, n_lat, K, groups, P, worst))
            assert ok, "K %d P %d: %d elements outside the bar (worst ratio %.3f)" % (K, P, n_bad, worst)
            np.testing.assert_array_equal(out[:, frozen], np.broadcast_to(base[frozen], out[:, frozen].shape))


@pytest.mark.parametrize("L,n_lat", NETS)
def test_bitwise_identities(ops, L, n_lat):
    K = 32
    lg = S.layer_groups(n_lat)["split_frozen_middle"]
    c, B, base = S.case(9, L, n_lat, K, lg, PMAX)
    whole = ops.dlatent_subspace(c, lg, B, base)
    # a zero row gives base
    cz = c.copy()
    cz[3] = 0
    cz[16] = 0
    z = ops.dlatent_subspace(cz, lg, B, base)
    np.testing.assert_array_equal(z[3], base)
    np.testing.assert_array_equal(z[16], base)
    np.testing.assert_array_equal(z[4], whole[4])
    # a candidate alone, as row 0, as row 16, inside P = 17
    one = c[7:8]
    alone = ops.dlatent_subspace(one, lg, B, base)[0]
    np.testing.assert_array_equal(alone, whole[7])
    moved = np.concatenate([one, c[:15], one])                  # rows 0 and 16 of a launch of 17
    m = ops.dlatent_subspace(moved, lg, B, base)
    np.testing.assert_array_equal(m[0], alone)
    np.testing.assert_array_equal(m[16], alone)
    # the layers of one group: base[l] + acc, with acc read from a launch whose base is 0 (0 + acc is acc, bit for bit)
    acc = ops.dlatent_subspace(c, lg, B, np.zeros_like(base))
    for l in range(n_lat):
        if lg[l] < 0:
            assert not acc[:, l].any()
            continue
        first = int(np.nonzero(lg == lg[l])[0][0])
        np.testing.assert_array_equal(acc[:, l], acc[:, first])                       # one product per (candidate, group)
        np.testing.assert_array_equal(whole[:, l], base[l][None] + acc[:, first])      # fp32 add on the host
    assert any(lg[l] == lg[m_] and l != m_ for l in range(n_lat) for m_ in range(n_lat))


def test_refusals_reach_the_op_by_name(ops):
    L, n_lat = 32, 8
    lg = np.zeros(n_lat, np.int32)

    def run(K=4, G=1, lg=lg, L=L):
        return ops.dlatent_subspace(np.zeros((2, G, K), F32), lg, np.zeros((K, L), F32), np.zeros((len(lg), L), F32))
    run()
    with pytest.raises(RuntimeError, match="components must be at least 1"):
        run(K=0)
    with pytest.raises(RuntimeError, match="components must not exceed latent_size 32"):
        run(K=33)
    with pytest.raises(RuntimeError, match="components must not exceed 512"):
        ops.dlatent_subspace(np.zeros((1, 1, 513), F32), np.zeros(2, np.int32), np.zeros((513, 1024), F32), np.zeros((2, 1024), F32))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        run(L=30)
    with pytest.raises(RuntimeError, match="group 1 is empty"):
        run(G=2)
    with pytest.raises(RuntimeError, match=r"layer_group\[2\] = 1 must be -1 \(frozen\) or a group index in \[0, 1\)"):
        run(lg=np.array([0, 0, 1, 0, 0, 0, 0, 0], np.int32))
    with pytest.raises(RuntimeError, match="groups must not exceed n_lat 8"):
        run(G=9, lg=np.arange(8, dtype=np.int32))
    with pytest.raises(ValueError, match="basis must be"):
        ops.dlatent_subspace(np.zeros((2, 1, 4), F32), lg, np.zeros((5, L), F32), np.zeros((n_lat, L), F32))
