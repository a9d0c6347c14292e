"""cosine_set_kernel and assemble_F_kernel's pareto layout (csrc/score.hip) in isolation, through the diagnostic ops.

Bit-equalities (the contract of include/glass.h "Prompt sets"): column t of a set is the cosine_views op's answer for entry t alone; one entry
of weight 1 is the cosine / cosine_views op; `sim` is the numpy float32 recombination of the kernel's own columns (product and sum
rounded separately, divided by the ordered sum of |w|); a row's bits do not depend on the launch it is in; assemble_F_set is its float32 twin.
The cosine ops are one kernel now, so the equalities between them compare it with itself at T = 1: every case is also compared with what the
separate kernels of the commit before score.hip returned (tests/score_tail_golden.py), and so are two shapes that only the directional tests
had: T = 5 without views (a ragged last accumulator group) and V = T = 16 (c[v][t] full).

Against float64 (tests/prompt_set_ref.py): the general bar of tests/test_gpu_small_ops.py — |got - ref64| <= 4 * max|ref32 - ref64| on the
same inputs, one ulp of max|ref| where the float32 twin is exact.

Shapes: D = 100 (no multiple of 64), 512, 640; V = 1, 3; T = 1, 2, 16 (one, half and four accumulator groups); P = 5 with one all-zero
feature row and, from T = 2 on, one all-zero entry (both give 0); weights of mixed sign between 1e-3 and 1e3.

Measured on an MI355X (every figure is logged through util.diag), largest |got - ref64| over the V / T cases, and the largest float32-twin error among them:
columns 3.2e-8 / 8.0e-8 (D 100), 1.6e-8 / 4.7e-8 (D 512), 2.0e-8 / 8.7e-8 (D 640), |column| <= 0.22; sim 3.2e-8 at worst (|sim| <= 0.16);
the case closest to its bar is D 100, V 3, T 1 at 0.45 of it (3.17e-8 against 7.03e-8); every bit-equality: 0 elements differ.  The first
version of the kernel combined with HIP's __fmul_rn / __fadd_rn, which the compiler fused into one multiply-add: 1 of 5 rows was one ulp off
the float32 recombination at D 100, V 1, T 16 — the test that found it."""
import os

import numpy as np
import pytest

import prompt_set_ref as PR
from score_tail_golden import golden, pack
from util import diag

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
F32 = np.float32
P = 5


@pytest.fixture(scope="module")
def ops():
    from clip_glass_amd import ops as _ops
    return _ops


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _bit_equal(name, got, want):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    diag("[prompt-set] %-52s bit-exact: %d / %d elements differ" % (name, int(bad.sum()), bad.size))
    assert not bad.any(), "%s: %d elements differ, first at %s" % (name, int(bad.sum()), np.argwhere(bad)[0])


def _bar(name, got, ref64, ref32):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    e32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    tol = float(np.spacing(F32(np.abs(ref64).max()))) if e32 == 0.0 else 4 * e32
    err = np.abs(got - ref64)
    diag("[prompt-set] %-52s max err %.3e  float32 twin's %.3e  bar %.3e  max|ref| %.3e" % (name, err.max(), e32, tol, np.abs(ref64).max()))
    assert np.isfinite(got).all(), "%s: non-finite values" % name
    assert (err <= tol).all(), "%s: max err %.3e, float32 twin %.3e, %d elements beyond the bar" % (name, err.max(), e32, int((err > tol).sum()))


def _inputs(Pn, V, T, D, seed=11):
    rng = np.random.default_rng(seed + 1000 * V + 10 * T + D)
    feat = (rng.standard_normal((Pn, V, D)) + (np.arange(Pn)[:, None, None] % 3 - 1.0) * 0.5).astype(F32)
    targets = rng.standard_normal((T, D)).astype(F32)
    if Pn > 3:
        feat[3, V - 1] = 0                                  # an all-zero feature row
    if T >= 2:
        targets[T - 1] = 0                                  # an all-zero entry
    mags = np.array([1.0, 1e-3, 1e3, 0.37, 12.5, 2.0, 0.05, 300.0, 1.5, 0.9, 7.0, 0.011, 45.0, 3.0, 0.6, 1.0])[:T]
    weights = (mags * np.where(np.arange(T) % 3 == 1, -1.0, 1.0)).astype(F32)
    if T == 1:
        weights[:] = -2.5
    return feat, targets, weights


def _recombine(set_sim, weights):
    """numpy float32: the rule of include/glass.h, term by term."""
    acc = np.zeros(set_sim.shape[0], F32)
    W = F32(0)
    for t in range(set_sim.shape[1]):
        acc = (acc + (F32(weights[t]) * set_sim[:, t]).astype(F32)).astype(F32)
        W = F32(W + np.abs(F32(weights[t])))
    return (acc / W).astype(F32)


SET_D, SET_V, SET_T = [100, 512, 640], [1, 3], [1, 2, 16]
STREAMED = (2, 2, 16, 1088)                                 # P, V, T, D
EDGES = [(5, 1, 5, 100), (1, 16, 16, 64)]                   # a ragged last accumulator group without views; c[v][t] full


@pytest.mark.parametrize("D", SET_D)
@pytest.mark.parametrize("V", SET_V)
@pytest.mark.parametrize("T", SET_T)
def test_cosine_set(ops, D, V, T):
    tag = "D%d V%d T%d" % (D, V, T)
    feat, targets, weights = _inputs(P, V, T, D)
    vs, ss, sim = ops.cosine_set(feat, targets, weights)
    assert vs.shape == (P, V) and ss.shape == (P, T) and sim.shape == (P,)
    _bit_equal("%s == the parent's cosine_set_kernel" % tag, pack(vs, ss, sim), golden("cosine_set_P%d_V%d_T%d_D%d" % (P, V, T, D)))
    for t in range(T):
        vt, mt = ops.cosine_views(feat, targets[t])
        _bit_equal("%s column %d == cosine_views" % (tag, t), ss[:, t], mt)
        if t == 0:
            _bit_equal("%s entry 0 per view == cosine_views" % tag, vs, vt)
    assert (ss[3] == 0).all() if V == 1 else True           # the zero row (the only view of candidate 3)
    assert vs[3, V - 1] == 0
    if T >= 2:
        assert (ss[:, T - 1] == 0).all()                    # the zero entry
    _bit_equal("%s sim == float32 recombination of the columns" % tag, sim, _recombine(ss, weights))
    r64, r32 = PR.cosine_set(feat, targets, weights), PR.cosine_set(feat, targets, weights, dt=F32)
    _bar("%s columns" % tag, ss, r64[1], r32[1])
    _bar("%s entry 0 per view" % tag, vs, r64[0], r32[0])
    _bar("%s sim" % tag, sim, r64[2], r32[2])


@pytest.mark.parametrize("D", [100, 512])
@pytest.mark.parametrize("V", [1, 3])
def test_one_entry_of_weight_one_is_the_single_target_kernel(ops, D, V):
    feat, targets, _ = _inputs(P, V, 1, D)
    vs, ss, sim = ops.cosine_set(feat, targets, [1.0])
    v1, m1 = ops.cosine_views(feat, targets[0])
    _bit_equal("D%d V%d sim == cosine_views" % (D, V), sim, m1)
    _bit_equal("D%d V%d views == cosine_views" % (D, V), vs, v1)
    _bit_equal("D%d V%d views == cosine" % (D, V), vs, ops.cosine(feat.reshape(P * V, D), targets[0]).reshape(P, V))
    if V == 1:
        _bit_equal("D%d sim == cosine" % D, sim, ops.cosine(feat[:, 0], targets[0]))


@pytest.mark.parametrize("V,T,D", [(3, 16, 100), (1, 2, 512)])
def test_a_row_does_not_depend_on_its_launch(ops, V, T, D):
    feat, targets, weights = _inputs(19, V, T, D)
    vs, ss, sim = ops.cosine_set(feat, targets, weights)
    for p in (0, 3, 18):
        v1, s1, m1 = ops.cosine_set(feat[p:p + 1], targets, weights)
        _bit_equal("V%d T%d D%d row %d of 19 == alone" % (V, T, D, p), np.concatenate([vs[p], ss[p], sim[p:p + 1]]),
                   np.concatenate([v1[0], s1[0], m1]))


def test_targets_beyond_the_staging_limit_stream_from_memory(ops):
    """T * D * 4 bytes > 64 KB: the kernel's other path, the same bits per column."""
    feat, targets, weights = _inputs(*STREAMED)
    vs, ss, sim = ops.cosine_set(feat, targets, weights)
    _bit_equal("streamed == the parent's cosine_set_kernel", pack(vs, ss, sim), golden("cosine_set_P%d_V%d_T%d_D%d" % STREAMED))
    for t in (0, 7, 15):
        _bit_equal("streamed column %d == cosine_views" % t, ss[:, t], ops.cosine_views(feat, targets[t])[1])
    _bit_equal("streamed sim == recombination", sim, _recombine(ss, weights))


@pytest.mark.parametrize("Pn,V,T,D", EDGES)
def test_shapes_that_only_the_directional_tests_had(ops, Pn, V, T, D):
    tag = "P%d V%d T%d D%d" % (Pn, V, T, D)
    feat, targets, weights = _inputs(Pn, V, T, D)
    vs, ss, sim = ops.cosine_set(feat, targets, weights)
    _bit_equal("%s == the parent's cosine_set_kernel" % tag, pack(vs, ss, sim), golden("cosine_set_P%d_V%d_T%d_D%d" % (Pn, V, T, D)))
    _bit_equal("%s sim == float32 recombination of the columns" % tag, sim, _recombine(ss, weights))
    r64, r32 = PR.cosine_set(feat, targets, weights), PR.cosine_set(feat, targets, weights, dt=F32)
    _bar("%s columns" % tag, ss, r64[1], r32[1])
    _bar("%s entry 0 per view" % tag, vs, r64[0], r32[0])
    _bar("%s sim" % tag, sim, r64[2], r32[2])


F_SET_P, F_SET_K, F_SET_COLS = [1, 65], [2, 4], [(False, False), (True, False), (False, True), (True, True)]


def _assemble_F_set_case(Pn, K, has_d, has_lp):
    rng = np.random.default_rng(3 + Pn + K)
    c = rng.uniform(-1, 1, (Pn, K)).astype(F32)
    w = np.array([2.0, -0.5, 1e-3, -40.0], F32)[:K]
    dis = rng.uniform(-2, 3, Pn).astype(F32) if has_d else None      # both sides of the hinge
    lp = rng.uniform(0, 1, Pn).astype(F32) if has_lp else None
    return c, w, dis, lp


@pytest.mark.parametrize("Pn", F_SET_P)
@pytest.mark.parametrize("K", F_SET_K)
@pytest.mark.parametrize("has_d,has_lp", F_SET_COLS)
def test_assemble_F_set(ops, Pn, K, has_d, has_lp):
    c, w, dis, lp = _assemble_F_set_case(Pn, K, has_d, has_lp)
    got = ops.assemble_F_set(c, w, dis, lp)
    assert got.shape == (Pn, K + has_d + has_lp)
    _bit_equal("assemble_F_set P%d K%d d%d lp%d == the parent's" % (Pn, K, has_d, has_lp), pack(got),
               golden("assemble_F_set_P%d_K%d_d%d_lp%d" % (Pn, K, has_d, has_lp)))
    _bit_equal("assemble_F_set P%d K%d d%d lp%d" % (Pn, K, has_d, has_lp), got, PR.assemble_F_set(c, w, dis, lp, dt=F32))
    assert (np.sign(got[:, 1]) == np.sign(c[:, 1])).all() and (np.sign(got[:, 0]) == -np.sign(c[:, 0])).all()


def test_ops_refuse_shapes_outside_the_limits(ops):
    feat, targets, weights = _inputs(2, 1, 2, 64)
    with pytest.raises(RuntimeError, match=r"\[1, 16\]"):
        ops.cosine_set(feat, np.zeros((17, 64), F32), np.ones(17, F32))
    with pytest.raises(RuntimeError, match=r"\[1, 16\]"):
        ops.cosine_set(np.zeros((1, 17, 64), F32), targets, weights)
