"""The directional form of cosine_set_kernel (csrc/score.hip) and latent_anchor_kernel (csrc/edit.hip) in isolation, through the diagnostic ops.

Against float64 (tests/edit_ref.py): the project's general bar — |got - ref64| <= 4 * max|ref32 - ref64| on the same inputs, one spacing of
max|ref| where the float32 twin is exact.  tests/test_edit_ref.py shows that the bar bites at these inputs.  The twin is written in the
kernel's documented order, so the number of elements whose bits differ from it is logged too (it is not asserted: the bar is the contract).

Directional cosine: D = 32, 100, 512, 1024; T = 1, 4, 5 (a ragged last group of accumulators), 16; V = 1, 3, 16; P = 1, 5; and T = 16,
D = 1040, whose set exceeds 64 KB and streams from memory.  Inputs are independent normal rows, |x| of order 1.  The near-source regime is
checked by properties only: a feature row that is an exact positive power-of-two multiple of its (exactly unit-length) source row gives
exactly 0.  Bit-equalities: a row moved to another position and another P; T = 1 against the first column of T = 16; the staged against the
streamed form at a D both accept; every case of the D / T / V / P grid, staged and streamed, against what cosine_set_dir_kernel of the commit
before score.hip returned (tests/score_tail_golden.py).  Shapes outside the limits come back as the launcher's refusal.

Latent anchor: L = 64, 512; n_lat = 1, 4, 18; the [P, n_lat, L] form and the one-row-for-every-layer form; exact 0 for w = a; bit-equality
across positions.

Measured on an MI355X (every figure is logged through util.diag): all 4264 values compared with float64 have the bits of the float32 twin,
so every case sits at 0.25 of its bar (the twin's own error: 1e-8 to 2e-7 for cosines up to 0.4 in magnitude; anchor distances from 1e-6
to 2.8 within 1.5e-7 relative, against relative bars of 6.6e-7 to 9.2e-6); every bit-equality: 0 elements differ; every x = 0 case: all
values exactly 0."""
import os

import numpy as np
import pytest

import edit_ref as E
from score_tail_golden import golden, pack
from util import diag

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
F32 = np.float32


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
    diag("[edit] %-56s bit-exact: %d / %d elements differ" % (name, int(bad.sum()), bad.size))
    assert not bad.any(), "%s: %d elements differ, first at %s" % (name, int(bad.sum()), np.argwhere(bad)[0])


def _bar(name, got, ref64, ref32):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    tol = E.bar(ref64, ref32)
    err = np.abs(got - ref64)
    twin = int((_bits(got) != _bits(ref32)).sum())
    diag("[edit] %-56s max err %.3e  bar %.3e  max|ref| %.3e  bits differ from the twin: %d / %d" % (name, err.max(), tol, np.abs(ref64).max(), twin, got.size))
    assert np.isfinite(got).all(), "%s: non-finite values" % name
    assert (err <= tol).all(), "%s: max err %.3e, bar %.3e, %d elements beyond the bar" % (name, err.max(), tol, int((err > tol).sum()))


def _check_dir(ops, tag, feat, targets, weights, src):
    P, V, _ = feat.shape
    T = targets.shape[0]
    vs, ss, sim = ops.cosine_set_dir(feat, targets, weights, src)
    assert vs.shape == (P, V) and ss.shape == (P, T) and sim.shape == (P,)
    r64, r32 = E.cosine_set_dir(feat, targets, weights, src), E.cosine_set_dir(feat, targets, weights, src, dt=F32)
    _bar("%s columns" % tag, ss, r64[1], r32[1])
    _bar("%s entry 0 per view" % tag, vs, r64[0], r32[0])
    _bar("%s sim" % tag, sim, r64[2], r32[2])
    return vs, ss, sim


DIR_D, DIR_T, DIR_V, DIR_P = [32, 100, 512, 1024], [1, 4, 5, 16], (1, 3, 16), (1, 5)


@pytest.mark.parametrize("D", DIR_D)
@pytest.mark.parametrize("T", DIR_T)
def test_cosine_set_dir(ops, D, T):
    got = {False: [], True: []}
    for V in DIR_V:
        for P in DIR_P:
            case = E.dir_inputs(P, V, T, D)
            got[False] += _check_dir(ops, "D%d T%d V%d P%d" % (D, T, V, P), *case)
            got[True] += ops.cosine_set_dir(*case, streamed=True)
    for streamed in (False, True):
        _bit_equal("D%d T%d %s == the parent's cosine_set_dir_kernel" % (D, T, "streamed" if streamed else "staged"), pack(*got[streamed]),
                   golden("cosine_set_dir_D%d_T%d" % (D, T)))


def test_a_set_beyond_the_staging_limit_streams_from_memory(ops):
    """T * D * 4 bytes = 66560 > 64 KB: the kernel's other path, against the same references."""
    feat, targets, weights, src = E.dir_inputs(5, 3, 16, 1040)
    vs, ss, sim = _check_dir(ops, "streamed D1040 T16 V3 P5", feat, targets, weights, src)
    _bit_equal("streamed D1040: the op's streamed form is that launch", np.concatenate([vs.ravel(), ss.ravel(), sim]),
               np.concatenate([a.ravel() for a in ops.cosine_set_dir(feat, targets, weights, src, streamed=True)]))


@pytest.mark.parametrize("V,T,D", [(1, 4, 100), (3, 16, 512), (16, 5, 1024)])
def test_staged_and_streamed_forms_agree_bit_for_bit(ops, V, T, D):
    feat, targets, weights, src = E.dir_inputs(5, V, T, D)
    a = ops.cosine_set_dir(feat, targets, weights, src)
    b = ops.cosine_set_dir(feat, targets, weights, src, streamed=True)
    for name, x, y in zip(("view_sim", "set_sim", "sim"), a, b):
        _bit_equal("V%d T%d D%d %s staged == streamed" % (V, T, D, name), x, y)


@pytest.mark.parametrize("V,T,D", [(3, 16, 100), (1, 5, 512), (16, 4, 1024)])
def test_a_row_does_not_depend_on_its_position_or_on_P(ops, V, T, D):
    feat, targets, weights, src = E.dir_inputs(19, V, T, D)
    vs, ss, sim = ops.cosine_set_dir(feat, targets, weights, src)
    for p in (0, 3, 18):
        v1, s1, m1 = ops.cosine_set_dir(feat[p:p + 1], targets, weights, src)
        _bit_equal("V%d T%d D%d row %d of 19 == alone" % (V, T, D, p), np.concatenate([vs[p], ss[p], sim[p:p + 1]]), np.concatenate([v1[0], s1[0], m1]))
    moved = feat[[18, 0, 3]]                                  # other positions, another P
    v3, s3, m3 = ops.cosine_set_dir(moved, targets, weights, src)
    _bit_equal("V%d T%d D%d rows 18, 0, 3 as a launch of 3" % (V, T, D), np.concatenate([v3, s3, m3[:, None]], 1),
               np.concatenate([vs, ss, sim[:, None]], 1)[[18, 0, 3]])


@pytest.mark.parametrize("V,D", [(1, 100), (3, 512), (3, 1040)])
def test_one_entry_is_the_first_column_of_sixteen(ops, V, D):
    """A value is a function of (row, view, entry): entry 0 alone, entries 0 .. 4 (a ragged group) and all sixteen give column 0 the same bits."""
    feat, targets, weights, src = E.dir_inputs(5, V, 16, D)
    vs16, ss16, _ = ops.cosine_set_dir(feat, targets, weights, src)
    for T in (1, 5):
        vs, ss, _ = ops.cosine_set_dir(feat, targets[:T], weights[:T], src)
        _bit_equal("V%d D%d T%d columns == the first of T16" % (V, D, T), ss, ss16[:, :T])
        _bit_equal("V%d D%d T%d entry 0 per view == T16's" % (V, D, T), vs, vs16)


@pytest.mark.parametrize("V,T,D", [(1, 1, 32), (3, 5, 100), (16, 16, 1024), (3, 16, 1040)])
def test_a_power_of_two_multiple_of_the_source_row_gives_exactly_zero(ops, V, T, D):
    src = E.dyadic_unit_rows(V, D)                            # |src[v]| = 1 exactly, in any summation order
    feat = np.stack([src * F32(2.0 ** k) for k in (-3, 0, 1, 5)])
    _, targets, weights, _ = E.dir_inputs(4, V, T, D)
    vs, ss, sim = ops.cosine_set_dir(feat, targets, weights, src)
    for name, a in (("view_sim", vs), ("set_sim", ss), ("sim", sim)):
        diag("[edit] V%d T%d D%d x = 0: %s max |value| %.3e" % (V, T, D, name, np.abs(a).max()))
        assert not a.any() and np.isfinite(a).all(), name
    # the other way round: one candidate on its source, its neighbours not — a zero row leaves the rows beside it alone
    other, _, _, _ = E.dir_inputs(2, V, T, D)
    mixed = np.concatenate([other[:1], feat[:1], other[1:]])
    v2, s2, m2 = ops.cosine_set_dir(mixed, targets, weights, src)
    assert not s2[1].any() and s2[0].any() and s2[2].any()
    _bit_equal("V%d T%d D%d neighbours of a zero row" % (V, T, D), s2[[0, 2]], ops.cosine_set_dir(other, targets, weights, src)[1])


def test_ops_refuse_shapes_outside_the_limits(ops):
    feat, targets, weights, src = E.dir_inputs(2, 1, 2, 64)
    for streamed in (False, True):
        with pytest.raises(RuntimeError, match="cosine_set_dir refused the shape"):
            ops.cosine_set_dir(feat, np.zeros((17, 64), F32), np.ones(17, F32), src, streamed=streamed)
        with pytest.raises(RuntimeError, match="cosine_set_dir refused the shape"):
            ops.cosine_set_dir(np.zeros((1, 17, 64), F32), targets, weights, np.zeros((17, 64), F32), streamed=streamed)
    with pytest.raises(RuntimeError, match="latent_anchor refused the shape"):
        ops.latent_anchor(np.zeros((1, 65, 4), F32), np.zeros((65, 4), F32))
    with pytest.raises(ValueError):
        ops.latent_anchor(np.zeros((1, 3, 4), F32), np.zeros((2, 4), F32))


@pytest.mark.parametrize("L", [64, 512])
@pytest.mark.parametrize("n_lat", [1, 4, 18])
@pytest.mark.parametrize("layered", [True, False])
def test_latent_anchor(ops, L, n_lat, layered):
    tag = "L%d n_lat%d %s" % (L, n_lat, "per layer" if layered else "one row")
    w, a = E.anchor_inputs(7, n_lat, L, layered)
    d = ops.latent_anchor(w, a)
    assert d.shape == (7,)
    _bar(tag, d, E.latent_anchor(w, a), E.latent_anchor(w, a, dt=F32))
    # every candidate relative to its own float64 value too: the distances span six decades, and the bar above is set by the largest.  A sum
    # of non-negative float32 terms, each (w - a)^2 three roundings off, added K = ceil(n_lat L / 64) deep per lane and 6 deep across lanes,
    # then one division: at most (K + 10) roundings of 2^-24 each, relative
    d64 = E.latent_anchor(w, a)
    rel = np.abs(d - d64) / d64
    rel_bar = ((n_lat * L + 63) // 64 + 10) * 2.0 ** -24
    diag("[edit] %-56s max relative err %.3e  bar %.3e  d from %.3e to %.3e" % (tag, rel.max(), rel_bar, d64.min(), d64.max()))
    assert (rel <= rel_bar).all()
    # exact 0 for w = a (for the one-row form: an anchor whose layers are all that row)
    a0 = a if layered else np.repeat(a[:1], n_lat, 0)
    w0 = np.broadcast_to(a0, (3,) + a0.shape) if layered else np.repeat(a0[:1], 3, 0)
    assert not ops.latent_anchor(w0, a0).any()
    # positions: rows 6, 0, 3 as a launch of 3, and row 3 alone
    _bit_equal("%s rows 6, 0, 3 as a launch of 3" % tag, ops.latent_anchor(w[[6, 0, 3]], a), d[[6, 0, 3]])
    _bit_equal("%s row 3 alone" % tag, ops.latent_anchor(w[3:4], a), d[3:4])
    if not layered:
        _bit_equal("%s == the per-layer form of the repeated row" % tag, ops.latent_anchor(np.repeat(w[:, None], n_lat, 1), a), d)
