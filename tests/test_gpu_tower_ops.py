"""The convolutions, pools and token builder of the two scoring networks (CLIP's ResNet towers, the LPIPS VGG16 walk), each kernel instance alone
through its diagnostic op against tests/tower_ops_ref.py: a float64 reference of the fp16 operands and an error bound PER ELEMENT derived from
the kernel's own roundings (no term fitted to the device), and — on lattice inputs, where the result is unique — the bits.

Every case of tower_ops_ref.CASES asserts: the kernel symbol the launcher reports (ops.last_kernel) is the instance the case is there for; the
whole output is finite and inside its bound (the op's outputs are poisoned: an element no thread stored is NaN; guards on both sides of the
output fail the op on a store outside it); the four border slices of an image-shaped output are; and, for the lattice cases, the bytes equal
tower_ops_ref.lattice_premise's.  Where (2 K + 8) U32 A |a| dominates U16 |out| — K >= 2304: the 512-channel VGG convs — the bound is wider than
an fp16 ulp by construction; the lattice runs at K = 4608 (2 x 2 and 1 x 1 maps) are the sharp check there.

Shapes are the smallest that reach each instance (tower_ops_ref.CASES says why next to each); the fill-rule cases are derived from
launch_gemm_tiled and confirmed by the symbol assertion.  References are computed once per process (tower_ops_ref.case)."""
import numpy as np
import pytest

import tower_ops_ref as R
from clip_glass_amd import ops
from util import check_bound, diag

pytestmark = pytest.mark.gpu


def _run(name):
    """One case on the device: symbol, whole output, borders; returns (inputs, output)."""
    inp, ref, tol = R.case(name)
    got = R.run(inp)
    assert ops.last_kernel() == R.CASES[name][1], "%s ran %r, the case is there for %r" % (name, ops.last_kernel(), R.CASES[name][1])
    assert got.shape == ref.shape
    if inp.get("relu"):
        pos, zero = R.relu_sides(ref)
        assert pos > 0.2 and zero > 0.2      # (a condition on the inputs: both sides of the ReLU are populated)
    check_bound("tower op: " + name, got, ref, tol)
    for side, sl in R.border_slices(ref):
        check_bound("tower op: %s, %s border" % (name, side), got[sl], ref[sl], tol[sl], log=False)
    rel = tol / (R.U16 * np.abs(ref) + R.SUBNORMAL)      # the bound in units of the output's own fp16 rounding (huge at the zeros of a ReLU)
    diag("[tower] %-36s %-32s worst err/tol %.4f median tol / (U16 |out| + 2^-24) %.2f (%.2f where out != 0)"
         % (name, R.CASES[name][1], float((np.abs(got - ref) / tol).max()), float(np.median(rel)), float(np.median(rel[ref != 0]))))
    return inp, got


@pytest.mark.parametrize("name", sorted(n for n in R.CASES if n not in R.LATTICE_CASES))
def test_instance_in_bound(name):
    _run(name)


@pytest.mark.parametrize("name", R.LATTICE_CASES)
def test_lattice_bit_exact(name):
    """Exact accumulators in any order, an exact epilogue, one deterministic fp16 rounding: the device returns these bits."""
    inp, got = _run(name)
    bits = R.lattice_premise(name, inp)
    nbad = int((got != bits).sum())
    assert got.astype(np.float16).tobytes() == bits.astype(np.float16).tobytes(), "%s: %d of %d values differ from the lattice bits" % (name, nbad, bits.size)


@pytest.mark.parametrize("name", ["1x1 M12 K256 N192 res1 relu1", "gather rn 2x2 M12"])
def test_poisoned_tail_does_not_reach_a_valid_row(name):
    """M = 12 rows of data in buffers of 64: rows 12 .. 63 of x and res are NaN on the device (the engine's ping-pong buffers hold the previous
    layer's values there).  The 1 x 1 form computes and stores those rows, the gather form may fetch them for lanes past M; the 12 rows that
    come back are finite and inside their bound, so none of them depends on the tail."""
    inp, got = _run(name)
    assert int(np.prod(got.shape[:3])) == 12 and np.isfinite(got).all()


@pytest.mark.parametrize("B,H,C", [(2, 2, 8), (2, 6, 64)])
def test_maxpool2_reports_its_kernel_and_stays_exact(B, H, C):
    x = R.h16(np.random.default_rng(60 + H).standard_normal((B, H, H, C)))
    got = ops.maxpool2(x)
    assert ops.last_kernel() == "maxpool2_kernel" and got.tobytes() == R.maxpool_ref(x).tobytes()
