"""The perceptual objective's own kernels (csrc/lpips.hip), each alone through its diagnostic op against tests/lpips_ref.py.

Bars: the input kernel sums the box in fp32 and rounds once to fp16 — at most one fp16 ulp of the float64 value; the first convolution is
held to tests/tower_ops_ref.py's error bound per element (27 fp32 FMAs, the bias, one fp16 store); the max pool is exact; the head is all
fp32 on fp16 inputs it reads exactly — 1e-5 relative (fp32 sums of at most 512 x 1024 terms of one sign).  The twelve gather convolutions
of the walk are tests/test_gpu_tower_ops.py's "vgg" cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
import tower_ops_ref as T
from clip_glass_amd import ops, synth
from util import check_bound

pytestmark = pytest.mark.gpu


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("box", [1, 2, 4])
def test_input_box_mean_and_scale(box):
    S, B = 16, 3
    y = synth.normal(40, "y%d" % box, (B, 3, S * box, S * box), std=0.6)       # unclamped: values past [-1, 1] too
    got = ops.lpips_input(y, S)
    assert got.shape == (B, S, S, 4) and (got[..., 3] == 0).all()
    ref = R.scale_input(R.area(y, S)).numpy().transpose(0, 2, 3, 1)
    ulp = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64)
    err = np.abs(got[..., :3].astype(np.float64) - ref)
    print("lpips_input box %d: max err / ulp %.3f" % (box, (err / ulp).max()))
    assert (err <= ulp).all()


def test_input_refusals_are_named():
    y = np.zeros((1, 3, 48, 48), np.float32)
    for S in (32, 4):       # 48 % 32 != 0; box 12
        with pytest.raises(RuntimeError, match="lpips_input: refused"):
            ops.lpips_input(y, S)


@pytest.mark.parametrize("S", [16, 32])
def test_vgg_conv1(S):
    B = 3
    x = np.zeros((B, S, S, 4), np.float32)
    x[..., :3] = h16(synth.normal(41, "x%d" % S, (B, S, S, 3), std=2.0))
    w = h16(synth.normal(41, "w", (64, 3, 3, 3), std=(2.0 / 27) ** 0.5))
    b = synth.normal(41, "b", (64,), std=0.05)
    got = ops.vgg_conv1(x, w, b)
    ref = torch.relu(F.conv2d(torch.tensor(x[..., :3].transpose(0, 3, 1, 2), dtype=torch.float64), torch.tensor(w, dtype=torch.float64),
                              torch.tensor(b, dtype=torch.float64), padding=1)).numpy().transpose(0, 2, 3, 1)
    assert got.shape == ref.shape == (B, S, S, 64) and ops.last_kernel() == "vgg_conv1_kernel"
    ref64, tol = T.conv_bn_ref(x[..., :3], w, np.ones(64), b, mfma=False)
    assert np.abs(ref64 - ref).max() <= 1e-12 * np.abs(ref).max()      # (the bound's reference is the float64 conv above)
    for name, sl in (("all", np.s_[:]), ("top", np.s_[:, 0]), ("bottom", np.s_[:, -1]), ("left", np.s_[:, :, 0]), ("right", np.s_[:, :, -1])):
        check_bound("vgg_conv1 S%d %s" % (S, name), got[sl], ref64[sl], tol[sl])
    assert (ref > 0).mean() > 0.2 and (ref == 0).mean() > 0.2       # both sides of the ReLU


@pytest.mark.parametrize("B,H,C", [(3, 2, 64), (2, 6, 128), (1, 16, 512)])
def test_maxpool2_is_exact(B, H, C):
    x = h16(synth.normal(42, "x", (B, H, H, C)))
    got = ops.maxpool2(x)
    ref = x.reshape(B, H // 2, 2, H // 2, 2, C).max(axis=(2, 4))
    assert got.shape == ref.shape and (got == ref).all()


def test_maxpool2_refuses_an_odd_side():
    with pytest.raises(RuntimeError, match="maxpool2: refused"):
        ops.maxpool2(np.zeros((1, 3, 3, 64), np.float32))


def _head_ref(x0, x1, lin):
    t = lambda a: np.asarray(a, np.float64).transpose(0, 2, 1)[..., None]       # [n, HW, C] -> [n, C, HW, 1]
    return R.head_term(t(x0), t(np.broadcast_to(x1, x0.shape)), lin).numpy()


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("HW", [1, 1024])
def test_head(C, HW):
    """n = 3 images; HW = 1024 is four workgroups per image.  Rows of zeros in one map, the other, or both take the eps path: finite, and
    exactly 0 where both are zero."""
    n = 3
    x0 = np.maximum(h16(synth.normal(43, "a", (n, HW, C))), 0)
    x1 = np.maximum(h16(synth.normal(43, "b", (n, HW, C))), 0)
    x0[0, 0] = 0
    x1[1, HW - 1] = 0
    lin = (synth._rng(43, "lin").random((C,), dtype=np.float32) / C).astype(np.float32)
    got = ops.lpips_head(x0, x1, lin)
    ref = _head_ref(x0, x1, lin)
    rel = np.abs(got - ref) / ref
    print("lpips_head C%d HW%d: max rel %.3e" % (C, HW, rel.max()))
    assert np.isfinite(got).all() and (rel <= 1e-5).all()
    shared = ops.lpips_head(x0, x1[:1], lin)                                   # one target map for every image
    assert (np.abs(shared - _head_ref(x0, x1[:1], lin)) <= 1e-5 * _head_ref(x0, x1[:1], lin)).all()
    assert shared[0] == got[0]
    assert (ops.lpips_head(x0, x0, lin) == 0).all()                            # equal maps: exactly 0 (no fused multiply-subtract)
    z = np.zeros((n, HW, C), np.float32)
    assert (ops.lpips_head(z, z, lin) == 0).all()


def test_head_value_does_not_depend_on_the_row():
    """The same image at row 0 and at row 2 of a launch: the same bits."""
    C, HW = 256, 320                                                           # two workgroups, the second partly filled
    a = np.maximum(h16(synth.normal(44, "a", (1, HW, C))), 0)
    o = np.maximum(h16(synth.normal(44, "o", (2, HW, C))), 0)
    t = np.maximum(h16(synth.normal(44, "t", (1, HW, C))), 0)
    lin = (synth._rng(44, "lin").random((C,), dtype=np.float32) / C).astype(np.float32)
    first = ops.lpips_head(np.concatenate([a, o]), t, lin)
    last = ops.lpips_head(np.concatenate([o, a]), t, lin)
    alone = ops.lpips_head(np.concatenate([a, a]), t, lin)
    assert first[0].tobytes() == last[2].tobytes() == alone[0].tobytes() == alone[1].tobytes()
    assert first[1].tobytes() == last[0].tobytes()


def test_head_refuses_other_widths():
    with pytest.raises(RuntimeError, match="lpips_head: refused"):
        ops.lpips_head(np.zeros((1, 4, 96), np.float32), np.zeros((1, 4, 96), np.float32), np.zeros((96,), np.float32))
