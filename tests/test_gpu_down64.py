"""conv_down64.hip — the 64 -> 128 discriminator block's second half in one kernel (FIR pad 2 + conv3x3 stride 2 + 1x1 skip + merge):
op level against the oracle's ops and against the two-pass GPU form it replaces, engine level on the smallest network that reaches it."""
import math

import numpy as np
import pytest
import torch

from clip_glass_amd import synth
from oracle import fitness_ref
from oracle import stylegan2_ref as sg
import glass_models as M
from util import check, check_logits, diag, nchw, nhwc

pytestmark = pytest.mark.gpu


def rnd(seed, name, shape, std=1.0):
    return synth.normal(seed, name, shape, std)


def h16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("B,R,Cin,Cout", [
    (2, 64, 64, 128),     # two tile columns, the second holding 3 of 29 pixels; both image borders in every window; every step primed
    (1, 116, 64, 128),    # R/2 = 58: exactly two tile columns, R % 64 != 0 (the gate asks R % 4 == 0 only)
    (3, 192, 64, 128),    # interior tiles with no mask; odd counts
    (4, 256, 64, 128),    # 1280 steps: 5 per persistent workgroup on 256 CUs, ranges crossing column and sample boundaries
])
def test_d_block_down64(B, R, Cin, Cout):
    """ops.dblock_down at 64 -> 128 (conv_down64.hip + launch_blur_down for the skip input) vs the oracle's ops on the same fp16-rounded
    inputs (test_d_block_down_fused's construction and tolerances), and vs blur pad 2 -> stride-2 conv with the fused skip branch, the
    two-pass form the engine ran on this block: the two differ in FIR order (vertical first here, horizontal first in blur_kernel), bound
    2^-7 * max(1, max|two-pass|) as in test_dblock0_fused."""
    from clip_glass_amd import ops
    h = rnd(14, "h", (B, Cin, R, R)); x = rnd(14, "x", (B, Cin, R, R))
    w1 = rnd(14, "w1", (Cout, Cin, 3, 3)); b1 = rnd(14, "b1", (Cout,), 0.3); ws = rnd(14, "ws", (Cout, Cin, 1, 1))
    ht, xt = torch.tensor(h16(h)), torch.tensor(h16(x))
    hb = sg._filter(ht, sg._fir(), 2, 2)
    h1 = sg._bias_act(sg._conv(hb, torch.tensor(w1), stride=2), torch.tensor(b1))
    xs = sg._filter(xt, sg._fir(), 1, 1)[:, :, ::2, ::2]
    ref = ((h1 + sg._conv(xs, torch.tensor(ws))) / math.sqrt(2)).numpy()
    got = ops.dblock_down(nhwc(h), nhwc(x), w1, ws, b1)
    check("D down64 B%d R%d %d->%d" % (B, R, Cin, Cout), nchw(got), ref, 6e-3)
    for name, sl in (("top", np.s_[:, :, :2, :]), ("bottom", np.s_[:, :, -2:, :]), ("left", np.s_[:, :, :, :2]), ("right", np.s_[:, :, :, -2:])):
        check("D down64 border " + name, nchw(got)[sl], ref[sl], 8e-3)
    # the two-pass GPU form: conv_s2 with the fused skip branch on 32-channel planes where it applies (R/2 % 32 == 0); else what the
    # walker falls back to on such a map, the 1x1 skip conv as a pass of its own and the stride-2 conv with it as the residual
    g_hb = ops.blur(h16(nhwc(h)), 2)
    g_xs = ops.blur(h16(nhwc(x)), 1)
    kw = dict(stride=2, pad=0, bias=b1, act=True, out_scale=2.0 ** -0.5)
    if (R // 2) % 32 == 0:
        two = ops.conv(g_hb, w1, impl=5, planar32_x=True, skip=(g_xs, ws), **kw)
    else:
        two = ops.conv(g_hb, w1, res=ops.conv(g_xs, ws, pad=0), **kw)
    d = np.abs(got - two)
    bound = 2.0 ** -7 * max(1.0, float(np.abs(two).max()))
    diag("[down64] B%d R%d vs two-pass: max|diff| %.3e (bound %.3e), %.2f%% of outputs differ" % (B, R, d.max(), bound, 100.0 * (d > 0).mean()))
    assert d.max() <= bound


_CH_FUSED = [32, 64, 128, 128]       # 32 px: D block 1 is 64 -> 128 at 16 x 16 (the gate: R >= 16, R % 4 == 0)
_CH_PLAIN = [32, 64, 64, 64]         # same depth, block 1 is 64 -> 64: the gate does not hold


def _engine_case(name, channels):
    M.CONFIGS[name] = dict(channels=channels, latent=32, mapping=2, clip=(64, 2, 1, 8, 32, 32))
    try:
        c = M.CONFIGS[name]
        P, bs = 4, 4
        sd = M.make_state(name, 0)
        x = synth.latents(1, P, c["latent"])
        planes = M.noise_planes(name, 77, 3, P // bs)
        detail = {}
        fitness_ref.evaluate({k: torch.as_tensor(v) for k, v in sd.items()}, x, np.ones(c["clip"][5], np.float32), bs, True,
                             lambda i: planes[i], clip_size=c["clip"][4], detail=detail)
        e = M.make_engine(name, sd, batch_size=bs, use_discriminator=True, max_pop=P, noise_mode=2, noise_seed=77)
        e.set_target(M.make_target(detail["features"].numpy()))
        e.set_profiling(True)
        e.evaluate(x, generation=3, noise=planes)
        det = e.details(P)
        names = [r["name"] for r in e.profile()]
        e.close()
        return det["dis"], detail["dis"].numpy()[:, 0], names
    finally:
        del M.CONFIGS[name]


def test_engine_reaches_down64():
    """A 32 px network whose second D block is 64 -> 128: D logits against the oracle within the engine parity tests' bar, the block on
    conv_down64_kernel with no blur pass of its own; with a 64 -> 64 block instead, the blur + stride-2 conv tags are back."""
    dis, dis_o, names = _engine_case("down64_fused", _CH_FUSED)
    check_logits("down64 engine D logits", dis, dis_o)
    assert "D.down.r8.64x128@conv_down64_kernel" in names, names
    assert "D.blur.r16" not in names and not any(n.startswith("D.conv1.r8.") for n in names), names
    dis, dis_o, names = _engine_case("down64_plain", _CH_PLAIN)
    check_logits("down64 engine (gate off) D logits", dis, dis_o)
    assert "D.blur.r16" in names and any(n.startswith("D.conv1.r8.64x64") for n in names), names
    assert not any("conv_down64" in n for n in names), names
