"""tests/conv_ops_ref.py on the CPU: the float64 reference agrees with the oracle, its per-element bound admits an fp32 emulation of a faithful
kernel at every case the GPU file runs, and every planted defect — applied to that emulation's output, in numpy — leaves the bound of every
kernel family, the loosest (conv_stream's three fp16 roundings) included.  No GPU; the built library's host code packs the weights."""
import math

import numpy as np
import pytest
import torch

import conv_ops_ref as R
from oracle import stylegan2_ref as sg
from util import check, check_bound, nchw, nhwc

FAMILIES = sorted(R.KERNELS)


def _oracle(inp):
    """oracle.stylegan2_ref of one launch (test_gpu_ops._oracle_conv's construction: the latent IS the style, no demodulation inside _mod_conv),
    then the epilogue as the kernels apply it."""
    B = inp["B"]
    xt = torch.tensor(nchw(np.broadcast_to(inp["x"], (B,) + inp["x"].shape[1:])))
    w = torch.tensor(inp["w"])
    Cin = xt.shape[1]
    if inp.get("sn") is None:
        y = sg._conv(xt, w, stride=inp["stride"], padding=inp["pad"])
    else:
        y = sg._mod_conv(xt, torch.tensor(inp["sn"]), w, torch.eye(Cin) * math.sqrt(Cin), torch.zeros(Cin), demod=False, up=False)
    if inp.get("dscale") is not None:
        y = y * torch.tensor(inp["dscale"])[:, :, None, None]
    if inp.get("noise") is not None:
        y = y + inp["noise_strength"] * torch.tensor(inp["noise"]).repeat_interleave(inp["batch_size"], dim=0)[:, None]
    if inp.get("bias") is not None:
        y = sg._bias_act(y, torch.tensor(inp["bias"]), act=inp["act"])
    if inp.get("res") is not None:
        y = y + torch.tensor(nchw(inp["res"]))
    return nhwc((y * inp["out_scale"]).numpy())


@pytest.mark.parametrize("family", ["conv_direct", "conv_tiled", "conv_glds", "conv_wreg"])      # x / sn, x / sn16, w / sn16, premod
@pytest.mark.parametrize("shape", [(3, 6, 10, 32, 24), (2, 9, 5, 48, 40)])
def test_reference_matches_the_oracle(family, shape):
    B, H, W, Cin, Cout = shape
    inp = R.make_inputs(B, H, W, Cin, Cout, batch_size=1, res=True, **R.FULL)
    ref, tol = R.conv_ref(inp, family)
    assert (tol > 0).all() and np.isfinite(ref).all()
    # 4e-4 max|ref|: what a float64 conv on the device's rounded operands leaves against the oracle's fp32 weights (test_gpu_conv_engine_forms.py)
    check("conv_ref[%s] vs oracle %s" % (family, (shape,)), ref, _oracle(inp), 4e-4)


@pytest.mark.parametrize("shape", [(2, 6, 10, 32, 24), (1, 9, 5, 48, 40)])
def test_reference_matches_the_oracle_unstyled(shape):
    B, H, W, Cin, Cout = shape
    for kw in (dict(), dict(KS=1, pad=0, bias=False, act=False), dict(stride=2, pad=0, res=True, out_scale=0.7)):
        inp = R.make_inputs(B, H, W, Cin, Cout, **kw)
        check("conv_ref unstyled %s %s" % (shape, sorted(kw)), R.conv_ref(inp, "conv_direct")[0], _oracle(inp), 4e-4)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_bound_admits_a_faithful_kernel(name):
    """An fp32 emulation (torch float32 conv of the mirrored operands, the epilogue in float32 — conv_stream: in packed fp16 — and the fp16 store)
    lies inside the bound everywhere, at every case of the GPU file: the inputs chosen let a correct kernel pass."""
    family, _, _, args = R.CASES[name]
    inp = R.make_inputs(**args)
    ref, tol = R.conv_ref(inp, family)
    check_bound("emulation in bound: " + name, R.Emulation(inp, family).finish(), ref, tol, log=False)


# ---- planted defects ------------------------------------------------------------------------------------------------------------------------------
TEETH = dict(B=4, H=16, W=32, Cin=64, Cout=32, batch_size=2, res=True, **R.FULL)      # two 32-channel chunks, two noise minibatches, one 8 x 32 tile row pair


def _defects(inp, family):
    """name -> the emulation's output with that defect planted."""
    em = R.Emulation(inp, family)
    clean = em.finish()
    B, H, W, Cin = em.a.shape
    out = {}
    # (a) one 32-channel chunk (the second) of one tap (ty 0, tx 0: inside the image there) dropped at the right border column of sample 1
    b, tap, ty, tx = 1, 0, 0, 0
    bw = em.b[b if em.b.shape[0] > 1 else 0][tap][:, 32:64].astype(np.float64)           # [Cout, 32]
    ap = np.pad(em.a[b].astype(np.float64), ((1, 1), (1, 1), (0, 0)))[:, :, 32:64]       # zero padding
    contrib = np.einsum("hc,oc->ho", ap[ty:ty + H, W - 1 + tx], bw)                       # output column W - 1 reads input column W - 2 + tx
    assert np.abs(contrib).max() > 0
    acc = em.acc.copy()
    acc[b, :, W - 1, :] -= contrib.astype(np.float32)
    out["a: chunk of a tap dropped"] = em.finish(acc=acc)
    # (b) sample 2 (minibatch 1) with the noise plane of minibatch 0
    nz = R._planes(inp, H, W).copy()
    nz[2] = nz[0]
    out["b: noise plane of minibatch m-1"] = em.finish(noise_planes=nz)
    # (c) sample 1 staged with candidate 3's style
    other = dict(inp, sn=inp["sn"].copy())
    other["sn"][1] = inp["sn"][3]
    d = clean.copy()
    d[1] = R.Emulation(other, family).finish()[1]
    out["c: another candidate's style"] = d
    # (d) one 8 x 32 tile of sample 0 holds the result for other weights (the previous launch's values)
    prev = R.Emulation(dict(inp, w=np.random.default_rng(5).standard_normal(inp["w"].shape).astype(np.float32)), family).finish()
    d = clean.copy()
    d[0, 8:16, 0:32] = prev[0, 8:16, 0:32]
    out["d: stale tile (other weights)"] = d
    # (e) the zero padding above sample 2 replaced by sample 1's last row
    ext = np.concatenate([em.a[1, H - 1:H], em.a[2]], axis=0)[None]                        # H + 1 rows: the row above row 0 is the neighbour's
    acc = em.acc.copy()
    acc[2, 0] = em.accumulate(ext, em.b[2:3] if em.b.shape[0] > 1 else em.b)[0, 1]
    out["e: neighbour's row for the top padding"] = em.finish(acc=acc)
    # (f) the residual added before the activation
    out["f: res before the activation"] = em.finish(res_before_act=True)
    return clean, out


@pytest.mark.parametrize("family", FAMILIES)
def test_bound_has_teeth(family):
    inp = R.make_inputs(**TEETH)
    ref, tol = R.conv_ref(inp, family)
    clean, defects = _defects(inp, family)
    check_bound("teeth[%s] clean" % family, clean, ref, tol, log=False)
    assert len(defects) == 6
    for name, got in defects.items():
        ratio = float((np.abs(got.astype(np.float64) - ref) / tol).max())
        print("[teeth] %-12s %-42s worst err/tol %.1f" % (family, name, ratio))
        assert ratio > 1, "%s: defect '%s' stays inside the bound (worst err/tol %.3f)" % (family, name, ratio)
        with pytest.raises(AssertionError):
            check_bound("teeth[%s] %s" % (family, name), got, ref, tol, log=False)


def test_stale_tile_under_the_old_bar_and_the_new():
    """Defect (d) as the suite saw it before the outputs were poisoned.  The old tests compared a kernel with its sibling at 4e-3 max|ref|, both
    launched at the same sizes: a tile the kernel under test never stored could hold the sibling's result from the launch before.  Old verdict:
    passes (the tile IS the reference).  With poisoned staging the tile is NaN, and against the float64 bound a tile from any other launch
    (other weights) is outside: both fail."""
    inp = R.make_inputs(**TEETH)
    got = R.Emulation(inp, "conv_tiled").finish()
    sibling = R.Emulation(inp, "conv_direct").finish()
    ref, tol = R.conv_ref(inp, "conv_tiled")
    tile = np.s_[0, 8:16, 0:32]
    stale = got.copy()
    stale[tile] = sibling[tile]                                  # raw staging: the pages of the sibling's output came back
    check("old bar: stale tile vs sibling", stale, sibling, 4e-3)     # passes: the missing tile is invisible
    print("[stale tile] old bar (4e-3 max|ref| against the sibling): PASS — the defect is invisible")
    poisoned = got.copy()
    poisoned[tile] = np.nan                                      # poisoned staging: nobody stored the tile
    with pytest.raises(AssertionError, match="non-finite"):
        check_bound("new: poisoned tile", poisoned, ref, tol, log=False)
    other = R.Emulation(dict(inp, w=np.random.default_rng(5).standard_normal(inp["w"].shape).astype(np.float32)), "conv_tiled").finish()
    prev = got.copy()
    prev[tile] = other[tile]
    with pytest.raises(AssertionError, match="exceed their bound"):
        check_bound("new: tile of another launch", prev, ref, tol, log=False)
    old_sees_other = float(np.abs(prev - sibling).max()) > 4e-3 * float(np.abs(sibling).max())
    print("[stale tile] new: poisoned tile -> FAIL (non-finite); tile of other weights -> FAIL under the bound (old bar: %s)" % ("FAIL" if old_sees_other else "PASS"))
