"""tests/glue_ops_ref.py on the CPU: (1) its float64 references are the oracle's operations (oracle/stylegan2_ref.py: _filter with _fir,
_conv + _bias_act behind utils.py's denorm, _mod_conv without demodulation + _upsample_skip); (2) its bars have teeth: on the inputs of the
GPU cases (tests/test_gpu_glue_ops.py) a float32 emulation of the correct arithmetic passes check_bound and each of seven subtly wrong kernels
fails it.  CPU only.

Bars of (1), the convention of test_small_ops_ref.py: 1e-11 * max|ref| where the oracle stays in float64 when fed float64 tensors (_fir's
taps k / 64 are exact in either format, so the filter is passed as float64), 2e-6 * max|ref| where it computes in float32 (_upsample_skip
builds its float32 ones / FIR tensors itself)."""
import math

import numpy as np
import pytest
import torch

import glue_ops_ref as R
from oracle import stylegan2_ref as sg
from util import check_bound, nchw, nhwc

f32 = np.float32


def _close(name, got, ref, rel):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= rel * float(np.abs(ref).max()), "%s: max err %.3e vs max|ref| %.3e" % (name, err, np.abs(ref).max())


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ---- (1) the references are the oracle's operations -----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", [(4, 8), (7, 3), (16, 24)])
def test_blur_is_filter(H, C):
    x = np.random.default_rng(H).standard_normal((2, C, H, H))
    fir = sg._fir().double()
    with torch.no_grad():
        pad2 = sg._filter(_t64(x), fir, 2, 2).numpy()
        down = sg._filter(_t64(x), fir, 1, 1)[:, :, ::2, ::2].numpy()
    ref, A = R.blur(nhwc(x), 2, 1)
    assert ref.shape == (2, H + 1, H + 1, C)
    _close("blur pad 2", nchw(ref), pad2, 1e-11)
    _close("blur pad 2, A", A, R.blur(np.abs(nhwc(x)), 2, 1)[0], 1e-14)
    ref, A = R.blur(nhwc(x), 1, 2)
    _close("blur pad 1 ::2", nchw(ref), down, 1e-11)
    assert (A >= np.abs(ref) * (1 - 1e-12)).all()


@pytest.mark.parametrize("R_,Cout", [(4, 8), (9, 20)])
def test_fromrgb_is_conv_bias_act(R_, Cout):
    rng = np.random.default_rng(R_)
    y = 0.9 * rng.standard_normal((2, 3, R_, R_)); w = rng.standard_normal((Cout, 3, 1, 1)); b = 0.3 * rng.standard_normal(Cout)
    y.reshape(-1)[:5] = [-1, 1, 1.5, -1.5, 0]
    with torch.no_grad():
        img = ((_t64(y) + 1) / 2).clip(0, 1) * 2 - 1                  # utils.py:19-21 (denorm), back to (-1, 1) as D takes it
        ref = sg._bias_act(sg._conv(img, _t64(w)), _t64(b)).numpy()
    got, A = R.fromrgb(y, w.reshape(Cout, 3) / math.sqrt(3), b)
    _close("fromrgb", nchw(got), ref, 1e-11)
    assert (A * math.sqrt(2) >= np.abs(got) * (1 - 1e-12)).all()


@pytest.mark.parametrize("H,C", [(4, 16), (6, 40)])
def test_torgb_is_mod_conv_plus_upsample_skip(H, C):
    B, L = 3, 24
    rng = np.random.default_rng(C)
    x = rng.standard_normal((B, C, H, H)); w = rng.standard_normal((3, C, 1, 1)); lat = rng.standard_normal((B, L))
    lat[1] *= 5.0                                                        # smax far from the other samples'
    dw = rng.standard_normal((C, L)); db = 1 + 0.2 * rng.standard_normal(C); bias = 0.3 * rng.standard_normal(3)
    yprev = rng.standard_normal((B, 3, H // 2, H // 2)).astype(f32)
    with torch.no_grad():
        t = sg._bias_act(sg._mod_conv(_t64(x), _t64(lat), _t64(w), _t64(dw), _t64(db), demod=False, up=False), _t64(bias), act=False).numpy()
        up = sg._upsample_skip(torch.from_numpy(yprev)).numpy()          # float32 inside
    s = lat @ (dw / math.sqrt(L)).T + db                                 # the style affine; the device gets it as sn * smax
    smax = np.abs(s).max(axis=1)
    args = (nhwc(x), w.reshape(3, C) / math.sqrt(C), bias, s / smax[:, None], smax)
    ref0, A0 = R.torgb(*args, None)
    _close("torgb, first layer", ref0, t, 1e-11)
    ref1, A1 = R.torgb(*args, yprev)
    _close("torgb + skip", ref1, t + up, 2e-6)
    _close("the skip term alone", ref1 - ref0, up, 2e-6)
    assert (A0 >= np.abs(ref0) * (1 - 1e-12)).all() and (A1 >= A0).all()


# ---- (2) float32 emulations of the kernels' arithmetic, with the mutants as switches ---------------------------------------------------
def emu_torgb(x16, wrgb, bias, sn, smax, yprev, swap_odd_cols=False, smax_of_sample0=False, group_from_neighbour=False):
    """torgb_kernel / torgb_pix_kernel in float32: w = wrgb * (sn * smax); per 8-channel group a running sum, the groups added as a tree
    (the xor-shuffle reduction), + bias, + the four-tap skip sum."""
    x = np.asarray(x16, f32)
    B, H, W, C = x.shape
    sm = np.asarray(smax, f32)
    if smax_of_sample0:
        sm = np.full_like(sm, sm[0])
    wm = (np.asarray(wrgb, f32)[None] * (np.asarray(sn, f32) * sm[:, None])[:, None, :]).astype(f32)      # [B,3,C]
    if group_from_neighbour:
        wm[:, :, 8:16] = wm[:, :, 0:8]
    part = []
    for g in range(C // 8):
        a = np.zeros((B, 3, H, W), f32)
        for j in range(8 * g, 8 * g + 8):
            a = (a + x[:, None, :, :, j] * wm[:, :, j, None, None]).astype(f32)
        part.append(a)
    while len(part) > 1:
        part = [(part[i] + part[i + 1]).astype(f32) for i in range(0, len(part), 2)]
    r = (part[0] + np.asarray(bias, f32)[None, :, None, None]).astype(f32)
    if yprev is not None:
        yp = np.pad(np.asarray(yprev, f32), ((0, 0), (0, 0), (1, 0), (1, 0)))       # tap (my - 1, mx - 1) with the zero border
        h2, w2 = H // 2, W // 2
        for py in range(2):
            for px in range(2):
                wy0 = f32(0.25 if py else 0.75)
                wx0 = f32(0.25 if px and not swap_odd_cols else 0.75)      # the mutant: odd columns weigh their taps as even ones do
                s = np.zeros((B, 3, h2, w2), f32)
                for dy in range(2):
                    for dx in range(2):
                        wt = f32((f32(1) - wy0 if dy else wy0) * (f32(1) - wx0 if dx else wx0))
                        s = (s + wt * yp[:, :, dy:dy + h2, dx:dx + w2]).astype(f32)
                r[:, :, py::2, px::2] = r[:, :, py::2, px::2] + s
    return r


def emu_blur(x16, pad, stride, tap=0.375, clamp_top=False):
    """blur_kernel in float32: per input row the horizontal sum of four taps (a zero tap weight outside the image), the vertical sum of four
    such rows (a zero row weight outside), one rounding to fp16."""
    x = np.asarray(x16, f32)
    B, H, W, C = x.shape
    f = np.array([0.125, tap, 0.375, 0.125], f32)
    Ho, Wo = (H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1
    out = np.zeros((B, Ho, Wo, C), f32)
    for oy in range(Ho):
        acc = np.zeros((B, Wo, C), f32)
        for jy in range(4):
            iy = oy * stride + jy - pad
            rw = f32(1.0 if 0 <= iy < H or (clamp_top and iy < 0) else 0.0)
            row = x[:, min(max(iy, 0), H - 1)]                                       # [B,W,C]
            hs = np.zeros((B, Wo, C), f32)
            for jx in range(4):
                ix = np.arange(Wo) * stride + jx - pad
                ok = (ix >= 0) & (ix < W)
                fx = np.where(ok, f[jx], f32(0)).astype(f32)[None, :, None]
                hs = (hs + fx * row[:, np.where(ok, ix, 0)]).astype(f32)
            acc = (acc + f[jy] * (rw * hs)).astype(f32)
        out[:, oy] = acc
    return R.h16(out)


def emu_fromrgb(y, w, bias, clamp=True, slope=0.2):
    """fromrgb_kernel in float32: n = clip((y + 1) * 0.5, 0, 1), v = 2 n - 1, three products + bias, lrelu * sqrt 2, one rounding to fp16."""
    y, w, bias = np.asarray(y, f32), np.asarray(w, f32), np.asarray(bias, f32)
    n = (y + f32(1)) * f32(0.5)
    if clamp:
        n = np.clip(n, f32(0), f32(1))
    v = (n * f32(2) - f32(1)).astype(f32).transpose(0, 2, 3, 1)                      # [B,R,R,3]
    t = v[..., 0, None] * w[:, 0]
    t = (t + v[..., 1, None] * w[:, 1]).astype(f32)
    t = (t + v[..., 2, None] * w[:, 2]).astype(f32)
    t = (t + bias).astype(f32)
    return R.h16(np.where(t > 0, t, f32(slope) * t).astype(f32) * f32(math.sqrt(2)))


def _fails(name, got, ref, tol):
    with pytest.raises(AssertionError, match="exceed their bound"):
        check_bound(name + " (a mutant: must FAIL)", got, ref, tol, log=False)


@pytest.mark.parametrize("C", R.TORGB_C)
@pytest.mark.parametrize("H", R.TORGB_H)
def test_torgb_bar_has_teeth(C, H):
    for with_skip in (True, False):
        a = R.torgb_inputs(C, H, with_skip)
        ref, A = R.torgb(*a)
        tol = R.tol_torgb(C, A)
        tag = "emu torgb C%d H%d skip%d" % (C, H, with_skip)
        check_bound(tag, emu_torgb(*a), ref, tol)
        _fails(tag + " smax of sample 0", emu_torgb(*a, smax_of_sample0=True), ref, tol)
        _fails(tag + " group 1 <- group 0", emu_torgb(*a, group_from_neighbour=True), ref, tol)
        if with_skip:
            _fails(tag + " .75/.25 swapped on odd columns", emu_torgb(*a, swap_odd_cols=True), ref, tol)


@pytest.mark.parametrize("pad,stride,H,C", [(2, 1, H, C) for H, C in R.BLUR_PAD2] + [(2, 1, H, C) for C in R.BLUR_PLANAR_C for H in R.BLUR_PLANAR_H]
                         + [(1, 2, H, C) for H, C in R.BLUR_DOWN])
def test_blur_bar_has_teeth(pad, stride, H, C):
    x = R.blur_inputs(H, C)
    ref, A = R.blur(x, pad, stride)
    tol = R.tol_blur(ref, A)
    tag = "emu blur pad%d H%d C%d" % (pad, H, C)
    check_bound(tag, emu_blur(x, pad, stride), ref, tol)
    _fails(tag + " tap 0.374", emu_blur(x, pad, stride, tap=0.374), ref, tol)
    _fails(tag + " top row clamped", emu_blur(x, pad, stride, clamp_top=True), ref, tol)


@pytest.mark.parametrize("Cout", R.FROMRGB_COUT)
@pytest.mark.parametrize("R_", R.FROMRGB_R)
def test_fromrgb_bar_has_teeth(Cout, R_):
    a = R.fromrgb_inputs(Cout, R_)
    assert all((a[0] == v).any() for v in (-1.0, 1.0, 1.5, -1.5, 0.0))
    ref, A = R.fromrgb(*a)
    tol = R.tol_fromrgb(ref, A)
    tag = "emu fromrgb Cout%d R%d" % (Cout, R_)
    check_bound(tag, emu_fromrgb(*a), ref, tol)
    _fails(tag + " no clamp", emu_fromrgb(*a, clamp=False), ref, tol)
    _fails(tag + " slope 0.25", emu_fromrgb(*a, slope=0.25), ref, tol)


def test_check_bound_sees_an_element_nobody_stored():
    ref = np.ones((2, 3))
    got = ref.copy(); got[1, 2] = np.nan                       # what the ops' poisoned staging returns for such an element
    with pytest.raises(AssertionError, match="non-finite"):
        check_bound("a NaN (must FAIL)", got, ref, np.full((2, 3), 1e-3), log=False)
    check_bound("an exact result", ref, ref, np.full((2, 3), 1e-12))
