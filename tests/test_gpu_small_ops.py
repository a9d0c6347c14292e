"""The small fp32 kernels around StyleGAN2 and the CLIP towers, one at a time through the diagnostic ABI (include/glass_ops.h) against the
float64 restatements of tests/small_ops_ref.py — which tests/test_small_ops_ref.py pins to the oracle on the CPU.

Inputs make an indexing bug O(1): P / B >= 2 everywhere, a candidate's values lie O(1) from its neighbours' and change sign, and whatever
lies between strided rows (and behind what a kernel writes) is NaN or a sentinel, so a read or a store outside the row shows.

Kernel instances reached (the launchers' own rules, csrc/kernels_misc.hip, kernels_clip.hip, clip_resnet.hip, stylegan2.cpp):
  mapping_fused_kernel<1> (L = 256 x 8, P = 5 / 8), mapping_fused_kernel<2> (L = 512 x 2), pixelnorm_kernel, dense_splitk_kernel (L = 64, 192,
  768 = exactly 64 KB of LDS; alone at N = 100 / 64 with row strides), dense_kernel (L = 96; ldx > K, ldo > N, eps_stride 3),
  dense_multi_kernel (4 problems, early-return workgroups, N = 8, K = 136), style_norm_kernel, gemm_tiled_kernel<64> / <128> in its `ld` / `batch`
  split-K form + dense01_finish_kernel, gemm_direct + dense_kernel (the unsplit D head), mbstd_kernel (C = 12), mbstd_vec_kernel (groups 2,
  4, 8; C = 512), finalize_image_kernel, embed_lnpre_kernel, embed_text_kernel, layernorm_kernel (register branch up to D = 1024, streaming
  branch above; row_stride 3 D; fp16 output), layernorm_rows_kernel, cosine_set_kernel at T = 1 (csrc/score.hip: the cosine and cosine_views ops),
  assemble_F_kernel (score.hip), image_patches_kernel, rn_token0_rows_kernel.

The D head's split form.  run_d_head takes it where 16 CL is a multiple of 1024 AND gemm_tiled takes the slices, and gemm_tiled refuses
fewer than 64 rows: at P = 8 and P = 5 every CL runs the unsplit form (gemm_direct + dense_kernel), as in the engine.  The cases P = 8 / 5
stay and assert that form; P = 64 and P = 70 (a partial 128-row tile) are added so that the split form and dense01_finish_kernel run.

Bars (none is taken from the device).
  * General rule: |got - ref64| <= 4 max|ref32 - ref64| on the same inputs (+ 2^-11 |ref64| where the kernel stores fp16); ref32 is the
    float32 twin of small_ops_ref.py, which adds long sums one term after the other.  Where that error is exactly zero the floor is one
    float32 ulp of max|ref64| (it is exactly zero for mbstd's features at C = 12 and at C = 32, group 2: differences of fp16 values).
  * mapping: 4 x the error of oracle.g_mapping in torch fp32 against float64, the rule of test_map_latents_matches_float64.
  * D head: the general rule, reference and twin on the fp16-rounded operands.
  * Bit-equality: embed_text (one float32 add), assemble_F, finalize_image, image_patches (numpy's float16 rounding), rn_token0_rows, style_norm's
    smax, the fp16 LayerNorm output against float16(the fp32 output), cosine_views' per-view values against the cosine op's and its mean
    against their float32 sum in the order v = 0 .. V - 1, layernorm_rows against layernorm_kernel on the gathered rows; cosine, cosine_views
    and assemble_F against what the separate kernels of the commit before csrc/score.hip returned (tests/score_tail_golden.py).
  * Position independence: a row's bits in launches of P = 5, 16, 19 at positions 0, 3, 15, 18 equal its bits in a launch of P = 1.

Measured on an MI355X (max abs error against float64 / the bar, absolute unless stated; every figure is also logged through util.diag):
  mapping           fused <1> L = 256 x 8: 2.7e-6 (P = 5), 3.2e-6 (P = 8) / 1.4e-5, 1.6e-5 (oracle fp32 3.6e-6, 4.1e-6; max|w| 6.7);
                    fused <2> L = 512 x 2: 1.1e-6 / 1.0e-5; per layer L = 64 x 3: 1.0e-6 (P = 5), 1.4e-6 (P = 19) / 5.0e-6, 8.1e-6;
                    L = 192 x 2: 1.0e-6 / 8.8e-6; L = 768 x 1: 1.6e-6 / 6.9e-6; L = 96 x 2 (dense_kernel): 1.3e-6 / 5.1e-6;
                    fused against per layer at L = 256: 2.5e-6 / 1.4e-5; path "auto" bit-equal to "fused"
  pixelnorm         1.4e-7 (L = 100), 1.9e-7 (L = 512) / 2.3e-6, 4.0e-6
  dense_splitk      (17, 64, 100): 5.3e-7 .. 9.7e-7 / 4.6e-6 .. 7.2e-6; (33, 192, 64): 7.4e-7 .. 1.0e-6 / 8.2e-6 .. 1.1e-5 (max|ref| 4 .. 6.5)
  dense strided     2.0e-6 / 8.6e-6 (max|ref| 5.6); in_sq + mode 2, eps_stride 3: 1.4e-7 / 5.4e-7 (max|ref| 0.37)
  dense_multi       2.1e-7, 3.3e-7, 3.4e-7, 2.9e-7 / 8.4e-7, 1.8e-6, 1.4e-6, 1.1e-6 (max|ref| 1.8 .. 2.7)
  style_norm        smax and the zero segment's eps_row (1e32) bit-equal; s: 6.8e-8 / 2.7e-7 (the twin's own error: the same two roundings);
                    eps_row relative: 1.0e-7 / 4.1e-7
  d_head            unsplit (P = 8, 5; CL = 64, 128, 32; P = 64 at CL = 32): 2.3e-7 .. 6.6e-7 / 2.7e-6 .. 1.2e-5; split (64, 64): 3.5e-7 / 7.2e-6;
                    (70, 128): 4.9e-7 / 1.3e-5 (max|ref| 1.1 .. 3.7; the twin adds 1024 / 2048 / 512 products one after the other)
  mbstd             features: the fp16 store, 9.8e-4 .. 1.9e-3 at max|ref| 3.6 .. 4.8, worst err / tol 0.993 .. 0.999 (the float32 twin's error
                    is 0 or 1.2e-7: fp16 inputs; the one-ulp floor applies to C = 12 and C = 32 at group 2); std: 1.3e-4 .. 4.8e-4, worst
                    err / tol 0.33 .. 0.89
  layernorm_ex      2.7e-7 .. 5.4e-7 / 1.2e-6 .. 2.0e-5 (max|ref| 3.4 .. 4.9; worst err / tol 0.34 at D = 64); fp16 output bit-equal
  layernorm_rows    3.7e-7 (D = 512), 3.9e-7 (D = 1280) / 3.6e-6, 7.8e-6; bit-equal to layernorm_kernel on the gathered rows
  embed_lnpre       3.7e-7, 7.0e-7, 4.4e-7 / 3.2e-6, 1.1e-5, 9.4e-6
  cosine            3.6e-9 (D = 512), 1.5e-8 (D = 100), 8.8e-9 (D = 640) / 5.2e-8, 1.8e-7, 1.1e-7 (|sim| <= 0.19); views: per view and mean bit-equal,
                    mean against float64 3.5e-9 .. 1.2e-8 / 4.7e-8 .. 1.3e-7
  embed_text, assemble_F, finalize_image, image_patches, rn_token0_rows: bit-exact
  position independence: 0 differing elements in all 63 launches (mapping fused <1> / <2>, per layer L = 64 / 192 / 96, dense_splitk, dense,
                    dense_multi x 7 placements)
"""
import math
import os

import numpy as np
import pytest
import torch

import small_ops_ref as R
from score_tail_golden import golden, pack
from clip_glass_amd import synth
from oracle import stylegan2_ref as sg
from util import diag

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
ops = None
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global ops
    from clip_glass_amd import ops as _ops
    ops = _ops
    yield


def h16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def _rng(seed):
    return np.random.default_rng(seed)


def _rows(rng, P, n, std=1.0):
    """[P, n] float32: N(0, std) plus a per-row offset of -1, 0, +1 (x std), so that neighbouring rows differ by O(1) and signs change."""
    return (std * (rng.standard_normal((P, n)) + (np.arange(P)[:, None] % 3 - 1.0))).astype(F32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _bit_equal(name, got, want):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    diag("[small-ops] %-44s bit-exact: %d / %d elements differ" % (name, int(bad.sum()), bad.size))
    assert not bad.any(), "%s: %d elements differ, first at %s" % (name, int(bad.sum()), np.argwhere(bad)[0])


def _bar(name, got, ref64, ref32, store16=False):
    """The general rule of the module docstring."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    e32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    floor = e32 == 0.0
    base = float(np.spacing(F32(np.abs(ref64).max()))) if floor else 4 * e32
    tol = base + (2.0 ** -11 * np.abs(ref64) if store16 else 0.0)
    err = np.abs(got - ref64)
    diag("[small-ops] %-44s max err %.3e  float32 twin's %.3e%s  bar %.3e  max|ref| %.3e  worst err / tol %.3f"
         % (name, np.nanmax(err), e32, " (zero: one-ulp floor)" if floor else "", base, np.abs(ref64).max(), np.nanmax(err / tol)))
    assert np.isfinite(got).all(), "%s: non-finite values" % name
    assert (err <= tol).all(), "%s: max err %.3e, float32 twin %.3e, %d elements beyond the bar" % (name, err.max(), e32, int((err > tol).sum()))


# ---- mapping network --------------------------------------------------------------------------------------------------------------------------
_nets = {}


def _map_net(L, layers):
    """Synthetic mapping weights: (torch state dict for the oracle, float64 folded [n, k, n] / [n, L], the float32 operands as
    finalize_generator folds them: W * (0.01f / sqrtf(L)) transposed, b * 0.01f)."""
    if (L, layers) not in _nets:
        sd = synth.make_state([s for s in synth.stylegan2_g_spec([16, 16], L, layers) if s[0].startswith("G_mapping.")], 4)
        W = [np.asarray(sd["G_mapping.main.%d.layer.weight" % i]) for i in range(layers)]
        b = [np.asarray(sd["G_mapping.main.%d.bias" % i]) for i in range(layers)]
        coef = F32(0.01) / np.sqrt(F32(L))
        _nets[(L, layers)] = ({k: torch.as_tensor(v) for k, v in sd.items()},
                              [w.astype(np.float64).T * (0.01 / math.sqrt(L)) for w in W], [x.astype(np.float64) * 0.01 for x in b],
                              np.stack([(w * coef).T for w in W]).astype(F32), np.stack([x * F32(0.01) for x in b]).astype(F32))
    return _nets[(L, layers)]


def _map_case(L, layers, P, path, kernels):
    tsd, w64, b64, w32, b32 = _map_net(L, layers)
    z = synth.latents(9 + P, P, L).astype(F32)
    ref = R.mapping(z, w64, b64)
    with torch.no_grad():
        err_o = float(np.abs(sg.g_mapping(tsd, torch.tensor(z)).numpy() - ref).max())
    got, ran = ops.mapping(z, w32, b32, path)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    diag("[small-ops] mapping L%d x%d P%d %-6s: max|ref| %.3f oracle fp32 err %.3e device err %.3e bar %.3e  ran %s"
         % (L, layers, P, path, np.abs(ref).max(), err_o, err, 4 * err_o, sorted(ran)))
    assert ran == kernels
    assert np.isfinite(got).all() and err <= 4 * err_o
    return got, ref, 4 * err_o


@pytest.mark.parametrize("L,layers,P", [(256, 8, 5), (256, 8, 8), (512, 2, 5)])
def test_mapping_fused(L, layers, P):
    got, _, _ = _map_case(L, layers, P, "fused", {"mapping_fused_kernel"})
    auto, ran = ops.mapping(synth.latents(9 + P, P, L).astype(F32), *_map_net(L, layers)[3:], "auto")
    assert ran == {"mapping_fused_kernel"}                  # what run_mapping launches at these sizes
    _bit_equal("mapping auto == fused L%d P%d" % (L, P), auto, got)


@pytest.mark.parametrize("L,layers,P,dense", [(64, 3, 5, "dense_splitk_kernel"), (64, 3, 19, "dense_splitk_kernel"), (192, 2, 5, "dense_splitk_kernel"),
                                              (768, 1, 5, "dense_splitk_kernel"), (96, 2, 5, "dense_kernel")])
def test_mapping_per_layer(L, layers, P, dense):
    """L = 768 is the largest dense_splitk admits (16 K + 4096 floats = 64 KB of dynamic LDS); L = 96 is no multiple of 64: dense_kernel.
    An odd layer count ends in the second buffer and is copied back."""
    _map_case(L, layers, P, "layers", {"pixelnorm_kernel", dense})


def test_mapping_fused_against_per_layer():
    L, layers, P = 256, 8, 5
    fused, ref, bar = _map_case(L, layers, P, "fused", {"mapping_fused_kernel"})
    per, _, _ = _map_case(L, layers, P, "layers", {"pixelnorm_kernel", "dense_splitk_kernel"})
    d = float(np.abs(fused.astype(np.float64) - per).max())
    diag("[small-ops] mapping L256 x8 P5 fused vs per-layer: max diff %.3e bar %.3e" % (d, bar))
    assert d <= bar


def test_mapping_fused_refuses_other_sizes():
    w32, b32 = _map_net(64, 3)[3:]
    with pytest.raises(RuntimeError, match="mapping_fused_kernel does not take this network"):
        ops.mapping(np.zeros((2, 64), F32), w32, b32, "fused")


@pytest.mark.parametrize("L", [100, 512])
def test_pixelnorm(L):
    z = _rows(_rng(L), 5, L, 2.0)
    z[3] *= 1e-3                                            # a small row: eps is not what normalises it
    _bar("pixelnorm L%d" % L, ops.pixelnorm(z), R.pixelnorm(z), R.pixelnorm(z, dt=F32))


# ---- dense kernels ------------------------------------------------------------------------------------------------------------------------------
def _dense_case(seed, P, K, N):
    rng = _rng(seed)
    return _rows(rng, P, K), (rng.standard_normal((K, N)) / math.sqrt(K)).astype(F32), (0.5 * rng.standard_normal(N)).astype(F32)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("P,K,N", [(17, 64, 100), (33, 192, 64)])
def test_dense_splitk(P, K, N, mode, with_bias):
    """P = 17 / 33: one row in the last 16-candidate workgroup; N = 100: the clamped weight column of the lanes past N."""
    x, wt, bias = _dense_case(P + K, P, K, N)
    b = bias if with_bias else None
    out = ops.dense_splitk(x, wt, b, mode, ldx=K + 8, ldo=N + 8)
    assert np.isnan(out[:, N:]).all(), "stored past column N"
    _bar("dense_splitk P%d K%d N%d mode%d bias%d" % (P, K, N, mode, with_bias), out[:, :N], R.dense(x, wt, b, mode=mode),
         R.dense(x, wt, b, mode=mode, dt=F32))


def test_dense_strided():
    """dense_kernel as the style path launches it: rows of a wider input table, the output into columns of a wider table."""
    P, K, N, col0, ldo = 37, 200, 150, 130, 400
    x, wt, bias = _dense_case(7, P, K, N)
    table = np.full((P, ldo), -77.0, F32)
    out = ops.dense_ex(x, wt, bias, ldx=K + 24, out=table, col0=col0)
    keep = np.ones(ldo, bool)
    keep[col0:col0 + N] = False
    assert (out[:, keep] == -77.0).all(), "stored outside its columns"
    _bar("dense strided P37 K200 N150", out[:, col0:col0 + N], R.dense(x, wt, bias), R.dense(x, wt, bias, dt=F32))
    eps = np.full((P, 3), np.nan, F32)                      # eps_stride 3: column 0 is read
    eps[:, 0] = _rng(8).uniform(0.01, 2.0, P)
    wsq = np.abs(wt)
    out = ops.dense_ex(x, wsq, None, in_sq=True, mode=2, eps_row=eps, ldx=K + 24, out=table, col0=col0)
    assert (out[:, keep] == -77.0).all(), "stored outside its columns"
    _bar("dense strided in_sq mode2 eps_stride3", out[:, col0:col0 + N], R.dense(x, wsq, in_sq=True, mode=2, eps_row=eps[:, 0]),
         R.dense(x, wsq, in_sq=True, mode=2, eps_row=eps[:, 0], dt=F32))


MULTI = [(16, 16), (32, 96), (64, 200), (136, 8)]          # (K, N): max_N = 200 (early-return workgroups), N = 8 < 64, K = 136 = 8 x 16 + 8
MULTI_EPS = [2, 0, 3, 1]                                    # eps_row index per problem, stride n_style = 5


def _multi_case(seed, P):
    rng = _rng(seed)
    ldx, ldo = sum(k for k, _ in MULTI) + 8, sum(n for _, n in MULTI) + 8
    x = np.full((P, ldx), np.nan, F32)
    x[:, :ldx - 8] = np.clip(_rows(rng, P, ldx - 8, 0.4), -1, 1)       # normalised styles lie in [-1, 1]
    eps_rows = rng.uniform(1e-3, 0.5, (P, 5)).astype(F32)
    problems, xo, oo = [], 0, 0
    for (K, N), ei in zip(MULTI, MULTI_EPS):
        problems.append((xo, (rng.uniform(0.0, 2.0, (K, N)) / K).astype(F32), oo, ei))
        xo, oo = xo + K, oo + N
    return x, problems, eps_rows, ldo


def _multi_ref(x, problems, eps_rows, dt):
    return [R.dense(x[:, xo:xo + w.shape[0]], w, in_sq=True, mode=2, eps_row=eps_rows[:, ei], dt=dt) for xo, w, oo, ei in problems]


def test_dense_multi():
    P = 18
    x, problems, eps_rows, ldo = _multi_case(21, P)
    out = ops.dense_multi(x, problems, eps_rows, ldo)
    assert np.isnan(out[:, ldo - 8:]).all(), "stored past the last problem's columns"
    r64, r32 = _multi_ref(x, problems, eps_rows, np.float64), _multi_ref(x, problems, eps_rows, F32)
    for i, (xo, w, oo, ei) in enumerate(problems):
        _bar("dense_multi problem %d K%d N%d" % (i, *w.shape), out[:, oo:oo + w.shape[1]], r64[i], r32[i])


def test_style_norm():
    P, segs, ld = 3, [(0, 16), (20, 64), (88, 100), (192, 512)], 712
    rng = _rng(31)
    s = np.full((P, ld), np.nan, F32)
    for o, n in segs:
        s[:, o:o + n] = _rows(rng, P, n, 3.0) * F32(10.0) ** rng.integers(-2, 3, (P, 1))
    s[1, 20:84] = 0.0                                       # an all-zero segment
    s[0, 88:188] = rng.uniform(-0.5, 0.5, 100)
    s[0, 187] = -3.0                                        # the maximum is negative and sits in the last element
    got, smax, eps_row = ops.style_norm(s, segs)
    r64 = R.style_norm(np.nan_to_num(s), segs)
    r32 = R.style_norm(np.nan_to_num(s), segs, dt=F32)
    gap = np.isnan(s)
    assert np.isnan(got[gap]).all(), "stored between the segments"
    _bit_equal("style_norm smax", smax, r32[1])
    assert smax[1, 1] == F32(1e-20) and smax[0, 2] == F32(3.0)
    assert (got[1, 20:84] == 0.0).all()
    _bit_equal("style_norm eps_row of the zero segment", eps_row[1, 1], r32[2][1, 1])      # 1e-8f * 1e20f * 1e20f: finite in float32
    assert np.isfinite(eps_row[1, 1])
    _bar("style_norm s", got[~gap], r64[0][~gap], r32[0][~gap])
    _bar("style_norm eps_row / max", eps_row / r64[2], np.ones_like(r64[2]), r32[2].astype(np.float64) / r64[2])      # relative: the rows span 1e-12 .. 1e32


# ---- D head -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,CL", [(8, 64), (5, 64), (8, 128), (5, 128), (8, 32), (5, 32), (64, 64), (70, 128), (64, 32)])
def test_d_head(P, CL):
    rng = _rng(P * CL)
    dfin = h16(_rows(rng, P, 16 * CL))
    w0 = h16(rng.standard_normal((CL, 16 * CL)) / math.sqrt(16 * CL))
    b0, w1, b1 = (0.3 * rng.standard_normal(CL)).astype(F32), (rng.standard_normal(CL) / math.sqrt(CL)).astype(F32), np.array([0.25], F32)
    dis, form = ops.d_head(dfin, w0, b0, w1, b1)
    # run_d_head's rule: 16 slices of a multiple of 64, on gemm_tiled, which takes no fewer than 64 rows
    assert form == ("split" if (16 * CL) % 1024 == 0 and P >= 64 else "whole")
    _bar("d_head P%d CL%d %s" % (P, CL, form), dis, R.d_head(dfin, w0, b0, w1, b1), R.d_head(dfin, w0, b0, w1, b1, dt=F32))


# ---- mbstd ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,Cpad,batch_size,group", [(8, 12, 16, 4, 4), (8, 12, 16, 4, 2), (8, 32, 48, 8, 2), (16, 32, 48, 8, 8),
                                                       (8, 512, 528, 8, 4)])
def test_mbstd(B, C, Cpad, batch_size, group):
    """C = 12: mbstd_kernel (C no multiple of 8); the others mbstd_vec_kernel; C = 512, hw = 16, batch 8: the real head's shape."""
    x = h16(_rows(_rng(C + group), B, 16 * C).reshape(B, 16, C))
    got = ops.mbstd(x, Cpad, batch_size, group)
    d64, s64 = R.mbstd(x, batch_size, group)
    d32, s32 = R.mbstd(x, batch_size, group, dt=F32)
    name = "mbstd B%d C%d bs%d g%d" % (B, C, batch_size, group)
    _bar(name + " features", got[..., :C], d64, d32, store16=True)
    _bar(name + " std", got[..., C], np.broadcast_to(s64[:, None], (B, 16)), np.broadcast_to(s32[:, None], (B, 16)), store16=True)
    assert (got[..., C + 1:] == 0).all()


# ---- CLIP glue --------------------------------------------------------------------------------------------------------------------------------
def _ln_case(seed, M, D):
    rng = _rng(seed)
    return _rows(rng, M, D, 2.0), (1 + 0.1 * rng.standard_normal(D)).astype(F32), (0.1 * rng.standard_normal(D)).astype(F32)


@pytest.mark.parametrize("M", [5, 9])
@pytest.mark.parametrize("D", [64, 100, 1024, 1088, 1280, 1600])
def test_layernorm_ex(M, D):
    """D <= 1024: the register branch (1024 fills it); above: the streaming branch.  row_stride = 3 D: the GPT-2 last-row form."""
    x, g, b = _ln_case(D + M, M, D)
    got = ops.layernorm_ex(x, g, b, row_stride=3 * D)
    _bar("layernorm_ex M%d D%d" % (M, D), got, R.layernorm(x, g, b), R.layernorm(x, g, b, dt=F32))
    got16 = ops.layernorm_ex(x, g, b, row_stride=3 * D, half_out=True)
    _bit_equal("layernorm_ex M%d D%d fp16 output" % (M, D), got16, h16(got))


@pytest.mark.parametrize("D", [512, 1280])
def test_layernorm_rows(D):
    x, g, b = _ln_case(D, 7, D)
    rows = [6, 6, 3, 2, 0]                                  # repeated and descending
    got = ops.layernorm_rows(x, rows, g, b)
    _bar("layernorm_rows D%d" % D, got, R.layernorm(x[rows], g, b), R.layernorm(x[rows], g, b, dt=F32))
    _bit_equal("layernorm_rows D%d == layernorm_kernel on the gathered rows" % D, got, ops.layernorm_ex(x[rows], g, b))


@pytest.mark.parametrize("P,T,D", [(3, 5, 128), (2, 50, 768), (2, 3, 1280)])
def test_embed_lnpre(P, T, D):
    rng = _rng(T * D)
    pe = _rows(rng, P * (T - 1), D).reshape(P, T - 1, D)
    cls, pos = rng.standard_normal(D).astype(F32), rng.standard_normal((T, D)).astype(F32)
    g, b = (1 + 0.1 * rng.standard_normal(D)).astype(F32), (0.1 * rng.standard_normal(D)).astype(F32)
    _bar("embed_lnpre P%d T%d D%d" % (P, T, D), ops.embed_lnpre(pe, cls, pos, g, b), R.embed_lnpre(pe, cls, pos, g, b),
         R.embed_lnpre(pe, cls, pos, g, b, dt=F32))


def test_embed_text():
    n, ctx, D, V = 3, 7, 100, 50
    rng = _rng(41)
    tok_emb, pos = rng.standard_normal((V, D)).astype(F32), rng.standard_normal((ctx, D)).astype(F32)
    tokens = rng.integers(1, V - 1, (n, ctx))
    tokens[0, 0], tokens[1, 6], tokens[2, 3], tokens[0, 5] = 0, V - 1, 0, V - 1
    _bit_equal("embed_text", ops.embed_text(tokens, tok_emb, pos), R.embed_text(tokens, tok_emb, pos, dt=F32))


COSINE_D, COSINE_VIEWS_V, ASSEMBLE_F_P = [512, 100, 640], [1, 3, 16], [1, 64, 65, 130]


def _cosine_case(D):
    rng = _rng(D)
    feat, target = _rows(rng, 5, D), rng.standard_normal(D).astype(F32)
    feat[3] = 0.0                                           # an all-zero feature row
    return feat, target


def _cosine_views_case(V):
    P, D = 5, 100
    rng = _rng(50 + V)
    return _rows(rng, P * V, D).reshape(P, V, D), rng.standard_normal(D).astype(F32)


def _assemble_F_case(P, n_obj):
    rng = _rng(P)
    sim = rng.uniform(-1, 1, P).astype(F32)
    dis = (1.0 + 2.0 * rng.standard_normal(P)).astype(F32)  # both sides of 1
    dis[0] = 1.0
    if P > 2:
        dis[1], dis[2] = 3.5, -2.0
    return sim, dis if n_obj == 2 else None


@pytest.mark.parametrize("D", COSINE_D)
def test_cosine(D):
    feat, target = _cosine_case(D)
    got = ops.cosine(feat, target)
    assert got[3] == 0.0
    _bit_equal("cosine D%d == the parent's cosine_kernel" % D, got, golden("cosine_D%d" % D))
    _bar("cosine D%d" % D, got, R.cosine(feat, target), R.cosine(feat, target, dt=F32))


@pytest.mark.parametrize("V", COSINE_VIEWS_V)
def test_cosine_views(V):
    feat, target = _cosine_views_case(V)
    P, _, D = feat.shape
    vs, sim = ops.cosine_views(feat, target)
    _bit_equal("cosine_views V%d == the parent's cosine_views_kernel" % V, pack(vs, sim), golden("cosine_views_V%d" % V))
    _bit_equal("cosine_views V%d per view == cosine_kernel" % V, vs, ops.cosine(feat.reshape(P * V, D), target).reshape(P, V))
    acc = np.zeros(P, F32)
    for v in range(V):
        acc = acc + vs[:, v]
    _bit_equal("cosine_views V%d mean in the order v = 0 .. V - 1" % V, sim, acc / F32(V))
    r64, r32 = R.cosine_views(feat, target), R.cosine_views(feat, target, dt=F32)
    _bar("cosine_views V%d mean" % V, sim, r64[1], r32[1])


@pytest.mark.parametrize("n_obj", [1, 2])
@pytest.mark.parametrize("P", ASSEMBLE_F_P)
def test_assemble_F(P, n_obj):
    sim, d = _assemble_F_case(P, n_obj)
    got = ops.assemble_F(sim, d)
    _bit_equal("assemble_F P%d n_obj%d" % (P, n_obj), got, R.assemble_F(sim, d, dt=F32))
    _bit_equal("assemble_F P%d n_obj%d == the parent's" % (P, n_obj), pack(got), golden("assemble_F_P%d_n%d" % (P, n_obj)))


@pytest.mark.parametrize("n", [1, 255, 257, 3 * 32 * 32])
def test_finalize_image(n):
    y = (1.2 * _rng(n).standard_normal(n)).astype(F32)
    special = np.array([-1.0, 1.0, -1.5, 1.5, -1.0 - 2.0 ** -23, 1.0 + 2.0 ** -23, 0.0, -0.0], F32)
    k = min(n, special.size)
    y[n - k:] = special[:k]
    _bit_equal("finalize_image n%d" % n, ops.finalize_image(y), R.finalize_image(y, dt=F32))


@pytest.mark.parametrize("S,ps,ld", [(32, 8, 192), (28, 14, 608), (64, 32, 3072)])
def test_image_patches(S, ps, ld):
    n, K = 2, 3 * ps * ps
    img = (_rng(S).standard_normal((n, 3, S, S)) + (np.arange(n)[:, None, None, None] - 0.5)).astype(F32)
    img[0, 0, 0, :4] = [70000.0, 2.0 ** -25, 1 + 2.0 ** -11, -65520.0]      # overflow, underflow, halfway cases
    got = ops.image_patches(img, ps, ld, sentinel=-7.0)
    with np.errstate(over="ignore"):
        want = R.image_patches(img, ps).astype(np.float16)
    assert got.shape == (n * (S // ps) ** 2, ld)
    np.testing.assert_array_equal(got[:, :K].astype(np.float16).view(np.uint16), want.view(np.uint16))
    assert (got[:, K:] == -7.0).all(), "columns past 3 ps^2 were written"


def test_rn_token0_rows():
    B, T, C = 3, 5, 300
    att = h16(_rows(_rng(61), B * T, C).reshape(B, T, C))
    _bit_equal("rn_token0_rows", ops.rn_token0_rows(att), att[:, 0, :])


# ---- position independence ----------------------------------------------------------------------------------------------------------------------
PLACES = [(5, 0), (5, 3), (16, 3), (16, 15), (19, 0), (19, 15), (19, 18)]


def _position_independent(name, run, row, others):
    """run(rows [P, n]) -> [P, m].  The bits of `row`'s result in a launch of P = 1 against launches of P candidates with it at position pos;
    others(P) makes the rows around it (different data)."""
    base = run(row[None])[0]
    assert np.isfinite(base).all()
    for P, pos in PLACES:
        x = others(P)
        assert not (x == row).all(axis=1).any()
        x[pos] = row
        got = run(x)[pos]
        bad = _bits(got) != _bits(base)
        diag("[small-ops] %-44s P%d pos%d: %d / %d elements differ from the P = 1 launch" % (name, P, pos, int(bad.sum()), bad.size))
        assert not bad.any(), "%s: P %d position %d: %d elements differ (max %.3e)" % (name, P, pos, int(bad.sum()), np.abs(got - base).max())


@pytest.mark.parametrize("L,layers,path", [(256, 8, "fused"), (512, 2, "fused"), (64, 3, "layers"), (192, 2, "layers"), (96, 2, "layers")])
def test_mapping_position_independent(L, layers, path):
    w32, b32 = _map_net(L, layers)[3:]
    _position_independent("mapping L%d %s" % (L, path), lambda z: ops.mapping(z, w32, b32, path)[0], synth.latents(70, 1, L).astype(F32)[0],
                          lambda P: synth.latents(71 + P, P, L).astype(F32))


def test_dense_splitk_position_independent():
    K, N = 192, 100
    x, wt, bias = _dense_case(80, 1, K, N)
    _position_independent("dense_splitk K192 N100", lambda v: ops.dense_splitk(v, wt, bias, 1, ldx=K + 8, ldo=N + 8)[:, :N], x[0],
                          lambda P: _rows(_rng(81 + P), P, K))


def test_dense_position_independent():
    K, N = 200, 150
    x, wt, bias = _dense_case(90, 1, K, N)
    _position_independent("dense K200 N150", lambda v: ops.dense_ex(v, wt, bias, mode=1, ldx=K + 24), x[0], lambda P: _rows(_rng(91 + P), P, K))


def test_dense_multi_position_independent():
    x1, problems, eps1, ldo = _multi_case(100, 1)

    def run(rows):                                          # rows [P, ldx + 5]: the style row and its eps_row entries travel together
        return ops.dense_multi(rows[:, :-5], problems, rows[:, -5:], ldo)[:, :ldo - 8]

    def others(P):
        x, _, eps, _ = _multi_case(101 + P, P)
        return np.nan_to_num(np.concatenate([x, eps], axis=1), nan=0.5)

    _position_independent("dense_multi", run, np.nan_to_num(np.concatenate([x1, eps1], axis=1), nan=0.5)[0], others)
