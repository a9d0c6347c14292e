"""Per-kernel parity of the GPT-2 trunk (csrc/gpt2.hip) through the diagnostic ops glass_op_gpt2_* (include/glass_ops.h), which launch
each kernel as the passes of gpt2_host.cpp launch it.  References: float64 numpy of the same operation (tests/gpt2_ops_ref.py, pinned to the
oracle by tests/test_gpt2_ops_ref.py).

Two kinds of input:
  exact   integers in [-3, 3]: every partial sum is an integer below 2^24, so an fp32 sum in ANY order is exact and modes 0 / 2 must
          equal the integer result (np.array_equal, no tolerance).
  real    standard normal, W scaled by K^-0.5.  Modes 0 / 2: the worst-case bound of fp32 summation in any order, per element,
          |got - ref64| <= (K + 3) 2^-24 (|A| @ |W|^T + |bias| + |res|).  GELU, LayerNorm-fused operands, statistics, attention and the
          head's logits: the same operation in float32 on the CPU (torch) has a worst error E32 against float64, normalised by the
          element's scale; the bar is 8 E32 (two correct fp32 implementations differ through summation order and a few ulp of libm; a
          masking or indexing error is of order 1/K .. 1/ns of the scale).
Every case writes a `[check]` line (E32, bar, observed) to the suite's diag.log (util.diag).

Figures of the first GPU run (MI355X; scaled errors, worst case of each family):
  exact inputs            65 products + 4 sets of rowblk partial means = 69 EQUAL lines (step S = 1 .. 16, rowblk, prefill, decode; M 1 .. 1472, N 32 .. 50257, K 64 .. 4096): all EQUAL
  real, modes 0 / 2       worst err / bound: step 0.004, rowblk 0.001, prefill 0.006, decode 0.001 (the bound is a worst case)
  GELU products           E32 4.3e-8 .. 2.7e-7; observed at most 1.37 x E32 (step M1 N768 K192)
  LayerNorm-fused (step)  E32 6.3e-8 .. 2.4e-7; at most 1.03 x E32; rowblk chain (partials + fused GELU product) at most 0.82 x E32
  statistics {mean, rstd} E32 6.9e-8 .. 1.5e-7; at most 1.03 x E32 (the 17 cases of 31 rows or more; single rows came later, see _check_stats)
  attention               E32 up to 2.2e-7 of max|v|; step kernel at most 1.18 x E32, general 1.20 x, device-past 1.09 x; the saturated
                          case is exact (E32 = observed = 0)
  head logits             E32 7.3e-8 .. 3.0e-7; at most 4.35 x E32 (M64 V4096 K1024: one fmaf chain over 1024 terms against a blocked sum)
  step vs general kernel  bitwise equal at past = 0 only (asserted there); past 16 / 47 / 63 differ by 2.5e-8 .. 3.5e-8 of max|v|, at most
                          0.84 x E32 (asserted within 8 E32)"""
import numpy as np
import pytest
import torch

import gpt2_ops_ref as R
from util import diag

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MARGIN = 8.0


def _ops():
    from clip_glass_amd import ops
    return ops


def _ints(rs, *shape):
    return rs.randint(-3, 4, size=shape).astype(np.float32)


def _t32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32))


def _check_exact(name, got, ref):
    ok = np.array_equal(np.asarray(got, dtype=np.float64), ref)
    bad = int((np.asarray(got, dtype=np.float64) != ref).sum())
    diag("[check] %-44s exact inputs: %s (%d/%d elements differ)" % (name, "EQUAL" if ok else "DIFFERENT", bad, ref.size))
    assert ok, "%s: %d/%d elements differ from the integer result" % (name, bad, ref.size)


def _check_bound(name, got, ref, bound):
    """Element-wise derived bound (no measured quantity)."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    nbad = int((~(err <= bound)).sum())
    diag("[check] %-44s derived bound: worst err/bound %.3f, max err %.3e, bad %d/%d %s"
         % (name, ratio, float(np.nanmax(err)) if err.size else 0.0, nbad, err.size, "OK" if nbad == 0 else "FAIL"))
    assert nbad == 0, "%s: %d/%d elements exceed the fp32 summation bound (worst err/bound %.3f)" % (name, nbad, err.size, ratio)


def _check_e32(name, got, ref64, ref32, scale, floor=0.0):
    """bar = 8 x the worst scaled error of the float32 CPU computation; scale: array broadcastable to ref64, or a scalar.  floor: the
    least E32 taken (see _check_stats).  Returns E32."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref64.shape, "%s: shape %s vs %s" % (name, got.shape, ref64.shape)
    scale = np.maximum(np.broadcast_to(np.asarray(scale, dtype=np.float64), ref64.shape), 1e-300)
    e32 = max(float((np.abs(np.asarray(ref32, dtype=np.float64) - ref64) / scale).max()), floor)
    bar = MARGIN * e32
    finite = bool(np.isfinite(got).all())
    obs = float(np.nanmax(np.abs(got - ref64) / scale)) if finite else float("inf")
    diag("[check] %-44s E32 %.3e bar %.3e observed %.3e (%.2f x E32) %s" % (name, e32, bar, obs, obs / max(e32, 1e-300),
                                                                        "OK" if finite and obs <= bar else "FAIL"))
    assert finite, "%s: non-finite values" % name
    assert obs <= bar, "%s: observed scaled error %.3e above the bar %.3e = 8 x E32 %.3e" % (name, obs, bar, e32)
    return e32


def _stats32(x):
    x = _t32(x)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return torch.stack([mean, torch.rsqrt(var + 1e-5)], dim=-1).numpy()


def _check_stats(name, got, x):
    """{mean, rstd} rows: the mean against the row's mean magnitude, rstd relative to itself.  E32 is a maximum over the case's
    elements; a single row has two, and the CPU's float32 may round both correctly (E32 = 0, a bar no fp32 kernel can meet).  E32 is
    therefore taken as at least 2^-24, the rounding of ONE float32 operation — below every E32 measured on 31 rows or more (6.9e-8 ..
    1.5e-7), so it only acts where the measurement has too few elements to mean anything."""
    ref = R.ln_stats(x)
    scale = np.stack([np.abs(R.f64(x)).mean(-1), ref[:, 1]], axis=-1)
    _check_e32(name, got, ref, _stats32(x), scale, floor=U)


def _ln32(x, g, b):
    x = _t32(x)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + 1e-5) * _t32(g) + _t32(b)


def _gelu32(v):
    return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v * v * v)))


def _gemm32(a, w, bias, mode, ln=None):
    a = _ln32(a, ln[0], ln[1]) if ln is not None else _t32(a)
    v = a @ _t32(w).T
    if bias is not None:
        v = v + _t32(bias)
    return (_gelu32(v) if mode == 1 else v).numpy()


# ---- products -------------------------------------------------------------------------------------------------------------------------
_BIG = {}


def _wte_ints():
    if "w" not in _BIG:
        _BIG["w"] = _ints(np.random.RandomState(77), 50257, 768)
    return _BIG["w"]


def _gemm_exact(form, M, N, K, mode, pad=0, want_pst=False):
    ops = _ops()
    rs = np.random.RandomState(1000 * M + N + K + mode)
    abuf = _ints(rs, M, K + pad)
    a = abuf[:, :K]
    w = _wte_ints() if (N, K) == (50257, 768) else _ints(rs, N, K)
    bias = _ints(rs, N)
    res = _ints(rs, M, N) if mode == 2 else None
    r = ops.gpt2_gemm(a, w, bias, mode=mode, form=form, res=res, want_pst=want_pst, width=min(N, K) if N != 50257 else 768)
    ref = R.gemm(a, w, bias, mode=mode, res=res)
    name = "gemm exact %s M%d N%d K%d%s mode%d S%d" % (form, M, N, K, "+%d" % pad if pad else "", mode, r["S"])
    _check_exact(name, r["out"], ref)
    return r, ref


# (M, N, K, lda - K): a covering set of M in {1, 31, 32, 33, 63, 64} x N in {32, 33, 768, 2304, 4096, 50257} x K in {64, 192, 768, 1024, 3072}
STEP_SHAPES = [(1, 32, 64, 0), (31, 33, 192, 0), (32, 768, 768, 0), (33, 2304, 768, 0), (63, 4096, 1024, 0), (64, 768, 3072, 0),
               (33, 50257, 768, 0), (64, 33, 1024, 0), (63, 32, 3072, 0), (31, 2304, 1024, 8), (32, 4096, 768, 0), (1, 768, 192, 0),
               (64, 4096, 64, 0), (33, 33, 3072, 4)]


@pytest.mark.parametrize("M,N,K,pad", STEP_SHAPES)
def test_step_gemm_exact(M, N, K, pad):
    """launch_gemm_f32_step + launch_gpt2_reduce (mode 0) / launch_gpt2_finalize (mode 2, N <= 1024) on integer operands."""
    _gemm_exact("step", M, N, K, 0, pad)
    if N <= 1024:
        r, ref = _gemm_exact("step", M, N, K, 2, pad)
        _check_stats("gemm step M%d N%d K%d finalize stats" % (M, N, K), r["stats"], r["out"])


def test_step_gemm_reaches_every_split():
    """The split S launch_gemm_f32_step chooses (returned by the op): S = 1, 2, 3, 4 and a value above 4 are each exercised, exactly.
    The launcher weighs its grids against glass_cu_count(): the shapes below are chosen for the 256 CUs of an MI355X in its default
    partition mode; on another CU count the same shapes may land on other splits and this list needs re-deriving (gpt2.hip,
    launch_gemm_f32_step: the factorisation with the most workgroups that fit the chip in one round)."""
    seen = {}
    for N, K in [(32, 64), (4096, 768), (2304, 768), (4096, 1024), (768, 768), (768, 3072), (1024, 4096)]:
        r, _ = _gemm_exact("step", 33, N, K, 0)
        seen.setdefault(r["S"], []).append((N, K))
    diag("[gpt2 ops] launch_gemm_f32_step splits reached: %r" % seen)
    assert {1, 2, 3, 4} <= set(seen) and max(seen) > 4, "splits reached: %r" % seen


@pytest.mark.parametrize("M,N,K,pad,mode,pst", [(33, 768, 768, 0, 2, True), (63, 2304, 768, 0, 0, False), (64, 4096, 768, 0, 0, False),
                                                (31, 768, 3072, 0, 2, True), (1, 32, 768, 0, 0, True), (32, 768, 768, 4, 2, True),
                                                (64, 768, 3072, 0, 0, False), (33, 4096, 3072, 0, 0, False)])
def test_rowblk_gemm_exact(M, N, K, pad, mode, pst):
    """launch_gemm_f32_rowblk on integer operands; the epilogue's row partials: the means of integers over 32 columns are exact, the
    M2s are sums of 32 squares (bound (32 + 3) 2^-24 relative)."""
    r, ref = _gemm_exact("rowblk", M, N, K, mode, pad, want_pst=pst)
    if pst:
        blk = ref.reshape(M, N // 32, 32)
        mean = blk.mean(-1)
        m2 = ((blk - mean[..., None]) ** 2).sum(-1)
        _check_exact("rowblk M%d N%d K%d partial means" % (M, N, K), r["pst"][..., 0], mean)
        _check_bound("rowblk M%d N%d K%d partial M2" % (M, N, K), r["pst"][..., 1], m2, 35 * U * m2)


@pytest.mark.parametrize("form,M,N,K,pad", [("prefill", 65, 768, 768, 0), ("prefill", 100, 33, 192, 4), ("prefill", 1472, 2304, 768, 0),
                                            ("prefill", 33, 32, 64, 0), ("prefill", 64, 4096, 1024, 0),
                                            ("decode", 65, 33, 64, 0), ("decode", 100, 768, 1024, 0), ("decode", 1472, 768, 3072, 0),
                                            ("decode", 33, 768, 768, 0), ("decode", 64, 32, 3072, 0), ("decode", 1, 33, 192, 0),
                                            ("decode", 63, 50257, 768, 0), ("decode", 31, 2304, 768, 8), ("decode", 32, 4096, 1024, 0)])
def test_launch_gemm_f32_exact(form, M, N, K, pad):
    """launch_gemm_f32 with prefill = true (tiled kernel) / false (streaming kernel + its own split-K reduce for M <= 64, tiled above)."""
    _gemm_exact(form, M, N, K, 0, pad)
    _gemm_exact(form, M, N, K, 2, pad)


def _real(rs, M, N, K):
    a = rs.standard_normal((M, K)).astype(np.float32)
    w = (rs.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    return a, w, bias


@pytest.mark.parametrize("form,M,N,K", [("step", 33, 2304, 768), ("step", 63, 768, 3072), ("step", 1, 33, 192), ("step", 64, 4096, 1024),
                                        ("rowblk", 33, 768, 768), ("rowblk", 63, 768, 3072), ("prefill", 100, 768, 768),
                                        ("decode", 33, 4096, 1024), ("decode", 64, 33, 3072)])
def test_gemm_real_summation_bound(form, M, N, K):
    ops = _ops()
    rs = np.random.RandomState(M + N + K)
    a, w, bias = _real(rs, M, N, K)
    res = rs.standard_normal((M, N)).astype(np.float32)
    for mode in (0, 2):
        if mode == 2 and form == "step" and N > 1024:
            continue
        r = ops.gpt2_gemm(a, w, bias, mode=mode, form=form, res=res if mode == 2 else None)
        ref = R.gemm(a, w, bias, mode=mode, res=res if mode == 2 else None)
        _check_bound("gemm real %s M%d N%d K%d mode%d S%d" % (form, M, N, K, mode, r["S"]), r["out"], ref,
                     (K + 3) * U * R.gemm_scale(a, w, bias, res if mode == 2 else None))


@pytest.mark.parametrize("form,M,N,K", [("step", 33, 3072, 768), ("step", 64, 4096, 1024), ("step", 1, 768, 192), ("rowblk", 63, 3072, 768),
                                        ("prefill", 65, 768, 192), ("decode", 33, 3072, 768)])
def test_gemm_real_gelu(form, M, N, K):
    ops = _ops()
    a, w, bias = _real(np.random.RandomState(7 + M + N + K), M, N, K)
    r = ops.gpt2_gemm(a, w, bias, mode=1, form=form)
    _check_e32("gemm gelu %s M%d N%d K%d S%d" % (form, M, N, K, r["S"]), r["out"], R.gemm(a, w, bias, mode=1), _gemm32(a, w, bias, 1),
               R.gemm_scale(a, w, bias))


def _ln_inputs(rs, M, K):
    x = (rs.standard_normal((M, K)) * (0.5 + rs.rand(M, 1) * 3.0) + rs.standard_normal((M, 1))).astype(np.float32)
    g = (1.0 + 0.1 * rs.standard_normal(K)).astype(np.float32)
    b = (0.1 * rs.standard_normal(K)).astype(np.float32)
    return x, g, b


@pytest.mark.parametrize("M,N,K,mode", [(33, 2304, 768, 0), (64, 4096, 1024, 1), (1, 576, 192, 0), (63, 256, 64, 1), (31, 768, 192, 1)])
def test_step_gemm_layernorm_fused(M, N, K, mode):
    """LayerNorm on the operand from gpt2_finalize_kernel's own statistics (returned and checked too)."""
    ops = _ops()
    rs = np.random.RandomState(11 + M + N + K)
    x, g, b = _ln_inputs(rs, M, K)
    _, w, bias = _real(rs, M, N, K)
    r = ops.gpt2_gemm(x, w, bias, mode=mode, form="step", ln=(g, b))
    name = "gemm LN-fused step M%d N%d K%d mode%d S%d" % (M, N, K, mode, r["S"])
    _check_stats(name + " stats", r["stats"], x)
    _check_e32(name, r["out"], R.gemm(x, w, bias, mode=mode, ln=(g, b)), _gemm32(x, w, bias, mode, ln=(g, b)),
               R.gemm_scale(R.layernorm(x, g, b), w, bias))


@pytest.mark.parametrize("M", [1, 33, 64])
def test_rowblk_chain_layernorm_from_row_partials(M):
    """The engine's rowblk pair at D = 768: x' = x + att @ Wo^T + b with the (mean, M2) partials in the epilogue, then
    hid = gelu(LN2(x') @ Wfc^T + b) consuming them.  The partials are the device's own; the reference normalises the device's x'."""
    ops = _ops()
    D = 768
    rs = np.random.RandomState(21 + M)
    att, wo, bo = _real(rs, M, D, D)
    x, g, b = _ln_inputs(rs, M, D)
    r1 = ops.gpt2_gemm(att, wo, bo, mode=2, form="rowblk", res=x, want_pst=True)
    _check_bound("rowblk chain M%d residual product" % M, r1["out"], R.gemm(att, wo, bo, mode=2, res=x), (D + 3) * U * R.gemm_scale(att, wo, bo, x))
    x1 = r1["out"]
    blk = R.f64(x1).reshape(M, D // 32, 32)
    pm = blk.mean(-1)
    p32 = _t32(x1).reshape(M, D // 32, 32)
    pm32 = p32.mean(-1)
    pq32 = ((p32 - pm32[..., None]) ** 2).sum(-1)
    pq = ((blk - pm[..., None]) ** 2).sum(-1)
    _check_e32("rowblk chain M%d partials" % M, r1["pst"], np.stack([pm, pq], -1), np.stack([pm32.numpy(), pq32.numpy()], -1),
               np.stack([np.abs(blk).mean(-1), pq], -1))
    _, wfc, bfc = _real(rs, M, 4 * D, D)
    r2 = ops.gpt2_gemm(x1, wfc, bfc, mode=1, form="rowblk", ln=(g, b), pst_in=r1["pst"])
    _check_e32("rowblk chain M%d LN-fused gelu product" % M, r2["out"], R.gemm(x1, wfc, bfc, mode=1, ln=(g, b)),
               _gemm32(x1, wfc, bfc, 1, ln=(g, b)), R.gemm_scale(R.layernorm(x1, g, b), wfc, bfc))


def test_gemm_ops_refuse_unsupported_shapes_by_name():
    ops = _ops()
    a, w = np.zeros((65, 64), np.float32), np.zeros((32, 64), np.float32)
    with pytest.raises(RuntimeError, match="launch_gemm_f32_step does not take this shape"):
        ops.gpt2_gemm(a, w, form="step")
    with pytest.raises(RuntimeError, match="launch_gemm_f32_rowblk does not take this shape"):
        ops.gpt2_gemm(a[:33], w, form="rowblk")
    with pytest.raises(RuntimeError, match="N <= 1024"):
        ops.gpt2_gemm(a[:33], np.zeros((2048, 64), np.float32), mode=2, res=np.zeros((33, 2048), np.float32), form="step")


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _att32(qkv, kc, vc, past, heads):
    P, _, D = kc.shape
    qkv = _t32(qkv).reshape(P, -1, 3 * D)
    nd = qkv.shape[1]
    ns = past + nd
    k = torch.cat([_t32(kc[:, :past]), qkv[:, :, D:2 * D]], dim=1).reshape(P, ns, heads, 64).permute(0, 2, 1, 3)
    v = torch.cat([_t32(vc[:, :past]), qkv[:, :, 2 * D:]], dim=1).reshape(P, ns, heads, 64).permute(0, 2, 1, 3)
    q = qkv[:, :, :D].reshape(P, nd, heads, 64).permute(0, 2, 1, 3)
    s = (q @ k.transpose(-1, -2)) * 0.125
    masked = torch.arange(ns)[None, :] > past + torch.arange(nd)[:, None]
    s = torch.where(masked, torch.full_like(s, -1e10), s)
    return (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(P * nd, D).numpy()


def _caches(rs, P, Tmax, D, past):
    """History rows standard normal, every row from `past` on NaN (the call writes past .. past + nd - 1 and must not use the rest)."""
    kc = rs.standard_normal((P, Tmax, D)).astype(np.float32)
    vc = rs.standard_normal((P, Tmax, D)).astype(np.float32)
    kc[:, past:] = np.nan
    vc[:, past:] = np.nan
    return kc, vc


def _check_attention(name, form, qkv_in, kc, vc, past, heads, bias=None, info=None):
    """qkv_in: [P * nd, 3 D] or slices [S, P, 3 D].  Returns the device output; info (a dict) receives the case's E32 and its scale
    vmax = max|v| over the history and the new rows."""
    ops = _ops()
    P, Tmax, D = kc.shape
    if qkv_in.ndim == 3:      # the kernel's own fp32 slice sum: 0 + p0 + p1 + ..., then + bias
        acc = np.zeros(qkv_in.shape[1:], np.float32)
        for s in range(qkv_in.shape[0]):
            acc = acc + qkv_in[s]
        qkv32 = acc + (bias if bias is not None else np.float32(0))
        qkv64 = R.f64(qkv_in).sum(0) + (R.f64(bias) if bias is not None else 0.0)
    else:
        qkv32, qkv64 = qkv_in, R.f64(qkv_in)
    nd = qkv32.shape[0] // P
    out, kc2, vc2 = ops.gpt2_attention(qkv_in, kc, vc, past, heads, form=form, bias=bias)
    ref, _, _ = R.attention(qkv64, np.nan_to_num(kc), np.nan_to_num(vc), past, heads)
    q3 = qkv32.reshape(P, nd, 3 * D)
    vmax = max(float(np.abs(q3[:, :, 2 * D:]).max()), float(np.abs(vc[:, :past]).max()) if past else 0.0)
    e32 = _check_e32(name, out, ref, _att32(qkv32, kc, vc, past, heads), vmax)
    if info is not None:
        info.update(e32=e32, vmax=vmax)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(kc2[:, past:past + nd]), bits(q3[:, :, D:2 * D])), "%s: appended key rows differ from k" % name
    assert np.array_equal(bits(vc2[:, past:past + nd]), bits(q3[:, :, 2 * D:])), "%s: appended value rows differ from v" % name
    assert np.array_equal(bits(kc2[:, :past]), bits(kc[:, :past])) and np.array_equal(bits(vc2[:, :past]), bits(vc[:, :past])), \
        "%s: history rows changed" % name
    assert np.isnan(kc2[:, past + nd:]).all() and np.isnan(vc2[:, past + nd:]).all(), "%s: rows above the history were written" % name
    return out


# (Tmax, past, heads, P, S): every past of the issue's list at Tmax = 64, the edges of Tmax = 8; P * heads % 4 != 0 in several
STEP_ATT = [(64, 0, 1, 5, 1), (64, 1, 2, 3, 2), (64, 15, 12, 2, 3), (64, 16, 1, 33, 4), (64, 17, 2, 8, 5), (64, 47, 12, 3, 8),
            (64, 48, 2, 7, 16), (64, 63, 1, 6, 0), (64, 63, 12, 5, 3), (8, 0, 2, 5, 4), (8, 1, 1, 1, 1), (8, 7, 12, 1, 2), (64, 33, 2, 64, 0)]


@pytest.mark.parametrize("Tmax,past,heads,P,S", STEP_ATT)
def test_attention_step_kernel(Tmax, past, heads, P, S):
    D = 64 * heads
    rs = np.random.RandomState(31 + Tmax + past + heads + P + S)
    kc, vc = _caches(rs, P, Tmax, D, past)
    if S:
        qkv = (rs.standard_normal((S, P, 3 * D)) * S ** -0.5).astype(np.float32)
        bias = (0.1 * rs.standard_normal(3 * D)).astype(np.float32)
    else:
        qkv, bias = rs.standard_normal((P, 3 * D)).astype(np.float32), None
    _check_attention("attention step Tmax%d past%d heads%d P%d S%d" % (Tmax, past, heads, P, S), "step", qkv, kc, vc, past, heads, bias)


@pytest.mark.parametrize("nd,past,heads,P", [(1, 0, 1, 3), (23, 0, 2, 5), (64, 0, 12, 2), (126, 0, 2, 3), (1, 64, 12, 3), (1, 255, 1, 5),
                                             (5, 60, 2, 3)])
def test_attention_general_kernel_host_past(nd, past, heads, P):
    D = 64 * heads
    rs = np.random.RandomState(41 + nd + past + heads)
    kc, vc = _caches(rs, P, past + nd + 2, D, past)
    qkv = rs.standard_normal((P * nd, 3 * D)).astype(np.float32)
    _check_attention("attention general nd%d past%d heads%d P%d" % (nd, past, heads, P), "general", qkv, kc, vc, past, heads)


@pytest.mark.parametrize("Tmax,past,heads,P", [(65, 0, 2, 3), (65, 64, 1, 5), (256, 0, 12, 1), (256, 64, 2, 8), (256, 255, 1, 33), (65, 64, 12, 2)])
def test_attention_general_kernel_device_past(Tmax, past, heads, P):
    D = 64 * heads
    rs = np.random.RandomState(51 + Tmax + past + heads)
    kc, vc = _caches(rs, P, Tmax, D, past)
    qkv = rs.standard_normal((P, 3 * D)).astype(np.float32)
    _check_attention("attention general_dev Tmax%d past%d heads%d P%d" % (Tmax, past, heads, P), "general_dev", qkv, kc, vc, past, heads)


@pytest.mark.parametrize("form", ["step", "general", "general_dev"])
def test_attention_saturated_and_uniform_softmax(form):
    """One key whose score exceeds every other by > 100 (the output is that key's value row); identical keys (the output is the mean
    of the value rows)."""
    heads, P, past, Tmax = 2, 3, 40, 64
    D = 64 * heads
    rs = np.random.RandomState(61)
    kc, vc = _caches(rs, P, Tmax, D, past)
    qkv = rs.standard_normal((P, 3 * D)).astype(np.float32)
    qkv[:, :D] = 4.0
    kc[:, 17] = 4.0                                    # score 128 against N(0, 16) for the others
    keys = np.concatenate([kc[:, :past], qkv[:, None, D:2 * D]], axis=1).reshape(P, past + 1, heads, 64)     # history + the new key
    s = np.einsum("phd,pthd->pht", R.f64(qkv[:, :D]).reshape(P, heads, 64), R.f64(keys)) / 8.0
    assert (np.sort(s, axis=-1)[..., -1] - np.sort(s, axis=-1)[..., -2]).min() > 100 and (s.argmax(-1) == 17).all()
    out = _check_attention("attention %s saturated softmax" % form, form, qkv, kc, vc, past, heads)
    np.testing.assert_array_equal(out, vc[:, 17])
    kc2, vc2 = _caches(rs, P, Tmax, D, past)
    kc2[:, :past] = kc2[:, :1]
    qkv2 = rs.standard_normal((P, 3 * D)).astype(np.float32)
    qkv2[:, D:2 * D] = kc2[:, 0]
    out = _check_attention("attention %s identical keys" % form, form, qkv2, kc2, vc2, past, heads)
    mean_v = (R.f64(vc2[:, :past]).sum(1) + R.f64(qkv2[:, 2 * D:])) / (past + 1)
    # 41 equal weights: each of the 41 products and sums rounds once, the weight 1/41 a few times (a wrong or missing row is 1/41 of |v|)
    assert np.abs(out - mean_v).max() <= 256 * U * np.abs(vc2[:, :past]).max()


@pytest.mark.parametrize("past,heads,P", [(0, 2, 5), (16, 1, 3), (47, 12, 2), (63, 2, 7)])
def test_attention_step_and_general_kernels_agree(past, heads, P):
    """The same inputs through the step kernel and the general kernel (both forms): each within the attention bar of the reference, and
    the step kernel within the same bar (8 E32 of max|v|) of the general kernel.  Without a history (past = 0) the two are bitwise
    equal, as the step kernel's comment says, and that is asserted; with one they are not (logged with the difference)."""
    D = 64 * heads
    rs = np.random.RandomState(71 + past + heads)
    kc, vc = _caches(rs, P, 64, D, past)
    qkv = rs.standard_normal((P, 3 * D)).astype(np.float32)
    info = {}
    outs = {f: _check_attention("attention agree %s past%d heads%d" % (f, past, heads), f, qkv, kc, vc, past, heads, info=info)
            for f in ("step", "general", "general_dev")}
    np.testing.assert_array_equal(outs["general"], outs["general_dev"])
    e32, vmax = info["e32"], info["vmax"]                # (the same inputs, reference and scale for the three forms)
    d = float(np.abs(outs["step"].astype(np.float64) - outs["general"]).max()) / vmax
    same = np.array_equal(outs["step"], outs["general"])
    diag("[check] %-44s E32 %.3e bar %.3e observed %.3e (%.2f x E32) bitwise equal %s %s"
         % ("attention step vs general past%d heads%d" % (past, heads), e32, MARGIN * e32, d, d / max(e32, 1e-300), same,
            "OK" if d <= MARGIN * e32 else "FAIL"))
    assert d <= MARGIN * e32, "step and general kernel differ by %.3e of max|v|, bar %.3e = 8 x E32" % (d, MARGIN * e32)
    if past == 0:
        assert same, "past = 0: the step kernel's output is not bitwise the general kernel's"


def test_attention_op_refuses_what_the_kernels_do_not_take():
    ops = _ops()
    kc = np.zeros((1, 130, 64), np.float32)
    with pytest.raises(RuntimeError, match="exceed 160 KB of LDS"):
        ops.gpt2_attention(np.zeros((127, 192), np.float32), kc, kc, 0, 1, form="general")
    with pytest.raises(RuntimeError, match="Tmax <= 64"):
        ops.gpt2_attention(np.zeros((1, 192), np.float32), kc, kc, 0, 1, form="step")


# ---- vocabulary head ------------------------------------------------------------------------------------------------------------------
def _head_inputs(M, V, K, ties):
    """ties: list of (row, i, j): wte rows i and j are made equal, a generic direction scaled so that its logit for `row` is 10 against
    N(0, 1) for the ordinary columns — both columns hold that row's (bitwise equal) maximum.  (Not a multiple of LN_f(x[row]) itself:
    then all K products have one sign, the kernel's fmaf chain over K = 1024 is ~10 x less accurate than a blocked float32 sum — a numpy
    emulation of a sequential chain gives 8.6e-7 of the scale where E32 is 9.3e-8 — and 8 E32 measures the CPU's summation order, not the
    kernel.)"""
    rs = np.random.RandomState(81 + M + V + K)
    x, g, b = _ln_inputs(rs, M, K)
    wte = (rs.standard_normal((V, K)) * K ** -0.5).astype(np.float32)
    y = R.layernorm(x, g, b)
    for row, i, j in ties:
        cand = rs.standard_normal((64, K))                # the candidate most aligned with this row and least with the other tie rows
        z = cand @ y[row]
        zo = np.abs(cand @ y[[r for r, _, _ in ties if r != row]].T).max(axis=1) if len(ties) > 1 else 0.0
        c = int((np.abs(z) / (zo + 0.25 * np.sqrt(K))).argmax())
        wte[i] = wte[j] = (cand[c] * (10.0 / z[c])).astype(np.float32)
    return x, g, b, wte


def _tie_plan(M, V):
    last = ((V - 1) // 32) * 32
    cols = [(70, 75), (100, 200), (last + 1, min(last + 6, V - 1))]        # inside one block, across two, in the last (partial) block
    return [(row, i, j) for row, (i, j) in enumerate(cols)] if M >= 3 else [(0,) + cols[V % 3]]


@pytest.mark.parametrize("M,V,K", [(1, 4096, 128), (33, 5000, 768), (64, 50257, 768), (64, 4096, 1024), (1, 5000, 1024), (33, 50257, 128)])
def test_head_logits_pairs_and_pick(M, V, K):
    ops = _ops()
    ties = _tie_plan(M, V)
    x, g, b, wte = _head_inputs(M, V, K, ties)
    r = ops.gpt2_head(x, wte, g, b)
    name = "head M%d V%d K%d" % (M, V, K)
    _check_stats(name + " stats", r["stats"], x)
    y = R.layernorm(x, g, b)
    _check_e32(name + " logits", r["logits"], y @ R.f64(wte).T, (_ln32(x, g, b) @ _t32(wte).T).numpy(), np.abs(y) @ np.abs(R.f64(wte)).T)
    pv, pi = R.block_pairs(r["logits"])
    assert np.array_equal(r["pair_val"], pv), "%s: block maxima differ from the device's own logits" % name
    assert np.array_equal(r["pair_idx"], pi), "%s: block arg-max is not the lowest index of the maximum" % name
    assert np.array_equal(r["token"], r["logits"].argmax(1)), "%s: the pick is not the first maximum of the device's own logits" % name
    for row, i, j in ties:
        lg = r["logits"][row]
        assert lg[i] == lg[j] == lg.max(), "%s: planted tie (%d, %d) of row %d is not the row maximum" % (name, i, j, row)
        assert r["token"][row] == min(i, j), "%s: tie (%d, %d) picked %d" % (name, i, j, r["token"][row])
    diag("[gpt2 ops] %s: pairs and pick exact, %d planted tie(s) pick the lowest index" % (name, len(ties)))


@pytest.mark.parametrize("M,V,K", [(1, 4096, 128), (33, 5000, 768), (64, 4096, 1024), (64, 50257, 768)])
def test_head_tail_matches_pick_and_embed_step(M, V, K):
    """launch_gpt2_head with the arg-max + embed / advance tail: the token of the plain arg-max pick, the next step's x / statistics bitwise
    as launch_gpt2_embed_step leaves them, the state advanced to {past + 1, step + 1, 0}."""
    ops = _ops()
    x, g, b, wte = _head_inputs(M, V, K, _tie_plan(M, V))
    wpe = (0.01 * np.random.RandomState(5).standard_normal((64, K))).astype(np.float32)
    past, step = 22, 3
    pick = ops.gpt2_head(x, wte, g, b)["token"]
    t = ops.gpt2_head(x, wte, g, b, tail=True, wpe=wpe, past=past, step=step)
    xe, se = ops.gpt2_embed_step(pick, wte, wpe, past + 1, step + 1)
    name = "head tail M%d V%d K%d" % (M, V, K)
    assert np.array_equal(t["token"], pick), "%s: token differs from launch_gpt2_head's pick" % name
    assert t["state"].tolist() == [past + 1, step + 1, 0], "%s: state %r" % (name, t["state"].tolist())
    bits = lambda a: a.view(np.uint32)
    assert np.array_equal(bits(t["x_next"]), bits(xe)), "%s: next x differs from gpt2_embed_step_kernel's" % name
    assert np.array_equal(bits(t["stats_next"]), bits(se)), "%s: next statistics differ from gpt2_embed_step_kernel's" % name
    assert np.array_equal(xe, wte[pick] + wpe[past + 1])
    _check_stats(name + " next stats", t["stats_next"], xe)
    diag("[gpt2 ops] %s: token, next x / stats (bitwise vs embed_step) and state OK" % name)
