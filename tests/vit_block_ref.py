"""Float64 restatements of the two kernels that do a CLIP ViT block's arithmetic — the GEMM with its five epilogues (csrc/gemm_tiled.hip,
csrc/conv_direct.hip gemm_direct_kernel) and attention (csrc/kernels_clip.hip) — with their float32 twins, the case tables and the bars
of tests/test_gpu_vit_block_ops.py (test infrastructure).

tests/test_vit_block_ref.py pins the float64 functions to numpy.matmul / torch in float64 on the CPU and shows that the bars can fail: the
restatements take a `fault`, and every planted fault exceeds the bar on a case of the family aimed at it.

Every function takes `dt`: numpy float64 (the reference) or float32 (the twin the bars are derived from: the same formula in float32,
long sums added one term after the other).  The twin restates the kernels' arithmetic CHOICES, not their order: exp is
exp2(float32(x log2 e)) (__expf is v_exp_f32 on the scaled argument), QuickGELU is v (1 / (1 + exp(-1.702 v))) (a reciprocal and a product,
gemm_tiled's v_rcp_f32 form).  Operands are the fp16-rounded values the device holds; nothing here rounds an OUTPUT to fp16 — the bar
carries the store's half ulp.
"""
import numpy as np

F32, F64 = np.float32, np.float64
SQRT2 = np.sqrt(2.0)
LOG2E = 1.4426950408889634
PAD = F32(-1234.0)           # what the tests put into the ldo padding (exact in fp16)
MODES = (0, 1, 2, 3, 4)      # GemmParams::mode: 0 fp16 v, 1 fp16 QuickGELU(v), 2 fp32 acc + v, 3 fp32 v, 4 fp32 lrelu(v) sqrt2
STORE16 = {0: True, 1: True, 2: False, 3: False, 4: False}


def h16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=F32).astype(np.float16).astype(F32)


def _a(x, dt):
    return np.asarray(x, dtype=dt)


def exp(x, dt):
    """e^x; the float32 twin as the kernels' __expf: exp2 of the argument scaled (and rounded) in float32."""
    x = _a(x, dt)
    if dt == F64:
        return np.exp(x)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp2((x * F32(LOG2E)).astype(F32)).astype(F32)


# ---- GEMM --------------------------------------------------------------------------------------------------------------------------------
def product(a, w, dt, k_end=None):
    """a [.., M, K] @ w [.., N, K]^T; the float32 twin adds the K products of an output one after the other."""
    a, w = _a(a, dt), _a(w, dt)
    K = a.shape[-1] if k_end is None else k_end
    if dt == F64:
        return a[..., :K] @ np.swapaxes(w[..., :K], -1, -2)
    acc = np.zeros(a.shape[:-1] + (w.shape[-2],), dt)
    for k in range(K):
        acc = acc + a[..., :, k, None] * w[..., None, :, k]
    return acc


def epilogue(v, bias, mode, acc, dt):
    """v [.., M, N] (the product) -> what the kernel stores, before the store's own rounding."""
    v = _a(v, dt)
    if bias is not None:
        v = v + _a(bias, dt)
    if mode == 1:
        return v * (dt(1) / (dt(1) + exp(dt(-1.702) * v, dt)))
    if mode == 2:
        return _a(acc, dt) + v
    if mode == 4:
        return np.where(v > 0, v, dt(0.2) * v) * dt(SQRT2)
    return v


def gemm(a, w, bias, mode, acc=None, dt=F64):
    return epilogue(product(a, w, dt), bias, mode, acc, dt)


GEMM_FAULTS = ("k_tail", "bias_shift", "row_clamp", "res_clamp", "tile_skip")


def gemm_faulty(a, w, bias, mode, acc, fault, tile=(128, 64)):
    """The float64 GEMM with one planted fault, as a kernel could have it:
    k_tail      the last 16 of K dropped (a K loop that stops one MFMA early)
    bias_shift  bias read 4 columns off (a quad index off by one)
    row_clamp   the rows of a partial m tile return row M - 1's values (the clamped operand loads, stored to the lane's own row)
    res_clamp   mode 2's residual of those rows taken from the clamped row M - 1
    tile_skip   one tile not stored (the tile walk's early return one tile too soon): the preloaded NaN stays"""
    assert fault in GEMM_FAULTS
    a, w = _a(a, F64), _a(w, F64)
    M, N = a.shape[-2], w.shape[-2]
    m_part = (M // tile[0]) * tile[0]                       # first row of the partial m tile (== M: there is none)
    v = product(a, w, F64, k_end=a.shape[-1] - 16 if fault == "k_tail" else None)
    b = None if bias is None else _a(bias, F64)
    if fault == "bias_shift" and b is not None:
        b = np.roll(b, -4)
    acc_ = None if acc is None else _a(acc, F64).copy()
    if fault == "res_clamp" and acc_ is not None:
        acc_[..., m_part:, :] = acc_[..., M - 1:M, :]
    out = epilogue(v, b, mode, acc_, F64)
    if fault == "row_clamp":
        out[..., m_part:, :] = out[..., M - 1:M, :]
    if fault == "tile_skip":
        out[..., M - min(M, tile[0]):, N - tile[1]:] = np.nan
    return out


def gemm_inputs(seed, M, N, K, batch=1):
    """(a [batch, M, K], w [batch, N, K], bias [N], acc [batch, M, N]): fp16-rounded operands, products of unit variance (max|ref| about 5
    at every K), rows O(1) from their neighbours, bias and residual different in every column and row."""
    rng = np.random.default_rng([seed, M, N, K, batch])
    a = h16(rng.standard_normal((batch, M, K)) + (np.arange(M)[:, None] % 3 - 1.0))
    w = h16(rng.standard_normal((batch, N, K)) / np.sqrt(K))
    bias = (0.5 * rng.standard_normal(N)).astype(F32)
    acc = rng.standard_normal((batch, M, N)).astype(F32)
    return a, w, bias, acc


# The cases of tests/test_gpu_vit_block_ops.py: (M, N, K), the smallest shapes at which each path exists.
TILED_64 = [(64, 64, 64), (65, 192, 128), (127, 64, 192), (129, 128, 64), (150, 256, 192), (300, 320, 448)]
TILED_128 = [(64, 128, 64), (129, 128, 64), (150, 256, 192), (300, 384, 128)]
CAND_ROWS_128 = 512          # 512 * 64 / 128 = 256 nominal m tiles: launch_gemm_tiled's fill rule takes the 128-wide instance at any N % 128 == 0
WALK_T = (7, 8, 9, 15, 16, 17, 23)
WALK_64 = [(128 * t - 37, 64, 64) for t in WALK_T] + [(300, 192, 64)]      # mode 3
WALK_128 = [(300, 384, 64)]                                                # mode 3
LDO = [((150, 192, 128), ldo) for ldo in (196, 256)]                       # modes 0, 2, 3
LDO_MODES = (0, 2, 3)
BATCHED = [((400, 128, 64), True, "gemm_tiled_kernel<128>"), ((400, 128, 64), False, "gemm_tiled_kernel<64>"),
           ((130, 128, 64), False, "gemm_tiled_kernel<64>")]               # batch 3: (shape, cand_batch, instance)
BATCH = 3
REFUSED = [((150, 128, 96), 128, "K"), ((63, 128, 64), 128, "M"), ((150, 96, 64), 96, "N"), ((150, 128, 64), 130, "ldo")]   # (shape, ldo, what)
DIRECT = [((1, 24, 16), 1, None, "gemm_direct_kernel<1>"), ((5, 32, 48), 1, None, "gemm_direct_kernel<1>"),
          ((33, 33, 80), 1, None, "gemm_direct_kernel<2>"), ((63, 64, 96), 1, None, "gemm_direct_kernel<2>"),
          ((130, 65, 96), 1, None, "gemm_direct_kernel<4>"), ((130, 200, 96), 1, None, "gemm_direct_kernel<4>"),
          ((17, 40, 32), 2, None, "gemm_direct_kernel<2>"), ((33, 33, 80), 1, 36, "gemm_direct_kernel<2>")]   # (shape, batch, ldo, instance)


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
def split_qkv(qkv, n_img, L, heads, dt):
    """qkv [n_img L, 3 heads 64] -> q, k, v [n_img heads, L, 64]."""
    x = _a(qkv, dt).reshape(n_img, L, 3, heads, 64).transpose(2, 0, 3, 1, 4).reshape(3, n_img * heads, L, 64)
    return x[0], x[1], x[2]


def merge_heads(o, n_img, L, heads):
    return o.reshape(n_img, heads, L, 64).transpose(0, 2, 1, 3).reshape(n_img * L, heads * 64)


def scores(q, k, causal, dt, q0=0):
    """q k^T / 8 with -inf where a key is masked (q holds queries q0 ..); the twin adds the 64 products one after the other."""
    if dt == F64:
        s = q @ np.swapaxes(k, -1, -2)
    else:
        qT, kT = np.ascontiguousarray(np.swapaxes(q, -1, -2)), np.ascontiguousarray(np.swapaxes(k, -1, -2))
        s = np.zeros(q.shape[:-1] + (k.shape[-2],), dt)
        t = np.empty_like(s)
        for d in range(q.shape[-1]):
            np.multiply(qT[..., d, :, None], kT[..., d, None, :], out=t)
            s += t
    s = s * dt(0.125)
    if causal:
        s = np.where(np.arange(s.shape[-1])[None, :] > q0 + np.arange(s.shape[-2])[:, None], dt(-np.inf), s)
    return s


def attention(qkv, n_img, L, heads, causal, dt=F64):
    """nn.MultiheadAttention's core per (image, head), head dim 64: softmax(q k^T / 8 [+ causal]) v -> [n_img L, heads 64]."""
    q, k, v = split_qkv(qkv, n_img, L, heads, dt)
    if dt == F64:
        s = scores(q, k, causal, dt)
        e = exp(s - s.max(axis=-1, keepdims=True), dt)
        return merge_heads((e / e.sum(axis=-1, keepdims=True)) @ v, n_img, L, heads)
    out = np.empty(q.shape, dt)
    for q0 in range(0, L, 256):      # (blocks of queries: the same arithmetic on arrays that stay in the cache)
        s = scores(q[..., q0:q0 + 256, :], k, causal, dt, q0)
        eT = np.ascontiguousarray(np.swapaxes(exp(s - s.max(axis=-1, keepdims=True), dt), -1, -2))      # [.., key, query]
        z = np.zeros(eT.shape[:-2] + eT.shape[-1:], dt)
        for j in range(L):
            z += eT[..., j, :]
        pT = eT * (dt(1) / z)[..., None, :]
        o = np.zeros(s.shape[:-1] + (64,), dt)
        t = np.empty_like(o)
        for j in range(L):
            np.multiply(pT[..., j, :, None], v[..., j, None, :], out=t)
            o += t
        out[..., q0:q0 + 256, :] = o
    return merge_heads(out, n_img, L, heads)


def lane_half(L):
    """The lane half that holds key j's score in the kernels' accumulator layout: keys with j % 8 >= 4 against the rest."""
    return (np.arange(L) >> 2) & 1


ATTENTION_FAULTS = ("last_key", "causal_ge", "half_max", "alpha_sum")


def attention_faulty(qkv, n_img, L, heads, causal, fault):
    """Attention with one planted fault, as a kernel could have it:
    last_key   key L - 1 masked off (`key >= L - 1`)
    causal_ge  the causal mask `key >= query` instead of `key > query`
    half_max   the two lane halves' maxima not combined: each half's scores lose their OWN maximum, the sums are combined — the halves'
               weights are off by e^gap against each other (a maximum that is merely the wrong one of the two is no fault until the
               float32 exp overflows: softmax does not care which constant it subtracts)
    alpha_sum  the online softmax over key tiles of 64 with alpha = exp(m_old - m_new) applied to the output but not to the running sum"""
    assert fault in ATTENTION_FAULTS
    dt = F64
    q, k, v = split_qkv(qkv, n_img, L, heads, dt)
    s = scores(q, k, causal, dt)
    if fault == "last_key":
        s[..., L - 1] = -np.inf
    if fault == "causal_ge" and causal:
        s = np.where(np.arange(L)[None, :] >= np.arange(L)[:, None], -np.inf, s)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if fault == "half_max":
            h1 = lane_half(L) == 1
            m0 = np.where(h1, -np.inf, s).max(axis=-1, keepdims=True)
            m1 = np.where(h1, s, -np.inf).max(axis=-1, keepdims=True) if h1.any() else m0
            e = exp(s - np.where(h1, m1, m0), dt)
            return merge_heads((e / e.sum(axis=-1, keepdims=True)) @ v, n_img, L, heads)
        if fault == "alpha_sum":
            m, z, o = np.full(s.shape[:-1] + (1,), -np.inf), 0.0, 0.0
            for k0 in range(0, L, 64):
                st = s[..., k0:k0 + 64]
                mn = np.maximum(m, st.max(axis=-1, keepdims=True))
                alpha, e = np.exp(m - mn), np.exp(st - mn)
                z = z + e.sum(axis=-1, keepdims=True)               # the fault: z * alpha + ...
                o = o * alpha + e @ v[..., k0:k0 + 64, :]
                m = mn
            return merge_heads(o / z, n_img, L, heads)
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        return merge_heads((e / e.sum(axis=-1, keepdims=True)) @ v, n_img, L, heads)


FAMILIES = ("unit", "peaked", "late", "early")
PEAKED_STD = 4.5


def attention_inputs(family, n_img, L, heads, seed=0):
    """qkv [n_img L, 3 heads 64], fp16-rounded.  unit: N(0, 1) — a row's scores span about 7.  peaked: N(0, 4.5) — scores of deviation 20:
    most rows span more than 88 (float32 exp overflows on a wrong maximum) and the two lane halves' maxima lie tens apart; max|qkv| about
    18 is far inside fp16.  late / early: unit, key j scaled by 0.5 + 4 j / L (late: the running maximum keeps moving in the late key
    tiles) or the reverse (early: it never moves after tile 0)."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), n_img, L, heads])
    x = rng.standard_normal((n_img, L, 3, heads, 64)) * (PEAKED_STD if family == "peaked" else 1.0)
    if family in ("late", "early"):
        ramp = 0.5 + 4.0 * np.arange(L) / L
        x[:, :, 1] *= (ramp if family == "late" else ramp[::-1])[None, :, None, None]
    return h16(x.reshape(n_img * L, 3 * heads * 64))


def score_spread(qkv, n_img, L, heads):
    """(largest score range of a row, largest gap between a row's two lane-half maxima) of the non-causal scores."""
    q, k, _ = split_qkv(qkv, n_img, L, heads, F64)
    s = scores(q, k, False, F64)
    h1 = lane_half(L) == 1
    gap = np.abs(np.where(h1, s, -np.inf).max(axis=-1) - np.where(h1, -np.inf, s).max(axis=-1)) if h1.any() else np.zeros(1)
    return float((s.max(axis=-1) - s.min(axis=-1)).max()), float(gap.max())


# 3 images x 2 heads unless stated: (kernel, L) — launch_attention's thresholds are 64 and 96
N_IMG, HEADS = 3, 2
ATT_MFMA2 = (1, 31, 32, 33, 50, 63, 64)
ATT_MFMA3 = (65, 77, 95, 96)
ATT_STREAM = (97, 127, 128, 129, 191, 192, 193, 256, 257)
ATT_ODD_PAIRS = [(3, 1), (1, 1)]      # (n_img, heads) at L = 50: attention_mfma_kernel<2>'s half-empty last workgroup
ATT_LIMIT = 4096                      # 1 image, 1 head
ATT_LENGTHS = [("attention_mfma_kernel<2>", L) for L in ATT_MFMA2] + [("attention_mfma_kernel<3>", L) for L in ATT_MFMA3] + \
              [("attention_stream_kernel", L) for L in ATT_STREAM]


# ---- bars ---------------------------------------------------------------------------------------------------------------------------------
def bar(ref64, ref32, store16):
    """(tolerance per element, its case-wide part, the twin's error).  |got - ref64| <= 4 max|ref32 - ref64| over the case — one float32
    ulp of max|ref64| where the twin's error is exactly zero — plus, where the kernel stores fp16, 2^-11 |ref64| + 2^-25 per element
    (half an fp16 ulp: normal, and in the subnormal range)."""
    ref64 = np.asarray(ref64, F64)
    e32 = float(np.abs(np.asarray(ref32, F64) - ref64).max())
    base = float(np.spacing(F32(np.abs(ref64).max()))) if e32 == 0.0 else 4 * e32
    tol = base + (2.0 ** -11 * np.abs(ref64) + 2.0 ** -25 if store16 else 0.0) + np.zeros_like(ref64)
    return tol, base, e32


def judge(got, ref64, ref32, store16):
    """(passes, max err, case-wide bar, twin's error, worst err / tol).  A non-finite element never passes."""
    got, ref64 = np.asarray(got, F64), np.asarray(ref64, F64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    tol, base, e32 = bar(ref64, ref32, store16)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref64)
        ok = bool(np.isfinite(got).all() and (err <= tol).all())
    fin = np.isfinite(err)
    return ok, float(err[fin].max()) if fin.any() else float("nan"), base, e32, float((err[fin] / tol[fin]).max()) if fin.any() else float("nan")
