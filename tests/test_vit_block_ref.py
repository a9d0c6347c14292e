"""tests/vit_block_ref.py on the CPU (no GPU, no built library): the float64 GEMM against numpy.matmul and torch's epilogues in float64, the
float64 attention against torch in float64, the input families keep their point, the case tables agree with the launchers' rules as the
sources state them — and the bars CAN fail: every planted fault exceeds the bar on a case of the family aimed at it, while the float32
twin and an fp16-rounded reference stay inside."""
import numpy as np
import pytest
import torch

import vit_block_ref as R

F32, F64 = np.float32, np.float64


# ---- the float64 references are the operations they claim to be ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 32, 48), (65, 192, 128), (130, 65, 96)])
@pytest.mark.parametrize("mode", R.MODES)
def test_gemm_is_matmul_and_torch_epilogues(shape, mode):
    a, w, bias, acc = R.gemm_inputs(1, *shape, batch=2)
    v = torch.from_numpy(np.matmul(a.astype(F64), w.astype(F64).transpose(0, 2, 1)) + bias.astype(F64))
    want = {0: v, 1: v * torch.sigmoid(1.702 * v), 2: torch.from_numpy(acc.astype(F64)) + v, 3: v,
            4: torch.nn.functional.leaky_relu(v, 0.2) * 2.0 ** 0.5}[mode].numpy()
    got = R.gemm(a, w, bias, mode, acc)
    assert got.dtype == F64 and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    twin = R.gemm(a, w, bias, mode, acc, dt=F32)
    assert twin.dtype == F32
    # the twin is float32 arithmetic on the same operands: K + 3 roundings of values <= max|a| max|w| K
    assert np.abs(twin - want).max() <= (shape[2] + 3) * 2.0 ** -24 * (np.abs(a).max() * np.abs(w).max() * shape[2] + np.abs(want).max())
    assert np.abs(twin - want).max() > 0


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("L,causal", [(1, 0), (1, 1), (33, 0), (50, 1), (77, 1), (130, 0), (130, 1)])
def test_attention_is_torch_float64(family, L, causal):
    n_img, heads = 2, 3
    qkv = R.attention_inputs(family, n_img, L, heads)
    x = torch.from_numpy(qkv.astype(F64)).reshape(n_img, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = x[0] @ x[1].transpose(-1, -2) / 8.0
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)
    want = (torch.softmax(s, dim=-1) @ x[2]).permute(0, 2, 1, 3).reshape(n_img * L, heads * 64).numpy()
    got = R.attention(qkv, n_img, L, heads, causal)
    assert got.dtype == F64 and np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1.0)
    twin = R.attention(qkv, n_img, L, heads, causal, dt=F32)
    assert twin.dtype == F32 and np.isfinite(twin).all()
    ok, err, base, e32, _ = R.judge(twin, got, twin, True)
    assert ok and e32 < 1e-4 * max(np.abs(want).max(), 1.0)


def test_twin_exp_is_exp2_of_the_scaled_argument():
    x = np.linspace(-100, 0, 4001).astype(F32)
    got = R.exp(x, F32)
    assert got.dtype == F32 and R.exp(np.array([-np.inf], F32), F32)[0] == 0
    # the argument's rounding: |x log2 e| 2^-24 ln 2 relative, + exp2's own ulp
    rel = np.abs(got.astype(F64) - np.exp(x.astype(F64))) / np.exp(x.astype(F64))
    assert (rel[got > 1e-37] <= (np.abs(x[got > 1e-37]) * 1.4427 * 2.0 ** -24 + 2.0 ** -22)).all()
    assert rel.max() > 2.0 ** -22      # it IS the fast form: libm's exp would stay inside an ulp


# ---- the input families keep their point --------------------------------------------------------------------------------------------------
def _att_cases():
    return [(R.N_IMG, L, R.HEADS) for _, L in R.ATT_LENGTHS] + [(n, 50, h) for n, h in R.ATT_ODD_PAIRS] + [(1, R.ATT_LIMIT, 1)]


@pytest.mark.parametrize("n_img,L,heads", _att_cases())
def test_peaked_family_overflows_a_wrong_maximum(n_img, L, heads):
    rng_, gap = R.score_spread(R.attention_inputs("peaked", n_img, L, heads), n_img, L, heads)
    rng_u, _ = R.score_spread(R.attention_inputs("unit", n_img, L, heads), n_img, L, heads)
    assert rng_u < 20
    if L >= 31:      # (shorter rows are exempt: too few keys for the range)
        assert rng_ > 88, "no row's scores span the float32 exp range"
        assert gap > 20, "no row's two lane-half maxima lie apart"
    qkv = R.attention_inputs("peaked", n_img, L, heads)
    assert np.abs(qkv).max() < 40 and np.isfinite(qkv).all()


@pytest.mark.parametrize("L", [97, 193, 257])
def test_late_family_moves_the_running_maximum(L):
    def moves(family):
        q, k, _ = R.split_qkv(R.attention_inputs(family, R.N_IMG, L, R.HEADS), R.N_IMG, L, R.HEADS, F64)
        s = R.scores(q, k, False, F64)
        tile_max = np.stack([s[..., k0:k0 + 64].max(axis=-1) for k0 in range(0, L, 64)], axis=-1)
        return (np.maximum.accumulate(tile_max, axis=-1)[..., 1:] > np.maximum.accumulate(tile_max, axis=-1)[..., :-1])
    late, early = moves("late"), moves("early")
    assert late.any(axis=-1).mean() > 0.9    # nearly every row's maximum moves after tile 0 ...
    assert late[..., -2 if L % 64 == 1 else -1].mean() > 0.8      # ... and for many still in the last tile of more than one key
    assert (~early.any(axis=-1)).mean() > 0.5    # most rows' maximum never moves after tile 0


# ---- the case tables against the launchers' rules (csrc/gemm_tiled.hip launch_gemm_tiled, conv_direct.hip launch_gemm_direct) ---------
def _tiled_instance(M, N, K, ldo=None, cand_rows=0, cand_batch=False, batch=1, nominal=64):
    if K % 64 or (ldo or N) % 4 or M < 64:
        return None
    gx = (M + 127) // 128
    gx_n = (cand_rows * nominal + 127) // 128 if cand_rows else gx
    gz_n = nominal if cand_batch else batch
    if N % 128 == 0 and gx_n * (N // 128) * gz_n >= 256:
        return "gemm_tiled_kernel<128>"
    return "gemm_tiled_kernel<64>" if N % 64 == 0 else None


def test_case_tables_name_the_instance_the_fill_rule_takes():
    for s in R.TILED_64 + R.WALK_64:
        assert _tiled_instance(*s) == "gemm_tiled_kernel<64>"
    assert _tiled_instance(*R.TILED_64[-1], cand_rows=R.CAND_ROWS_128) == "gemm_tiled_kernel<64>"      # N = 320: under any cand_rows
    for s in R.TILED_128 + R.WALK_128:
        assert _tiled_instance(*s, cand_rows=R.CAND_ROWS_128) == "gemm_tiled_kernel<128>"
    for s, ldo in R.LDO:
        assert _tiled_instance(*s, ldo=ldo) == "gemm_tiled_kernel<64>"
    for s, cb, name in R.BATCHED:
        assert _tiled_instance(*s, cand_batch=cb, batch=R.BATCH) == name
    for s, ldo, _ in R.REFUSED:
        assert _tiled_instance(*s, ldo=ldo) is None
    for (M, N, K), batch, ldo, name in R.DIRECT:
        assert name == "gemm_direct_kernel<%d>" % (4 if N > 64 else 2 if N > 32 else 1) and K % 16 == 0
    # the tile walk: tile counts whose last XCD slices are ragged, and whole ones
    assert sorted(((M + 127) // 128) * (N // 64) for M, N, _ in R.WALK_64) == [7, 8, 9, 9, 15, 16, 17, 23]
    assert [k for k, L in R.ATT_LENGTHS if L in (64, 65, 96, 97)] == ["attention_mfma_kernel<2>", "attention_mfma_kernel<3>",
                                                                       "attention_mfma_kernel<3>", "attention_stream_kernel"]


# ---- the bars can fail ------------------------------------------------------------------------------------------------------------------------
_gemm_cache = {}


def _gemm_case(shape, mode):
    """(inputs, float64 reference, float32 twin) of a case, computed once."""
    if shape not in _gemm_cache:
        a, w, bias, acc = R.gemm_inputs(2, *shape)
        _gemm_cache[shape] = (a, w, bias, acc, R.product(a, w, F64), R.product(a, w, F32))
    a, w, bias, acc, v64, v32 = _gemm_cache[shape]
    return (a, w, bias, acc), R.epilogue(v64, bias, mode, acc, F64), R.epilogue(v32, bias, mode, acc, F32)


GEMM_SHAPES = R.TILED_64 + [s for s, *_ in R.DIRECT[:6]]
# the family each fault is aimed at: (shape, mode)
GEMM_FAMILY = {
    "k_tail": [(s, m) for s in GEMM_SHAPES for m in R.MODES],
    "bias_shift": [(s, m) for s in GEMM_SHAPES for m in R.MODES],
    # (a partial m tile of ONE row is row M - 1 itself: M = 129 cannot show these two)
    "row_clamp": [(s, m) for s in R.TILED_64 + R.WALK_64[:2] if s[0] % 128 > 1 for m in R.MODES],
    "res_clamp": [(s, 2) for s in R.TILED_64 + R.TILED_128 if s[0] % 128 > 1],
    "tile_skip": [(s, 3) for s in R.WALK_64 + R.WALK_128],
}


@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_gemm_bars_hold_for_the_twin_and_an_fp16_store(shape):
    for mode in R.MODES:
        _, ref, twin = _gemm_case(shape, mode)
        ok, err, base, e32, worst = R.judge(twin, ref, twin, False)
        assert ok and worst <= 0.25 + 1e-12
        assert R.judge(R.h16(ref), ref, twin, True)[0]                       # a correctly rounded fp16 store stays inside
        if R.STORE16[mode]:
            assert not R.judge(R.h16(ref) * (1 + 2.0 ** -9), ref, twin, True)[0]      # two fp16 ulps do not
        if shape in R.TILED_64:      # the scale the bars are quoted at: max|ref| about 5, bars of 5e-6 .. 1.2e-5 on the fp32 modes
            assert 1e-6 < base < 4e-5 and 3.5 < np.abs(_gemm_case(shape, 3)[1]).max() < 9.0, (shape, mode, base)


@pytest.mark.parametrize("fault", R.GEMM_FAULTS)
def test_planted_gemm_fault_exceeds_the_bar(fault):
    caught = []
    for shape, mode in GEMM_FAMILY[fault]:
        (a, w, bias, acc), ref, twin = _gemm_case(shape, mode)
        tile = (128, 128 if shape in R.WALK_128 else 64)
        bad = R.gemm_faulty(a, w, bias, mode, acc, fault, tile=tile)[0]
        ok, err, base, _, _ = R.judge(bad, ref[0], twin[0], R.STORE16[mode])
        caught.append(not ok)
        print("%-10s %-16s mode %d: err %.3e bar %.3e %s" % (fault, shape, mode, err, base, "caught" if not ok else "MISSED"))
    assert len(caught) >= 1 and all(caught), "%s: missed on %d of %d cases" % (fault, caught.count(False), len(caught))


ATT_FAMILY = {      # (family, n_img, L, heads, causal)
    "last_key": [(f, R.N_IMG, L, R.HEADS, 0) for f in ("unit", "peaked") for _, L in R.ATT_LENGTHS],
    "causal_ge": [(f, R.N_IMG, L, R.HEADS, 1) for f in ("unit", "late") for _, L in R.ATT_LENGTHS],
    "half_max": [("peaked", R.N_IMG, L, R.HEADS, c) for _, L in R.ATT_LENGTHS if L >= 31 for c in (0, 1)],
    "alpha_sum": [(f, R.N_IMG, L, R.HEADS, c) for f in ("late", "peaked") for L in R.ATT_STREAM for c in (0, 1)],
}


@pytest.mark.parametrize("fault", R.ATTENTION_FAULTS)
def test_planted_attention_fault_exceeds_the_bar(fault):
    caught = []
    for family, n_img, L, heads, causal in ATT_FAMILY[fault]:
        qkv = R.attention_inputs(family, n_img, L, heads)
        ref, twin = R.attention(qkv, n_img, L, heads, causal), R.attention(qkv, n_img, L, heads, causal, dt=F32)
        assert R.judge(R.h16(ref), ref, twin, True)[0]
        bad = R.attention_faulty(qkv, n_img, L, heads, causal, fault)
        ok, err, base, _, _ = R.judge(bad, ref, twin, True)
        caught.append(not ok)
        print("%-10s %-7s L %4d causal %d: err %.3e bar %.3e %s" % (fault, family, L, causal, err, base, "caught" if not ok else "MISSED"))
    assert all(caught), "%s: missed on %d of %d cases" % (fault, caught.count(False), len(caught))
