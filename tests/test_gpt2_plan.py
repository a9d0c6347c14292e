"""CPU: what one GPT-2 token step launches, read from the engine's own host code (glass_host_gpt2_step_plan, include/glass_ops.h: the step
functions of gpt2_host.cpp run into a text instead of a stream) on a device of 256 compute units — the statements of the GEOMETRY_CASES
comment in test_gpt2.py as assertions, the step of GPT-2 small launch by launch, the split rule and its independence of the row count."""
import os
import re

import pytest

from clip_glass_amd import engine, ops
from test_gpt2 import GEOMETRY_CASES

pytestmark = pytest.mark.skipif(not os.path.exists(engine.LIB_PATH),
                                reason="libglass.so is not built here (python -c 'import __graft_entry__ as g; g.build()')")
N_CU = 256
N_LAYER = 2         # as _geometry_state


def _plan(case, sample=False):
    D, V, P, n_ctx, length, _ = GEOMETRY_CASES[case]
    return ops.host_gpt2_step_plan(P, D, V, N_LAYER, n_ctx + length, sample=sample, n_cu=N_CU)


def _names(plan):
    return [name for name, _, _ in plan]


def _products(plan):
    """(form, S, NK, LN) of every step product in launch order; form "stream" / "rowblk"."""
    out = []
    for name, grid, block in plan:
        m = re.fullmatch(r"gemm_f32_(stream|rowblk)_kernel<(\d+),(true|false),(true|false)>", name)
        if m:
            nk = int(m.group(2))
            assert block == ((128 if m.group(1) == "stream" else 64) * nk, 1, 1), (name, block)
            out.append((m.group(1), grid[1] if m.group(1) == "stream" else 1, nk, m.group(3) == "true"))
    return out


def _fused(plan):
    return "layernorm_kernel" not in _names(plan)


def _tail(plan):
    names = _names(plan)
    return names[-1] in ("gpt2_pick_embed_kernel", "gpt2_sample_kernel<true,true>") and "gpt2_embed_step_kernel" not in names and \
        "gpt2_advance_kernel" not in names


def _layer_splits(plan):
    """S of the four products of each layer (qkv, attention output, MLP first, MLP second); the layers must agree."""
    prods = _products(plan)[:4 * N_LAYER]
    per_layer = [prods[4 * l:4 * l + 4] for l in range(N_LAYER)]
    assert all(p == per_layer[0] for p in per_layer), per_layer
    return [s for _, s, _, _ in per_layer[0]], per_layer[0]


def test_case_D64():
    plan = _plan("D64")
    assert _fused(plan) and _tail(plan) and all(form == "stream" for form, _, _, _ in _products(plan))
    assert _layer_splits(plan)[0] == [1, 1, 1, 4]
    assert _names(plan).count("gpt2_attention_step_kernel") == N_LAYER and "gpt2_attention_kernel" not in _names(plan)
    assert "splitk_reduce_kernel" not in _names(plan)          # the one split product is finished by gpt2_finalize_kernel


def test_case_D192():
    plan = _plan("D192")
    splits, prods = _layer_splits(plan)
    assert _fused(plan) and _tail(plan) and splits == [3, 3, 3, 12]
    assert [nk for _, _, nk, _ in prods[:3]] == [1, 1, 1]


def test_case_D1024():
    plan = _plan("D1024")
    assert _fused(plan) and _tail(plan) and all(form == "stream" for form, _, _, _ in _products(plan))
    assert _layer_splits(plan)[0] == [4, 8, 4, 16]
    assert _names(plan).count("gpt2_finalize_kernel") == 2 * N_LAYER


@pytest.mark.parametrize("sample", [False, True])
def test_case_D1280(sample):
    plan = _plan("D1280", sample=sample)
    names = _names(plan)
    assert not _fused(plan) and names[0] == "gpt2_embed_step_kernel" and names[-1] == "gpt2_advance_kernel"
    assert names.count("layernorm_kernel") == 2 * N_LAYER + 1
    prods = _products(plan)         # launch_gemm_f32's streaming form: no LayerNorm in the product, at most four K parts, every split reduced
    assert len(prods) == 4 * N_LAYER + 1 and all(form == "stream" and not ln and nk in (1, 2, 4) for form, _, nk, ln in prods)
    assert names.count("splitk_reduce_kernel") == sum(1 for _, s, _, _ in prods if s > 1)
    assert names.count("gpt2_attention_kernel") == N_LAYER and "gpt2_attention_step_kernel" not in names
    assert "gpt2_finalize_kernel" not in names and "gpt2_head_kernel" not in names
    if sample:
        assert names[-2] == "gpt2_sample_kernel<false,false>" and "argmax_seg_kernel" not in names
    else:
        assert names[-3:-1] == ["argmax_seg_kernel", "argmax_final_kernel"]


@pytest.mark.parametrize("case", ["L1+63", "L23+41"])
def test_cases_with_Tmax_64_take_the_step_attention(case):
    names = _names(_plan(case))
    assert names.count("gpt2_attention_step_kernel") == N_LAYER and "gpt2_attention_kernel" not in names


def test_case_L23_42():
    plan = _plan("L23+42")
    names = _names(plan)
    assert _fused(plan) and "gpt2_attention_step_kernel" not in names
    at = [i for i, n in enumerate(names) if n == "gpt2_attention_kernel"]
    assert len(at) == N_LAYER
    for i in at:        # the qkv product's slices are summed by launch_gpt2_reduce in front of the general kernel
        assert names[i - 1] == "splitk_reduce_kernel" and names[i - 2].startswith("gemm_f32_stream_kernel") and plan[i - 2][1][1] > 1


def test_cases_P1_and_P63_differ_in_the_row_blocks_only():
    p1, p63 = _plan("P1"), _plan("P63")
    assert _fused(p1) and _tail(p1)
    assert [(n, b) for n, _, b in p1] == [(n, b) for n, _, b in p63] and _products(p1) == _products(p63)
    for (name, g1, _), (_, g63, _) in zip(p1, p63):
        if name.startswith("gemm_f32_stream_kernel") or name == "gpt2_head_kernel":
            assert g1 == g63, name          # column blocks x slices: no row dimension
        else:
            assert g1 != g63, name          # one workgroup per row (finalize, pick) or per four (sequence, head) pairs


SMALL = dict(D=768, V=50257, n_layer=12, Tmax=23 + 30)


@pytest.mark.parametrize("sample", [False, True])
def test_gpt2_small_step_launch_by_launch(sample):
    """GPT-2 small, 64 rows, 23 + 30 tokens: 74 launches per step, six per layer and the head with its tail."""
    plan = ops.host_gpt2_step_plan(64, SMALL["D"], SMALL["V"], SMALL["n_layer"], SMALL["Tmax"], sample=sample, n_cu=N_CU)
    layer = [("gemm_f32_stream_kernel<4,true,true>", (72, 3, 1), (512, 1, 1)),          # qkv: S = 3, NK = 4, 216 workgroups
             ("gpt2_attention_step_kernel", (64 * 12 // 4, 1, 1), (256, 1, 1)),
             ("gemm_f32_rowblk_kernel<12,false,true>", (24, 2, 1), (768, 1, 1)),        # attention output, complete
             ("gemm_f32_rowblk_kernel<12,true,true>", (96, 2, 1), (768, 1, 1)),         # MLP first, complete
             ("gemm_f32_stream_kernel<6,false,true>", (24, 8, 1), (768, 1, 1)),         # MLP second: S = 8, NK = 6, 192 workgroups
             ("gpt2_finalize_kernel", (64, 1, 1), (256, 1, 1))]
    head = [("gpt2_head_kernel", ((50257 + 31) // 32 // 4 + 1, 1, 1), (256, 1, 1)),
            ("gpt2_sample_kernel<true,true>" if sample else "gpt2_pick_embed_kernel", (64, 1, 1), (256, 1, 1))]
    assert len(plan) == 74
    assert plan == layer * 12 + head


def test_step_split_rule_reaches_every_split_at_256_cus():
    """test_gpu_gpt2_ops.test_step_gemm_reaches_every_split without the device: the same shapes at M = 33, the chooser asked with 256 CUs."""
    seen = {}
    for N, K in [(32, 64), (4096, 768), (2304, 768), (4096, 1024), (768, 768), (768, 3072), (1024, 4096)]:
        S, NK = ops.host_gpt2_gemm_choice(33, N, K, n_cu=N_CU)
        assert S >= 1 and K % (S * NK * 64) == 0
        seen.setdefault(S, []).append((N, K))
    assert {1, 2, 3, 4} <= set(seen) and max(seen) > 4, "splits reached: %r" % seen


def test_gpt2_small_products_do_not_depend_on_the_row_count():
    """What test_engine_gpt2_decode_rows_do_not_depend_on_the_launch relies on, at the real size: 8 rows and 64 rows take the same kernels
    with the same (S, NK); only the row-block dimension of a grid may differ."""
    p8, p64 = (ops.host_gpt2_step_plan(P, SMALL["D"], SMALL["V"], SMALL["n_layer"], SMALL["Tmax"], n_cu=N_CU) for P in (8, 64))
    assert [(n, b) for n, _, b in p8] == [(n, b) for n, _, b in p64]
    assert _products(p8) == _products(p64) and len(_products(p8)) == 4 * 12
    for (name, g8, _), (_, g64, _) in zip(p8, p64):
        if name.startswith("gemm_f32_stream_kernel"):
            assert g8 == g64
        elif name.startswith("gemm_f32_rowblk_kernel"):
            assert g8[0] == g64[0] and (g8[1], g64[1]) == (1, 2)
