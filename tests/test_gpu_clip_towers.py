"""The larger CLIP image towers (ViT-B/16, ViT-L/14, ViT-L/14@336) on the GPU: the streaming attention kernel through the diagnostic
op, the padded patch embedding, full-size towers through the C ABI against the oracle, and the search surface on top.

Bars are the project's own: 2e-3 * max|ref| for the attention op (test_gpu_ops.test_layernorm_attention), 1e-3 for the resize,
5e-3 * max|ref| on CLIP features and 1e-3 relative on the similarity (README parity table)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clip_glass_amd import ops, synth
from clip_glass_amd.engine import Engine
from oracle import clip_ref, fitness_ref
import glass_models as M
from util import check, check_logits, diag

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VIT_B16 = (768, 12, 12, 16, 224, 512)
VIT_L14 = (1024, 24, 16, 14, 224, 768)
VIT_L14_336 = (1024, 24, 16, 14, 336, 768)


def _t(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


def h16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def _attention_ref(qkv, n_img, L, heads, causal):
    """The torch formula of test_gpu_ops.test_layernorm_attention."""
    t = torch.tensor(qkv).view(n_img, L, 3, heads, 64)
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
    a = (q * 0.125) @ k.transpose(-1, -2)
    if causal:
        a = a + torch.full((L, L), float("-inf")).triu_(1)
    return (torch.softmax(a, -1) @ v).transpose(1, 2).reshape(n_img * L, heads * 64).numpy()


# ---- the streaming kernel (every L > 96) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,causal,n_img,heads", [
    (97, False, 3, 2),       # first length past the whole-sequence kernels: pins the switch-over
    (128, False, 3, 2), (197, False, 3, 2), (200, False, 3, 2), (257, False, 3, 2), (577, False, 3, 2),
    (130, True, 3, 2), (257, True, 3, 2),
    (197, False, 3, 1),      # an odd number of (image, head) pairs
])
def test_streaming_attention(L, causal, n_img, heads):
    qkv = h16(synth.normal(21, "qkv%d_%d" % (L, heads), (n_img * L, 3 * heads * 64)))
    got = ops.attention(qkv, n_img, L, heads, causal)
    check("attention L%d causal%d pairs%d" % (L, causal, n_img * heads), got, _attention_ref(qkv, n_img, L, heads, causal), 2e-3)


def test_attention_op_bounds():
    qkv = np.zeros((4097, 3 * 64), np.float32)
    with pytest.raises(RuntimeError, match="L <= 4096"):
        ops.attention(qkv, 1, 4097, 1)


# ---- L <= 96 still runs the kernels it ran: bit-identical to the build before the streaming kernel existed -------------------
SHORT_CASES = [(50, False), (77, True)]
SHORT_N_IMG, SHORT_HEADS = 3, 2
SHORT_GOLDEN = os.path.join(GOLDEN, "attention_short_dispatch.npz")      # tests/golden/record_attention_dispatch.py


def short_case_input(L):
    return h16(synth.normal(22, "short_qkv%d" % L, (SHORT_N_IMG * L, 3 * SHORT_HEADS * 64)))


@pytest.mark.parametrize("L,causal", SHORT_CASES)
def test_short_sequence_dispatch_is_bit_identical(L, causal):
    want = np.load(SHORT_GOLDEN)["L%d_causal%d" % (L, int(causal))]
    got = ops.attention(short_case_input(L), SHORT_N_IMG, L, SHORT_HEADS, causal)
    assert want.dtype == np.float16 and got.shape == want.shape
    np.testing.assert_array_equal(got, want.astype(np.float32))


# ---- patch 14: 3 * 14 * 14 = 588 columns, dense in the op's output -----------------------------------------------------------
def test_resize_patches_patch14():
    B, R, S, ps = 2, 256, 224, 14
    y = synth.normal(23, "y", (B, 3, R, R), 0.8)
    img = ((torch.tensor(y) + 1) / 2).clip(0, 1)
    ref = F.interpolate(img, size=(S, S), mode="bilinear", align_corners=False)
    G = S // ps
    ref = ref.view(B, 3, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, 3 * ps * ps).numpy()
    got = ops.resize(y, S, ps)
    assert got.shape == (B * G * G, 588)
    check("resize %d->%d patch 14" % (R, S), got, ref, 1e-3)


# ---- full-size towers through the C ABI --------------------------------------------------------------------------------------
def _clip_engine(geom, sd, max_pop=4):
    e = Engine([], latent_size=4, mapping_layers=0, batch_size=1, use_discriminator=False, n_obj=1, max_pop=max_pop, clip=geom,
               noise_mode=0)
    e.load_state(sd)
    e.finalize()
    return e


@pytest.mark.parametrize("name,geom", [("ViT-B/16", VIT_B16), ("ViT-L/14", VIT_L14), ("ViT-L/14@336", VIT_L14_336)])
def test_full_size_image_tower(name, geom):
    w, layers, heads, patch, res, embed = geom
    sd = synth.make_state(synth.clip_visual_spec(w, layers, patch, res, embed), 0)
    img = synth.normal(24, "img%d" % res, (4, 3, res, res))              # preprocessed images are ~unit-variance
    e = _clip_engine(geom, sd)
    got = e.encode_image(img)
    again = e.encode_image(img[2:])
    e.close()
    with torch.no_grad():
        ref = clip_ref.encode_image(_t(sd), torch.tensor(img)).numpy()
    check("%s features" % name, got, ref, 5e-3)
    np.testing.assert_array_equal(again, got[2:])                         # a row does not depend on what it is batched with


def test_vit_l14_text_tower():
    """ViT-L/14's text tower (width 768, 12 heads, 12 layers, embed 768) beside a 1-layer cut of its image tower."""
    geom = (1024, 1, 16, 14, 224, 768)
    sd = synth.make_state(synth.clip_visual_spec(geom[0], geom[1], geom[3], geom[4], geom[5]), 0)
    sd.update(synth.make_state(synth.clip_text_spec(width=768, layers=12, out_dim=768), 0))
    g = dict(np.load(os.path.join(GOLDEN, "mini_problem.npz")))
    tokens = np.stack([g["tokens"], np.r_[g["tokens"][:5], 49407, np.zeros(71, np.int64)]]).astype(np.int64)
    e = _clip_engine(geom, sd)
    got = e.encode_text(tokens)
    e.close()
    with torch.no_grad():
        ref = clip_ref.encode_text(_t(sd), torch.tensor(tokens)).numpy()
    assert got.shape == (2, 768)
    check("ViT-L/14 text tower", got, ref, 5e-3)


# ---- end to end: mini StyleGAN2 + a full-size tower --------------------------------------------------------------------------
def _gan_state(geom, seed=0):
    c = M.CONFIGS["mini"]
    sd = synth.make_state(synth.stylegan2_g_spec(c["channels"], c["latent"], c["mapping"]), seed)
    sd.update(synth.make_state(synth.stylegan2_d_spec(c["channels"]), seed))
    sd.update(synth.make_state(synth.clip_visual_spec(geom[0], geom[1], geom[3], geom[4], geom[5]), seed))
    return sd


def _gan_engine(geom, sd, P, bs, chunk):
    c = M.CONFIGS["mini"]
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=bs, use_discriminator=True,
               n_obj=2, max_pop=P, chunk=chunk, clip=geom, noise_mode=2)
    e.load_state(sd)
    e.finalize()
    return e


def _end_to_end(name, geom, P, bs, chunks):
    c = M.CONFIGS["mini"]
    sd = _gan_state(geom)
    tsd = _t(sd)
    x = synth.latents(3, P, c["latent"])
    planes = M.noise_planes("mini", 31, 0, P // bs)
    detail = {}
    fitness_ref.evaluate(tsd, x, np.ones(geom[5], np.float32), bs, True, lambda i: planes[i], clip_size=geom[4], detail=detail)
    feats = detail["features"].numpy()
    target = M.make_target(feats)
    sim_o = torch.cosine_similarity(detail["features"], torch.tensor(target)[None]).numpy()
    dis_o = detail["dis"].numpy()[:, 0]
    rows = []
    for chunk in chunks:
        e = _gan_engine(geom, sd, P, bs, chunk)
        e.set_target(target)
        Fe = e.evaluate(x, noise=planes)
        det = e.details(P)
        e.close()
        tag = "mini + %s P%d chunk%d" % (name, P, chunk)
        check(tag + " clip features", det["features"], feats, 5e-3)
        rel = np.abs(det["sim"] - sim_o) / np.abs(sim_o)
        diag("[e2e] %s sim range [%.3f, %.3f] max rel err %.3e" % (tag, sim_o.min(), sim_o.max(), rel.max()))
        assert rel.max() < 1e-3, "CLIP similarity relative error %.3e > 1e-3" % rel.max()
        np.testing.assert_allclose(Fe[:, 0], -det["sim"], rtol=0, atol=1e-7)
        check_logits(tag + " hinge", Fe[:, 1], np.maximum(1 - dis_o, 0), case="mini")
        rows.append(Fe)
    for other in rows[1:]:
        np.testing.assert_array_equal(rows[0], other)      # whole population == two chunks, bit for bit


def test_end_to_end_vit_b16_whole_and_chunked():
    _end_to_end("ViT-B/16", VIT_B16, P=8, bs=4, chunks=(8, 4))


def test_end_to_end_vit_l14_padded_patch_gemm():
    _end_to_end("ViT-L/14", VIT_L14, P=4, bs=4, chunks=(4,))


# ---- the search surface ------------------------------------------------------------------------------------------------------
def test_generator_with_named_model():
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.problem import GenerationProblem
    c = M.CONFIGS["mini"]
    cfg = types.SimpleNamespace(config="StyleGAN2_ffhq_d", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("StyleGAN2_ffhq_d"))
    target = M.make_target(synth.normal(25, "t", (8, 512)))
    vars(cfg).update(weights="synthetic:0", clip_weights="synthetic:0", clip_model="ViT-B/16", channels=c["channels"], dim_z=c["latent"],
                     mapping_layers=c["mapping"], target_features=target, noise_mode=1, noise_seed=42,
                     problem_args=dict(cfg.problem_args, n_var=c["latent"], n_constr=c["latent"]))
    prob = GenerationProblem(cfg)
    gen = prob.generator
    assert gen.clip_geometry == VIT_B16
    ec = gen.engine.cfg
    assert (ec.clip_width, ec.clip_layers, ec.clip_heads, ec.clip_patch, ec.clip_res, ec.clip_embed) == VIT_B16
    out = {}
    prob._evaluate(synth.latents(1, 8, c["latent"]), out)
    assert out["F"].shape == (8, 2) and out["F"].dtype == np.float32 and np.isfinite(out["F"]).all()
    assert (np.abs(out["F"][:, 0]) <= 1 + 1e-6).all() and np.abs(out["F"][:, 0]).max() > 0      # a cosine, and not a constant zero
    gen.engine.close()
