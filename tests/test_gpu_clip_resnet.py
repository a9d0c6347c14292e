"""CLIP's ResNet image towers (RN50, RN101) on the GPU: every new kernel through its diagnostic op against the float64 references of
tests/clip_resnet_ref.py, whole towers through Engine.encode_image, and the fitness pass / search surface on top.

Bars are the project's own: 5e-3 * max|ref| on CLIP features, 1e-3 relative on the similarity.  The op-level tests compare with the float64
references of tests/tower_ops_ref.py under its error bound per element (derived from the kernels' own roundings) and assert the kernel symbol
the launcher reports; tests/test_gpu_tower_ops.py runs every instance at its smallest shapes.  References are float64, computed from the
fp16-rounded operands.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_resnet_ref as R
import tower_ops_ref as T
import glass_models as M
from clip_glass_amd import ops, synth
from clip_glass_amd.engine import Engine
from clip_glass_amd.generator import CLIP_PREPROCESS
from oracle import fitness_ref
from util import check, check_bound, check_logits, diag

pytestmark = pytest.mark.gpu
h16 = R.h16
MINI = R.TOWER_CASES["mini64"][:4]


def _bn(seed, C, gain=1.0):
    """A non-trivial BatchNorm as the scale / shift pair the engine keeps."""
    sd = {"p.weight": gain * synth.normal(seed, "g", (C,), 0.1, 1.0), "p.bias": synth.normal(seed, "b", (C,), 0.1),
          "p.running_mean": synth.normal(seed, "m", (C,), 0.2), "p.running_var": 0.4 + 1.2 * np.abs(np.tanh(synth.normal(seed, "v", (C,))))}
    a, s = R.bn_affine(sd, "p")
    return a.astype(np.float32), s.astype(np.float32)


def _w(seed, cout, cin, ks):
    return h16(synth.normal(seed, "w", (cout, cin, ks, ks), (2.0 / (cin * ks * ks)) ** 0.5))


# ---- op level ------------------------------------------------------------------------------------------------------------------------
def test_avgpool_odd_output_side():
    x = h16(synth.normal(30, "x", (2, 6, 6, 64)))
    got = ops.rn_avgpool(x)
    assert got.shape == (2, 3, 3, 64) and ops.last_kernel() == "rn_avgpool2_kernel"
    check_bound("rn avgpool 6x6 -> 3x3", got, *T.avgpool_ref(x))


@pytest.mark.parametrize("S", [64, 96])
def test_stem_conv1(S):
    """3 -> 32 channels, stride 2, read through the 32-pixel patch operand (2 x 2 and 3 x 3 patches); all four borders are compared."""
    img = h16(synth.normal(31, "img%d" % S, (2, 3, S, S)))
    w = _w(31, 32, 3, 3)
    a, s = _bn(31, 32)
    got = ops.rn_stem_conv1(img, w, a, s)
    ref, tol = T.conv_bn_ref(img.transpose(0, 2, 3, 1), w, a, s, stride=2, mfma=False)
    assert got.shape == ref.shape == (2, S // 2, S // 2, 32) and ops.last_kernel() == "rn_stem_conv1_kernel"
    check_bound("rn stem conv1 %d px" % S, got, ref, tol)
    for name, sl in (("top", np.s_[:, 0]), ("bottom", np.s_[:, -1]), ("left", np.s_[:, :, 0]), ("right", np.s_[:, :, -1])):
        check_bound("rn stem conv1 %d px %s border" % (S, name), got[sl], ref[sl], tol[sl])


@pytest.mark.parametrize("B,H", [(2, 7), (3, 2)])                   # M = 98 (not a tile multiple) and M = 12 (below 64: padded rows)
@pytest.mark.parametrize("K,N", [(64, 64), (256, 64), (64, 192), (256, 192)])      # N = 192: no multiple of 128, so three 64-wide n tiles (launch_gemm_tiled)
@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (True, False), (False, False)])
def test_conv1x1_bn(B, H, K, N, res, relu):
    x = h16(synth.normal(32, "x", (B, H, H, K)))
    w = _w(32, N, K, 1)
    a, s = _bn(32, N, 0.5)
    r = h16(synth.normal(32, "r", (B, H, H, N))) if res else None
    got = ops.rn_conv_bn(x, w, a, s, res=r, relu=relu)
    assert ops.last_kernel() == T.G64
    check_bound("rn 1x1 M%d K%d N%d res%d relu%d" % (B * H * H, K, N, res, relu), got, *T.conv_bn_ref(x, w, a, s, res=r, relu=relu))


@pytest.mark.parametrize("KS,C", [(1, 128), (3, 128)])
def test_conv_bn_128_wide_tiles(KS, C):
    """One image of 32 x 32 pixels: 1024 rows per candidate, where the launcher's fill rule picks the 128-wide n tile (the instance the
    full-size tower's early stages run on) — asserted through the symbol it reports."""
    x = h16(synth.normal(37, "x", (1, 32, 32, C)))
    w = _w(37, C, C, KS)
    a, s = _bn(37, C)
    got = ops.rn_conv_bn(x, w, a, s)
    assert ops.last_kernel() == (T.G128 if KS == 1 else T.T128)
    check_bound("rn %dx%d 128-wide tile" % (KS, KS), got, *T.conv_bn_ref(x, w, a, s))


def test_residual_is_added_before_the_relu():
    """Pre-activation sum negative where the residual alone is positive: relu(v + r) = 0 there, relu(v) + r = r."""
    B, H, K, N = 2, 7, 64, 64
    x = np.abs(h16(synth.normal(33, "x", (B, H, H, K))))
    w = -np.abs(_w(33, N, K, 1))                                     # every product negative
    a, s = np.ones(N, np.float32), np.zeros(N, np.float32)
    r = np.full((B, H, H, N), 0.25, np.float32)
    ref = R.conv_bn(x, w, a, s, res=r, relu=True)
    v = R.conv_bn(x, w, a, s, relu=False)
    assert (v + r < 0).mean() > 0.9 and (ref == 0).mean() > 0.9      # the case is what it claims to be
    got = ops.rn_conv_bn(x, w, a, s, res=r, relu=True)
    assert ops.last_kernel() == T.G64
    check_bound("rn 1x1 add-then-relu", got, *T.conv_bn_ref(x, w, a, s, res=r, relu=True))
    assert (got[v + r < -1e-2] == 0).all()


@pytest.mark.parametrize("B,H,C", [(2, 7, 64), (2, 14, 64), (2, 4, 128)])
def test_conv3x3_bn_relu_gather(B, H, C):
    x = h16(synth.normal(34, "x", (B, H, H, C)))
    w = _w(34, C, C, 3)
    a, s = _bn(34, C)
    got = ops.rn_conv_bn(x, w, a, s)
    assert ops.last_kernel() == T.T64
    check_bound("rn 3x3 gather %dx%d C%d" % (H, H, C), got, *T.conv_bn_ref(x, w, a, s))


@pytest.mark.parametrize("B,H,Cin,Cout", [(2, 32, 32, 32), (2, 48, 32, 64), (3, 7, 32, 64)])      # the stem's conv2 / conv3; 147 rows: a partial wave
def test_stem_conv3x3(B, H, Cin, Cout):
    x = h16(synth.normal(35, "x", (B, H, H, Cin)))
    w = _w(35, Cout, Cin, 3)
    a, s = _bn(35, Cout)
    got = ops.rn_conv_bn(x, w, a, s, form=1)
    assert ops.last_kernel() == "rn_conv3x3_kernel<%d>" % (2 if Cout % 64 == 0 else 1)
    check_bound("rn stem 3x3 %dx%d %d->%d" % (H, H, Cin, Cout), got, *T.conv_bn_ref(x, w, a, s))


def test_attnpool_tokens():
    B, HW, C = 2, 9, 128
    x = h16(synth.normal(36, "x", (B, HW, C)))
    pos = synth.normal(36, "pos", (HW + 1, C), 0.3)
    got = ops.rn_tokens(x, pos)
    ref = R.attnpool_tokens(x, pos)
    assert got.shape == (B, HW + 1, C) and ops.last_kernel() == "rn_attnpool_tokens_kernel"
    check_bound("rn tokens", got, *T.tokens_ref(x, pos))
    check("rn tokens", got, ref, 1e-3)
    check("rn tokens mean row", got[:, 0], x.astype(np.float64).mean(axis=1) + pos[0], 1e-3)
    check("rn tokens positional add", got[:, 1:] - x, np.broadcast_to(pos[1:], (B, HW, C)), 1e-3, atol=2.0 ** -9)      # (+ the rounding of a sum near 4)


# ---- whole towers through Engine.encode_image ------------------------------------------------------------------------------------
def _tower_engine(case, max_pop, sd=None):
    layers, width, res, embed, _ = R.TOWER_CASES[case]
    e = Engine([], latent_size=4, mapping_layers=0, batch_size=1, use_discriminator=False, n_obj=1, max_pop=max_pop,
               clip_resnet=(layers, width, res, embed), noise_mode=0)
    e.load_state(sd if sd is not None else R.tower_state(case))
    e.finalize()
    return e


@pytest.mark.parametrize("case", ["mini64", "mini96", "nodown64"])
def test_mini_towers(case):
    P = R.TOWER_CASES[case][4]
    img, ref = R.tower_images(case), R.tower_reference(case)
    e = _tower_engine(case, P)
    got = e.encode_image(img)
    one = e.encode_image(img[:1])                                   # P 1: the img2txt shape (4 rows at layer4)
    e.close()
    check("rn %s features" % case, got, ref, R.FEATURE_BAR)
    check("rn %s features, one image" % case, one, ref[:1], R.FEATURE_BAR)


def test_full_size_rn50():
    img, ref = R.tower_images("rn50"), R.tower_reference("rn50")
    e = _tower_engine("rn50", 4)
    got = e.encode_image(img)
    again = e.encode_image(img[2:])
    e.close()
    check("RN50 features", got, ref, R.FEATURE_BAR)
    np.testing.assert_array_equal(again, got[2:])                   # a row does not depend on what it is batched with


# ---- end to end: mini StyleGAN2 + the res-64 mini tower ------------------------------------------------------------------------------
def _gan_state(seed=0):
    c = M.CONFIGS["mini"]
    sd = synth.make_state(synth.stylegan2_g_spec(c["channels"], c["latent"], c["mapping"]), seed)
    sd.update(synth.make_state(synth.stylegan2_d_spec(c["channels"]), seed))
    sd.update(R.tower_state("mini64"))
    return sd


def _gan_engine(sd, P, bs, chunk, preprocess=None):
    c = M.CONFIGS["mini"]
    kw = {}
    if preprocess is not None:
        kw.update(clip_resize=CLIP_PREPROCESS[preprocess][0], clip_normalize=CLIP_PREPROCESS[preprocess][1])
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=bs, use_discriminator=True, n_obj=2,
               max_pop=P, chunk=chunk, clip_resnet=MINI, noise_mode=2, **kw)
    e.load_state(sd)
    e.finalize()
    return e


def _compare(tag, e, P, x, planes, feats, target, dis_o):
    sim_o = torch.cosine_similarity(torch.tensor(feats), torch.tensor(target, dtype=torch.float64)[None]).numpy()
    e.set_target(target)
    Fe = e.evaluate(x, noise=planes)
    det = e.details(P)
    check(tag + " clip features", det["features"], feats, R.FEATURE_BAR)
    rel = np.abs(det["sim"] - sim_o) / np.abs(sim_o)
    diag("[e2e] %s sim range [%.3f, %.3f] max rel err %.3e" % (tag, sim_o.min(), sim_o.max(), rel.max()))
    assert rel.max() < 1e-3, "CLIP similarity relative error %.3e > 1e-3" % rel.max()
    np.testing.assert_allclose(Fe[:, 0], -det["sim"], rtol=0, atol=1e-7)
    check_logits(tag + " hinge", Fe[:, 1], np.maximum(1 - dis_o, 0), case="mini")
    return Fe


def test_end_to_end_whole_and_chunked():
    c, P, bs = M.CONFIGS["mini"], 8, 4
    sd = _gan_state()
    tsd = {k: torch.as_tensor(v) for k, v in sd.items()}
    x = synth.latents(3, P, c["latent"])
    planes = M.noise_planes("mini", 31, 0, P // bs)
    with torch.no_grad():
        img = fitness_ref.generate(tsd, x, bs, lambda i: planes[i])
        dis_o = fitness_ref.discriminate(tsd, img, bs).numpy()[:, 0]
        pre = fitness_ref.resize224(img, MINI[2]).numpy()           # generator.py:45, to the tower's 64 px
    feats = R.forward(sd, h16(pre))
    target = M.make_target(feats)
    rows = []
    for chunk in (8, 4):
        e = _gan_engine(sd, P, bs, chunk)
        rows.append(_compare("mini + RN mini64 P%d chunk%d" % (P, chunk), e, P, x, planes, feats, target, dis_o))
        e.close()
    np.testing.assert_array_equal(rows[0], rows[1])                 # whole population == two chunks, bit for bit


def test_end_to_end_clip_preprocess():
    """clip_preprocess="clip": the engine's own images -> the torch definition of the transform -> the float64 tower."""
    c, P, bs = M.CONFIGS["mini"], 8, 4
    sd = _gan_state()
    tsd = {k: torch.as_tensor(v) for k, v in sd.items()}
    x = synth.latents(3, P, c["latent"])
    planes = M.noise_planes("mini", 31, 0, P // bs)
    e = _gan_engine(sd, P, bs, 0, preprocess="clip")
    img = torch.tensor(e.generate(x, noise=planes)).double()
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073], dtype=torch.float64)[None, :, None, None]      # clip/clip.py:73
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711], dtype=torch.float64)[None, :, None, None]
    pre = (F.interpolate(img, (MINI[2], MINI[2]), mode="bicubic", align_corners=False, antialias=True).clamp(0, 1) - mean) / std
    feats = R.forward(sd, h16(pre.numpy()))
    with torch.no_grad():
        dis_o = fitness_ref.discriminate(tsd, fitness_ref.generate(tsd, x, bs, lambda i: planes[i]), bs).numpy()[:, 0]
    _compare("mini + RN mini64 clip preprocess", e, P, x, planes, feats, M.make_target(feats), dis_o)
    e.close()


# ---- the search surface --------------------------------------------------------------------------------------------------------------
def test_generation_problem_with_resnet_geometry():
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.problem import GenerationProblem
    c = M.CONFIGS["mini"]
    cfg = types.SimpleNamespace(config="StyleGAN2_ffhq_d", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("StyleGAN2_ffhq_d"))
    target = M.make_target(synth.normal(25, "t", (8, MINI[3])))
    vars(cfg).update(weights="synthetic:0", clip_weights="synthetic:0", clip_resnet_geometry=MINI, channels=c["channels"], dim_z=c["latent"],
                     mapping_layers=c["mapping"], target_features=target, noise_mode=1, noise_seed=42,
                     problem_args=dict(cfg.problem_args, n_var=c["latent"], n_constr=c["latent"]))
    prob = GenerationProblem(cfg)
    gen = prob.generator
    assert gen.clip_resnet == MINI and gen.clip_geometry == (64, 4, 32, 32, 64, 64)
    ec = gen.engine.cfg
    assert ec.clip_arch == 1 and list(ec.clip_rn_layers) == [1, 1, 1, 1]
    assert (ec.clip_width, ec.clip_layers, ec.clip_heads, ec.clip_patch, ec.clip_res, ec.clip_embed) == (64, 4, 32, 32, 64, 64)
    out = {}
    prob._evaluate(synth.latents(1, 8, c["latent"]), out)
    assert out["F"].shape == (8, 2) and out["F"].dtype == np.float32 and np.isfinite(out["F"]).all()
    assert (np.abs(out["F"][:, 0]) <= 1 + 1e-6).all() and np.ptp(out["F"][:, 0]) > 0        # a cosine, and not a constant
    gen.engine.close()


def test_img2txt_generator_with_resnet_tower(tmp_path):
    """The img2txt branch: a text-only engine (no GAN) with the ResNet image tower and the text tower; its encode_image is the target's."""
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.generator import Generator
    ej, vb, cb = synth.write_bpe_assets(str(tmp_path), gpt2_vocab=600, clip_vocab=700)
    cfg = types.SimpleNamespace(config="GPT2", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("GPT2"))
    vars(cfg).update(weights="synthetic:2", clip_weights="synthetic:11", clip_resnet_geometry=MINI,
                     clip_text_geometry=dict(width=64, layers=2, vocab=700), encoder_size=600, gpt2_geometry=dict(n_embd=128, n_layer=2),
                     encoder=ej, vocab=vb, bpe_path=cb, target_features=synth.normal(3, "imgfeat", (MINI[3],)), pop_size=4, max_pop=4)
    gen = Generator(cfg)
    assert gen.clip_resnet == MINI and gen.engine.cfg.clip_arch == 1 and gen.engine.cfg.n_blocks == 0
    got = gen.engine.encode_image(R.tower_images("mini64")[:1])      # synthetic:11 is tower_state's seed: the same weights
    check("img2txt RN mini64 target feature", got, R.tower_reference("mini64")[:1], R.FEATURE_BAR)
    sims = gen.clip_similarity_texts(["the picture of", "of the"])
    assert sims.shape == (2,) and np.isfinite(sims).all() and np.ptp(sims) > 0
    gen.engine.close()
