"""Crop views on the device: view_patches_kernel against the torch definition (tests/clip_views_ref.py), the pass end to end against the
float64 oracle tower, the bitwise identities of the pass (one view, view 0, chunks, slices, stream modes), the boxes per generation, the
BigGAN and ResNet-tower paths, and the search driver."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import clip_resnet_ref as RN
import clip_views_ref as VR
import glass_models as M
from clip_glass_amd import ops, synth
from clip_glass_amd.engine import Engine
from oracle import clip_ref
from util import check, diag

pytestmark = pytest.mark.gpu

SEED, GEN, V = 7, 3, 4          # the boxes' seed (the engine's noise_seed), the generation most tests evaluate, the views


def _t(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


# ---- op level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("R,S,ps", [(32, 32, 8), (64, 32, 8), (256, 224, 14), (1024, 224, 32)])
def test_view_patches_op(R, S, ps, normalize):
    """Bar: the project's resize bar, 1e-3 * max|ref| (fp32 coordinates and blend, one fp16 rounding of the result).  The four boxes touch
    every edge between them: the whole image (s = R), a flipped s = 2 crop in the far corner, top-right, flipped bottom-left."""
    boxes = VR.edge_boxes(R)
    for B in ((2, 3) if R < 1024 else (2,)):
        y = synth.normal(23, "y%d" % B, (B, 3, R, R), 0.8)
        ref = VR.as_patch_rows(VR.torch_views(((torch.tensor(y).double() + 1) / 2).clip(0, 1), S, boxes, normalize), ps)
        got = ops.view_patches(y, S, ps, boxes, normalize)
        assert got.shape == ref.shape == (B * 4 * (S // ps) ** 2, 3 * ps * ps)
        check("views %d->%d ps%d norm%d B%d" % (R, S, ps, normalize, B), got, ref, 1e-3)


@pytest.mark.parametrize("R,S,ps", [(32, 32, 8), (64, 32, 8), (256, 224, 14), (1024, 224, 32)])
def test_whole_image_view_is_the_default_resize_bit_for_bit(R, S, ps):
    y = synth.normal(23, "y", (2, 3, R, R), 0.8)
    np.testing.assert_array_equal(ops.view_patches(y, S, ps, [(0, 0, R, 0)]), ops.resize(y, S, ps))
    np.testing.assert_array_equal(ops.view_patches(y, S, ps, [(0, 0, R, 0)], normalize=1), ops.preprocess(y, S, ps, 0, 1))


def test_op_refuses_a_box_outside_the_image():
    y = synth.normal(23, "y", (1, 3, 32, 32), 0.8)
    for box in [(1, 0, 32, 0), (0, 31, 2, 0), (-1, 0, 4, 0), (0, 0, 0, 0), (0, 0, 4, 2)]:
        with pytest.raises(RuntimeError, match="box"):
            ops.view_patches(y, 32, 8, [box])


# ---- engines -----------------------------------------------------------------------------------------------------------------
def _sg2_engine(name, sd, P, bs, views, chunk=0, use_d=False, **kw):
    c = M.CONFIGS[name]
    if "clip_resnet" not in kw:
        kw["clip"] = c["clip"]
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=bs, use_discriminator=use_d,
               n_obj=2 if use_d else 1, max_pop=P, chunk=chunk, noise_mode=2, noise_seed=SEED, clip_views=views, **kw)
    e.load_state(sd)
    e.finalize()
    return e


def _bg_engine(sd, P, bs, views):
    c = M.BIGGAN_CONFIGS["bg_mini"]
    e = Engine([], batch_size=bs, max_pop=P, clip=c["clip"], noise_seed=SEED, clip_views=views,
               biggan=dict(layers=c["layers"], attention_pos=c["attention_pos"], ch=c["ch"], z_dim=c["z_dim"],
                           num_classes=c["num_classes"], truncation=1.0))
    e.load_state(sd)
    e.finalize()
    return e


def _against_oracle(tag, e, P, x, S, encode, feature_bar, **run):
    """The engine's own images -> the torch definition of the views -> the oracle's image tower, against view_details() / details()."""
    img = e.generate(x, generation=GEN, **run)
    boxes = synth.clip_view_boxes(SEED, GEN, V, img.shape[-1], 500, True, False)
    views = VR.torch_views(img, S, boxes).reshape(P * V, 3, S, S)
    feats = np.asarray(encode(views), np.float64).reshape(P, V, -1)
    target = M.make_target(feats.mean(axis=1))
    tn = np.asarray(target, np.float64)
    sims_o = (feats @ tn) / np.maximum(np.linalg.norm(feats, axis=2) * np.linalg.norm(tn), 1e-8)
    mean_o = sims_o.mean(axis=1)
    diag("[views] %s oracle mean sim range [%.3f, %.3f]" % (tag, mean_o.min(), mean_o.max()))
    assert (np.abs(mean_o) > 0.1).all(), mean_o          # on the oracle's values alone: a relative bar needs a scale
    e.set_target(target)
    Fe = e.evaluate(x, generation=GEN, **run)
    vd, det = e.view_details(P), e.details(P)
    np.testing.assert_array_equal(vd["boxes"], boxes)
    check(tag + " view features", vd["features"], feats, feature_bar)
    rel_v = np.abs(vd["sims"] - sims_o) / np.abs(sims_o)
    rel_m = np.abs(det["sim"] - mean_o) / np.abs(mean_o)
    diag("[views] %s view sims max rel err %.3e, mean %.3e" % (tag, rel_v.max(), rel_m.max()))
    assert rel_v.max() < 1e-3 and rel_m.max() < 1e-3, (rel_v.max(), rel_m.max())
    np.testing.assert_array_equal(det["sim"], VR.mean_sims(vd["sims"]))       # the fixed-order fp32 mean of the engine's own cosines
    np.testing.assert_array_equal(det["features"], vd["features"][:, 0])
    np.testing.assert_allclose(Fe[:, 0], -det["sim"], rtol=0, atol=1e-7)
    return target, Fe


@functools.lru_cache(maxsize=None)
def _mid():
    P, bs = 8, 4
    sd = M.make_state("mid", 0, with_d=False)
    x = synth.latents(3, P, M.CONFIGS["mid"]["latent"])
    planes = M.noise_planes("mid", 31, 0, P // bs)
    target = M.make_target(synth.normal(25, "t", (P, M.CONFIGS["mid"]["clip"][5])))
    return P, bs, sd, x, planes, target


def _vit_encode(sd):
    tsd = _t(sd)

    def encode(views):
        with torch.no_grad():
            return clip_ref.encode_image(tsd, views.float()).numpy()
    return encode


def test_end_to_end_mid():
    P, bs, sd, x, planes, _ = _mid()
    e = _sg2_engine("mid", sd, P, bs, V)
    _against_oracle("mid V4", e, P, x, M.CONFIGS["mid"]["clip"][4], _vit_encode(sd), 5e-3, noise=planes)
    e.close()


def test_end_to_end_biggan_mini():
    P, bs = 8, 4
    c = M.BIGGAN_CONFIGS["bg_mini"]
    sd = M.make_biggan_state("bg_mini", 0)
    x = synth.biggan_population(1, P, c["z_dim"], c["num_classes"])
    e = _bg_engine(sd, P, bs, V)
    _against_oracle("bg_mini V4", e, P, x, c["clip"][4], _vit_encode(sd), 5e-3)
    e.close()


def test_end_to_end_resnet_tower():
    """mini64 behind "mini": 32 px images up-sampled to the tower's 64 px, every crop smaller than the output."""
    P, bs = 8, 4
    c, mini = M.CONFIGS["mini"], RN.TOWER_CASES["mini64"][:4]
    sd = synth.make_state(synth.stylegan2_g_spec(c["channels"], c["latent"], c["mapping"]), 0)
    sd.update(RN.tower_state("mini64"))
    x = synth.latents(3, P, c["latent"])
    planes = M.noise_planes("mini", 31, 0, P // bs)
    e = _sg2_engine("mini", sd, P, bs, V, clip_resnet=mini)
    _against_oracle("mini + RN mini64 V4", e, P, x, mini[2], lambda views: RN.forward(sd, RN.h16(views.numpy())), RN.FEATURE_BAR, noise=planes)
    e.close()


# ---- identities, bit for bit ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid_views_off():
    P, bs, sd, x, planes, target = _mid()
    e = _sg2_engine("mid", sd, P, bs, 0)
    e.set_target(target)
    F0 = e.evaluate(x, generation=GEN, noise=planes)
    det = e.details(P)
    e.close()
    return F0, det


def test_one_view_is_the_default_pass():
    P, bs, sd, x, planes, target = _mid()
    F0, det0 = _mid_views_off()
    e = _sg2_engine("mid", sd, P, bs, 1)
    e.set_target(target)
    F1 = e.evaluate(x, generation=GEN, noise=planes)
    vd, det = e.view_details(P), e.details(P)
    e.close()
    np.testing.assert_array_equal(F1, F0)
    np.testing.assert_array_equal(vd["boxes"], [(0, 0, 64, 0)])
    np.testing.assert_array_equal(vd["sims"][:, 0], det0["sim"])
    np.testing.assert_array_equal(det["features"], det0["features"])


def test_view_zero_is_the_default_pass_and_chunks_and_slices_agree():
    P, bs, sd, x, planes, target = _mid()
    F0, det0 = _mid_views_off()
    rows = {}
    for chunk in (8, 4):
        e = _sg2_engine("mid", sd, P, bs, V, chunk=chunk)
        e.set_target(target)
        rows[chunk] = e.evaluate(x, generation=GEN, noise=planes)
        vd, det = e.view_details(P), e.details(P)
        np.testing.assert_array_equal(vd["sims"][:, 0], det0["sim"])
        np.testing.assert_array_equal(det["features"], det0["features"])
        np.testing.assert_array_equal(vd["features"][:, 0], det0["features"])
        if chunk == 8:      # the population as two 4-row calls: the boxes do not depend on the slice
            halves = [e.evaluate(x[:4], generation=GEN, first_minibatch=0, noise=planes[:1]),
                      e.evaluate(x[4:], generation=GEN, first_minibatch=1, noise=planes[1:])]
        e.close()
    assert not np.array_equal(rows[8], F0)          # the crops count
    np.testing.assert_array_equal(rows[8], rows[4])
    np.testing.assert_array_equal(np.concatenate(halves), rows[8])


def test_stream_modes_agree_and_the_discriminator_sees_the_whole_image():
    P, bs = 8, 4
    sd = M.make_state("mini", 0)
    x = synth.latents(3, P, M.CONFIGS["mini"]["latent"])
    planes = M.noise_planes("mini", 31, 0, P // bs)
    target = M.make_target(synth.normal(25, "t", (P, M.CONFIGS["mini"]["clip"][5])))
    e0 = _sg2_engine("mini", sd, P, bs, 0, use_d=True)
    e0.set_target(target)
    F0 = e0.evaluate(x, generation=GEN, noise=planes)
    e0.close()
    e = _sg2_engine("mini", sd, P, bs, V, use_d=True)
    e.set_target(target)
    rows = []
    for mode in (0, 1, 2):
        e.set_overlap(mode)
        rows.append(e.evaluate(x, generation=GEN, noise=planes))
    e.close()
    np.testing.assert_array_equal(rows[1], rows[0])
    np.testing.assert_array_equal(rows[2], rows[0])
    np.testing.assert_array_equal(rows[0][:, 1], F0[:, 1])
    assert rows[0].shape == (P, 2) and not np.array_equal(rows[0][:, 0], F0[:, 0])


# ---- generations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True])
def test_boxes_follow_the_generation(fixed):
    P, bs, sd, x, planes, target = _mid()
    e = _sg2_engine("mid", sd, P, bs, V, clip_view_fixed=fixed, clip_view_min=0.25)
    e.set_target(target)
    seen = []
    for g in (0, 5):
        e.evaluate(x, generation=g, noise=planes)
        b = e.view_details(P)["boxes"]
        np.testing.assert_array_equal(b, synth.clip_view_boxes(SEED, g, V, 64, 250, True, fixed))
        seen.append(b)
    assert np.array_equal(seen[0], seen[1]) == fixed


def test_setter_call_order_and_refusals():
    P, bs, sd, _, _, _ = _mid()
    e = _sg2_engine("mid", sd, P, bs, 0)
    assert e.lib.glass_engine_set_clip_views(e._h, 4, 500, 1, 0) == -2 and "finalize" in e.lib.glass_last_error().decode()
    with pytest.raises(RuntimeError, match="off"):
        e.view_details(P)
    e.close()
    c = M.CONFIGS["mid"]
    for kw, word in [(dict(clip_views=17), "views"), (dict(clip_views=4, clip_view_min=0.0), "per mille"),
                     (dict(clip_views=4, clip_resize=2), "clip_resize")]:
        with pytest.raises(RuntimeError, match=word):
            Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], use_discriminator=False, n_obj=1, clip=c["clip"], **kw)
    with pytest.raises(RuntimeError, match="no generator"):
        Engine([], latent_size=4, mapping_layers=0, batch_size=1, use_discriminator=False, n_obj=1, clip=c["clip"], noise_mode=0, clip_views=4)


# ---- the search driver ---------------------------------------------------------------------------------------------------------
def _driver_extra():
    c = M.CONFIGS["mini"]
    return dict(channels=c["channels"], dim_z=c["latent"], mapping_layers=c["mapping"], clip_geometry=c["clip"],
                target_features=M.make_target(synth.normal(25, "t", (8, c["clip"][5]))), noise_mode=1, noise_seed=42,
                problem_args=dict(n_var=c["latent"], n_obj=2, n_constr=c["latent"], xl=-10, xu=10))


def test_generation_problem_with_views():
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.problem import GenerationProblem
    c = M.CONFIGS["mini"]
    cfg = types.SimpleNamespace(config="StyleGAN2_ffhq_d", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("StyleGAN2_ffhq_d"))
    vars(cfg).update(weights="synthetic:0", clip_weights="synthetic:0", clip_views=4, **_driver_extra())
    prob = GenerationProblem(cfg)
    gen = prob.generator
    assert gen.augmentation["clip_views"] == 4 and gen.engine.clip_views == 4
    x = synth.latents(1, 8, c["latent"])
    seen = []
    for g in range(2):
        out = {}
        prob._evaluate(x, out)
        assert out["F"].shape == (8, 2) and out["F"].dtype == np.float32 and np.isfinite(out["F"]).all()
        vd = gen.engine.view_details(8)
        np.testing.assert_array_equal(vd["boxes"], synth.clip_view_boxes(42, g, 4, 32, 500, True, False))
        np.testing.assert_allclose(out["F"][:, 0], -VR.mean_sims(vd["sims"]), rtol=0, atol=1e-7)
        seen.append(out["F"])
    assert not np.array_equal(seen[0][:, 0], seen[1][:, 0])        # new crops (and new noise) in the second generation
    gen.engine.close()


def test_run_main_with_views(tmp_path):
    from clip_glass_amd import run
    argv = ["--config", "StyleGAN2_ffhq_d", "--generations", "2", "--save-each", "2", "--tmp-folder", str(tmp_path),
            "--weights", "synthetic:0", "--clip-weights", "synthetic:0", "--pop-size", "8", "--clip-views", "2"]
    res = run.main(argv, extra_config=_driver_extra())
    assert np.atleast_2d(res.F).shape[1] == 2
    for f in ("genetic-it-final.jpg", "genetic_result", "ls_result", "output.jpg"):
        assert os.path.getsize(os.path.join(str(tmp_path), f)) > 0, f
