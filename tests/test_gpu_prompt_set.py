"""Prompt sets through the engine (include/glass.h "Prompt sets"): the identities with the single-target pass (bit for bit), the pareto
layout next to the discriminator and the LPIPS column, chunks / shards / stream modes, parity of every column against the float64 oracle
tower, image prompts through encode_generated, the profile of the pass, the refusals, and the search driver."""
import ctypes as C
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import clip_views_ref as VR
import glass_models as M
import lpips_ref as LR
from clip_glass_amd import synth
from clip_glass_amd.engine import Engine, prompt_n_obj
from oracle import clip_ref
from util import diag

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED, GEN, P, BS = 7, 3, 8, 4


def _engine(name, sd, *, views=0, use_d=False, K=0, chunk=0, lpips_size=0, max_pop=P, n_obj=None, **kw):
    c = M.CONFIGS[name]
    if n_obj is None:
        n_obj = prompt_n_obj(K, use_d, bool(lpips_size))
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=BS, use_discriminator=use_d, n_obj=n_obj,
               max_pop=max_pop, chunk=chunk, clip=c["clip"], noise_mode=2, noise_seed=SEED, clip_views=views, sim_columns=K,
               lpips_size=lpips_size, **kw)
    e.load_state(sd)
    e.finalize()
    return e


@functools.lru_cache(maxsize=None)
def _case(name):
    c = M.CONFIGS[name]
    sd = M.make_state(name, 0)
    x = synth.latents(3, P, c["latent"])
    planes = M.noise_planes(name, 31, 0, P // BS)
    base = synth.normal(25, "t", (P, c["clip"][5]))
    targets = np.stack([M.make_target(base[i:], seed=i) for i in range(3)])
    return sd, x, planes, targets


def _recombine(cols, weights):
    acc, W = np.zeros(cols.shape[0], F32), F32(0)
    for t in range(cols.shape[1]):
        acc = (acc + (F32(weights[t]) * cols[:, t]).astype(F32)).astype(F32)
        W = F32(W + np.abs(F32(weights[t])))
    return (acc / W).astype(F32)


# ---- (a) one entry of weight 1 is set_target ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [0, 4])
@pytest.mark.parametrize("use_d", [False, True])
def test_one_entry_of_weight_one_is_set_target(views, use_d):
    sd, x, planes, targets = _case("mini")
    e = _engine("mini", sd, views=views, use_d=use_d)
    e.set_target(targets[0])
    F0 = e.evaluate(x, generation=GEN, noise=planes)
    d0 = e.details(P)
    v0 = e.view_details(P)["sims"] if views else None
    e.set_targets(targets[:1], [1.0])
    F1 = e.evaluate(x, generation=GEN, noise=planes)
    d1 = e.details(P)
    assert F1.shape == (P, 1 + use_d) and np.ptp(F1[:, 0]) > 0
    assert F1.tobytes() == F0.tobytes()
    assert d1["sim"].tobytes() == d0["sim"].tobytes() and e.set_details(P)[:, 0].tobytes() == d0["sim"].tobytes()
    if views:
        assert e.view_details(P)["sims"].tobytes() == v0.tobytes()
    e.set_target(targets[0])                                # back to one target: the set is cleared
    assert e.evaluate(x, generation=GEN, noise=planes).tobytes() == F0.tobytes()
    with pytest.raises(RuntimeError, match="no prompt set is active"):
        e.set_details(P)
    e.close()


# ---- (b) three entries, mixed signs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [0, 4])
def test_three_entries_are_three_single_target_passes(views):
    sd, x, planes, targets = _case("mini")
    w = np.array([1.5, -0.25, 3.0], F32)
    e = _engine("mini", sd, views=views, use_d=True)
    singles = []
    for t in range(3):
        e.set_target(targets[t])
        e.evaluate(x, generation=GEN, noise=planes)
        singles.append(e.details(P)["sim"])
    singles = np.stack(singles, axis=1)
    e.set_targets(targets, w)
    Fs = e.evaluate(x, generation=GEN, noise=planes)
    cols = e.set_details(P)
    e.close()
    assert cols.tobytes() == singles.tobytes()
    assert Fs[:, 0].tobytes() == (-_recombine(singles, w)).tobytes()
    assert not np.array_equal(Fs[:, 0], -singles[:, 0])     # the other entries count


# ---- (c) pareto next to the discriminator and the LPIPS column ---------------------------------------------------------------------------
def test_pareto_columns_with_discriminator_and_lpips():
    sd, x, planes, targets = _case("mini")
    lp_sd = synth.lpips_state(3)
    tgt = LR.images(9, 1, 32, "target")[0]
    single = _engine("mini", dict(sd, **lp_sd), use_d=True, lpips_size=32)
    single.set_lpips_target(tgt)
    ref = []
    for t in range(2):
        single.set_target(targets[t])
        ref.append(single.evaluate(x, generation=GEN, noise=planes))
    single.close()
    assert ref[0].shape == (P, 3)
    e = _engine("mini", dict(sd, **lp_sd), use_d=True, lpips_size=32, K=2)
    e.set_lpips_target(tgt)
    e.set_targets(targets[:2], [0.5, -2.0], mode="pareto")
    Fp = e.evaluate(x, generation=GEN, noise=planes)
    sim = e.details(P)["sim"]
    cols = e.set_details(P)
    e.close()
    assert Fp.shape == (P, 4) and Fp.dtype == F32
    assert Fp[:, 0].tobytes() == ref[0][:, 0].tobytes()             # w > 0: -sim, towards
    assert Fp[:, 1].tobytes() == (-ref[1][:, 0]).tobytes()          # w < 0: +sim, away from
    assert Fp[:, 2].tobytes() == ref[0][:, 1].tobytes() and Fp[:, 3].tobytes() == ref[0][:, 2].tobytes()
    assert (Fp[:, 2] >= 0).all() and (Fp[:, 3] > 0).all()
    assert sim.tobytes() == _recombine(cols, [0.5, -2.0]).tobytes()   # details' sim: the mode-sum value in both modes


# ---- (d) chunks, shards, stream modes ------------------------------------------------------------------------------------------------
def test_chunks_shards_and_stream_modes_agree():
    sd, x, planes, targets = _case("mid")
    w = [1.0, -0.5, 2.0]
    rows = {}
    for chunk in (8, 4):
        e = _engine("mid", sd, views=4, use_d=True, chunk=chunk)
        e.set_targets(targets, w)
        rows[chunk] = e.evaluate(x, generation=GEN, noise=planes)
        cols = e.set_details(P)
        if chunk == 8:
            halves, hcols = [], []
            for h in range(2):
                halves.append(e.evaluate(x[4 * h:4 * h + 4], generation=GEN, first_minibatch=h, noise=planes[h:h + 1]))
                hcols.append(e.set_details(4))
            assert np.concatenate(hcols).tobytes() == cols.tobytes()
            modes = []
            for mode in (0, 1, 2):
                e.set_overlap(mode)
                modes.append(e.evaluate(x, generation=GEN, noise=planes))
        e.close()
    assert rows[8].shape == (P, 2)
    assert rows[4].tobytes() == rows[8].tobytes()
    assert np.concatenate(halves)[:, 0].tobytes() == rows[8][:, 0].tobytes()      # (the hinge of a 4-row call has its own minibatch groups: the same here, bs 4)
    assert np.concatenate(halves).tobytes() == rows[8].tobytes()
    assert modes[0].tobytes() == rows[8].tobytes() and modes[1].tobytes() == rows[8].tobytes() and modes[2].tobytes() == rows[8].tobytes()


# ---- (e) every column against the float64 oracle tower -----------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [0, 4])
def test_columns_against_the_oracle(views):
    sd, x, planes, _ = _case("mid")
    S = M.CONFIGS["mid"]["clip"][4]
    tsd = {k: torch.as_tensor(v) for k, v in sd.items()}
    e = _engine("mid", sd, views=views)
    img = e.generate(x, generation=GEN, noise=planes)
    V = max(views, 1)
    boxes = synth.clip_view_boxes(SEED, GEN, V, img.shape[-1], 500, True, False) if views else [(0, 0, img.shape[-1], 0)]
    with torch.no_grad():
        feats = clip_ref.encode_image(tsd, VR.torch_views(img, S, boxes).reshape(P * V, 3, S, S).float()).numpy().astype(np.float64).reshape(P, V, -1)
    mean_f = feats.mean(axis=1)
    targets = np.stack([M.make_target(mean_f[i:], seed=i) for i in range(3)])
    w = np.array([2.0, -1.0, 0.5])
    tn = targets.astype(np.float64)
    c_o = np.einsum("pvd,td->pvt", feats, tn) / np.maximum(np.linalg.norm(feats, axis=2)[:, :, None] * np.linalg.norm(tn, axis=1)[None, None, :], 1e-8)
    cols_o = c_o.mean(axis=1)
    sim_o = (cols_o * w).sum(axis=1) / np.abs(w).sum()
    diag("[prompt-set] oracle V%d columns range [%.3f, %.3f], sim range [%.3f, %.3f]" % (V, cols_o.min(), cols_o.max(), sim_o.min(), sim_o.max()))
    assert (np.abs(cols_o) > 0.1).all() and (np.abs(sim_o) > 0.1).all(), (cols_o, sim_o)      # on the oracle's values alone
    e.set_targets(targets, w)
    Fe = e.evaluate(x, generation=GEN, noise=planes)
    cols, sim = e.set_details(P), e.details(P)["sim"]
    e.close()
    rel_c = np.abs(cols - cols_o) / np.abs(cols_o)
    rel_s = np.abs(sim - sim_o) / np.abs(sim_o)
    diag("[prompt-set] oracle V%d: columns max rel err %.3e, sim %.3e" % (V, rel_c.max(), rel_s.max()))
    assert rel_c.max() < 1e-3 and rel_s.max() < 1e-3, (rel_c.max(), rel_s.max())
    assert Fe[:, 0].tobytes() == (-sim).tobytes()


# ---- (f) an image prompt is comparable with the candidates ---------------------------------------------------------------------------
@pytest.mark.parametrize("preprocess", ["reference", "clip"])
def test_encode_generated_of_a_candidates_image_scores_one(preprocess):
    from clip_glass_amd.generator import CLIP_PREPROCESS
    sd, x, planes, _ = _case("mid")
    rz, nm = CLIP_PREPROCESS[preprocess]
    e = _engine("mid", sd, clip_resize=rz, clip_normalize=nm)
    img = e.generate(x, generation=GEN, noise=planes)
    feats = e.encode_generated(2 * img - 1)
    assert feats.shape == (P, M.CONFIGS["mid"]["clip"][5]) and np.isfinite(feats).all()
    sims = []
    for p in (0, 5):
        e.set_targets(feats[p:p + 1], [1.0])
        e.evaluate(x, generation=GEN, noise=planes)
        s = e.details(P)["sim"]
        sims.append(s[p])
        assert s[p] == s.max()                               # its own image is the best match
    e.close()
    diag("[prompt-set] encode_generated %s: own-image sims %s" % (preprocess, sims))
    assert min(sims) >= 1 - 1e-3 and max(sims) <= 1 + 1e-6, sims


# ---- (g) the profile of the pass ----------------------------------------------------------------------------------------------------
def test_profile_rows_default_and_with_a_set():
    """The default engine's pass: row for row the pinned table of tests/test_gpu_engine.py::test_launch_table_is_pinned.  With a set active: the
    same rows and launches — the one cosine kernel inside clip.head and the one assemble_F kernel (csrc/score.hip) end both."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_table.json")) as f:
        golden = json.load(f)["mid"]
    c = M.CONFIGS["mid"]
    x = synth.latents(1, 4, c["latent"])
    t = np.ones((3, c["clip"][5]), F32)
    got = {}
    for tag, K in (("default", 0), ("sum T=1", 0), ("sum T=3", 0), ("pareto K=2", 2)):
        e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=4, use_discriminator=True,
                   n_obj=prompt_n_obj(K, True), max_pop=4, clip=c["clip"], noise_mode=1, sim_columns=K)
        e.load_state(M.make_state("mid", 0))
        e.finalize()
        if tag == "default":
            e.set_target(t[0])
        elif K:
            e.set_targets(t[:2], [1.0, -1.0], mode="pareto")
        else:
            e.set_targets(t[:1] if tag.endswith("1") else t, [1.0] if tag.endswith("1") else [1.0, -2.0, 0.5])
        e.set_profiling(True)
        e.evaluate(x)
        got[tag] = [[r["name"], r["launches"]] for r in e.profile()]
        e.close()
    assert got["default"] == golden
    for tag in ("sum T=1", "sum T=3", "pareto K=2"):
        assert got[tag] == got["default"], tag


# ---- (h) refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_by_status_and_message():
    sd, x, planes, targets = _case("mini")
    E = targets.shape[1]
    e = _engine("mini", sd)
    lib = e.lib

    def fp(a):
        return a.ctypes.data_as(C.POINTER(C.c_float))
    w3 = np.ones(3, F32)

    def call(feats, weights, T, En, mode):
        rc = lib.glass_engine_set_targets(e._h, fp(np.ascontiguousarray(feats, F32)), fp(np.ascontiguousarray(weights, F32)), T, En, mode)
        return rc, lib.glass_last_error().decode()
    rc, msg = call(targets, w3, 3, E - 1, 0)
    assert rc == -1 and "clip_embed" in msg
    for bad in (0.0, np.nan, np.inf):
        rc, msg = call(targets, [1.0, bad, 1.0], 3, E, 0)
        assert rc == -1 and "weight 1 must be finite and non-zero" in msg, (bad, msg)
    rc, msg = call(np.zeros((17, E), F32), np.ones(17, F32), 17, E, 0)
    assert rc == -1 and "1 .. 16" in msg
    rc, msg = call(targets, w3, 3, E, 1)
    assert rc == -1 and "sim_columns" in msg               # a front needs an engine made for it
    rc, msg = call(targets, w3, 3, E, 2)
    assert rc == -1 and "mode must be" in msg
    with pytest.raises(RuntimeError, match="no prompt set is active"):
        e.set_details(P)
    with pytest.raises(RuntimeError, match=r"set_target\(\) first"):
        e.evaluate(x, noise=planes)
    with pytest.raises(RuntimeError, match="more images than max_pop"):
        e.encode_generated(np.zeros((P + 1, 3, 32, 32), F32))
    with pytest.raises(ValueError, match=r"\[n, 3, 32, 32\]"):
        e.encode_generated(np.zeros((1, 3, 16, 16), F32))
    e.close()

    k2 = _engine("mini", sd, K=2)
    rc = k2.lib.glass_engine_set_target(k2._h, fp(targets[0]), E)
    assert rc == -2 and "set_targets()" in k2.lib.glass_last_error().decode()
    with pytest.raises(RuntimeError, match=r"libglass error -2: set_targets\(\) first"):
        k2.evaluate(x, noise=planes)
    with pytest.raises(RuntimeError, match="mode sum"):
        k2.set_targets(targets[:2], [1.0, 1.0])
    with pytest.raises(RuntimeError, match="number of entries"):
        k2.set_targets(targets, w3, mode="pareto")
    k2.set_targets(targets[:2], [1.0, -1.0], mode="pareto")
    assert k2.evaluate(x, noise=planes).shape == (P, 2)
    k2.close()

    c = M.CONFIGS["mini"]
    text_only = Engine([], latent_size=4, mapping_layers=0, batch_size=1, use_discriminator=False, n_obj=1, clip=c["clip"], noise_mode=0)
    out = np.zeros((1, E), F32)
    rc = text_only.lib.glass_engine_encode_generated(text_only._h, fp(np.zeros((1, 3, 32, 32), F32)), 1, fp(out))
    assert rc == -2 and "no generator" in text_only.lib.glass_last_error().decode()
    text_only.close()


# ---- (i) the search driver -------------------------------------------------------------------------------------------------------------
def _driver_extra():
    c = M.CONFIGS["mini"]
    base = synth.normal(25, "t", (8, c["clip"][5]))
    return dict(channels=c["channels"], dim_z=c["latent"], mapping_layers=c["mapping"], clip_geometry=c["clip"],
                target_features=M.make_target(base), noise_mode=1, noise_seed=42,
                prompts=[(M.make_target(base[1:], seed=1), -1.0)], prompt_mode="pareto",
                problem_args=dict(n_var=c["latent"], n_obj=2, n_constr=c["latent"], xl=-10, xu=10))


def test_generation_problem_and_search_with_a_pareto_set():
    from clip_glass_amd import config as gconfig, search
    from clip_glass_amd.operators import get_operators
    from clip_glass_amd.problem import GenerationProblem
    c = M.CONFIGS["mini"]
    cfg = types.SimpleNamespace(config="StyleGAN2_ffhq_d", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("StyleGAN2_ffhq_d"))
    vars(cfg).update(weights="synthetic:0", clip_weights="synthetic:0", pop_size=8, **_driver_extra())
    prob = GenerationProblem(cfg)
    gen = prob.generator
    assert prob.config.problem_args["n_obj"] == 3 and prob.config.algorithm == "nsga2" and prob.n_obj == 3
    assert cfg.problem_args["n_obj"] == 2                                   # the caller's config keeps its values
    assert gen.prompt_mode == "pareto" and gen.prompt_features.shape == (2, c["clip"][5]) and gen.prompt_weights.tolist() == [1.0, -1.0]
    np.testing.assert_array_equal(gen.prompt_features[0], cfg.target_features)
    out = {}
    prob._evaluate(synth.latents(1, 8, c["latent"]), out)
    assert out["F"].shape == (8, 3) and out["F"].dtype == F32 and np.isfinite(out["F"]).all()
    cols = gen.engine.set_details(8)
    assert out["F"][:, 0].tobytes() == (-cols[:, 0]).tobytes() and out["F"][:, 1].tobytes() == cols[:, 1].tobytes()
    res = search.minimize(prob, prob.config.algorithm, 8, 2, get_operators(prob.config)["sampling"], seed=1, verbose=False)
    assert np.atleast_2d(res.F).shape[1] == 3
    gen.engine.close()


def test_sum_set_through_the_generator_keeps_the_objectives():
    from clip_glass_amd import config as gconfig
    from clip_glass_amd.problem import GenerationProblem
    c = M.CONFIGS["mini"]
    extra = _driver_extra()
    extra.update(prompt_mode=None, target_weight=2.0)
    cfg = types.SimpleNamespace(config="StyleGAN2_ffhq_d", device="cuda", target="unused")
    vars(cfg).update(gconfig.get_config("StyleGAN2_ffhq_d"))
    vars(cfg).update(weights="synthetic:0", clip_weights="synthetic:0", pop_size=8, **extra)
    prob = GenerationProblem(cfg)
    assert prob.config is cfg and prob.n_obj == 2 and prob.generator.prompt_mode == "sum"
    out = {}
    prob._evaluate(synth.latents(1, 8, c["latent"]), out)
    assert out["F"].shape == (8, 2)
    cols = prob.generator.engine.set_details(8)
    assert out["F"][:, 0].tobytes() == (-_recombine(cols, [2.0, -1.0])).tobytes()
    prob.generator.engine.close()


def test_run_main_with_a_pareto_set(tmp_path):
    from clip_glass_amd import run
    argv = ["--config", "StyleGAN2_ffhq_d", "--generations", "2", "--save-each", "2", "--tmp-folder", str(tmp_path),
            "--weights", "synthetic:0", "--clip-weights", "synthetic:0", "--pop-size", "8"]
    res = run.main(argv, extra_config=_driver_extra())
    assert np.atleast_2d(res.F).shape[1] == 3
    for f in ("genetic-it-final.jpg", "genetic_result", "ls_result", "output.jpg", "F-similarity-0-similarity-1.jpg",
              "F-similarity-0-discriminator.jpg", "F-similarity-1-discriminator.jpg"):
        assert os.path.getsize(os.path.join(str(tmp_path), f)) > 0, f
    assert not os.path.exists(os.path.join(str(tmp_path), "F.jpg"))
