"""Host side of the perceptual objective (no GPU): the library's rule and the n_obj rule of create, target preparation, the config keys
and flags, the search surface with three objectives."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from clip_glass_amd import config as gconfig
from clip_glass_amd import engine, generator, parallel, run, search, synth


# ---- the library's rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen_res,S", [(0, 16), (0, 256), (0, 512), (32, 32), (64, 32), (1024, 256), (1024, 128), (256, 256)])
def test_supported(gen_res, S):
    assert engine.lpips_supported(gen_res, S) == (True, "")


@pytest.mark.parametrize("gen_res,S,word", [
    (0, 24, "multiple of 16"),            # 24 / 8 = 3: the fourth max pool would meet an odd side
    (0, 8, "multiple of 16"),
    (0, 1024, "[16, 512]"),
    (96, 64, "must divide"),
    (1024, 64, "at most 8"),              # box 16
    (512, 32, "at most 8"),
])
def test_refused_with_the_reason(gen_res, S, word):
    ok, msg = engine.lpips_supported(gen_res, S)
    assert not ok and word in msg, msg


def test_config_struct_appends_the_two_fields():
    G = engine.GlassConfig
    names = [f[0] for f in G._fields_]
    assert names[31:35] == ["clip_arch", "clip_rn_layers", "lpips_size", "lpips_lambda"]
    assert (G.clip_arch.offset, G.clip_rn_layers.offset) == (364, 368)            # nothing before them moved
    assert (G.lpips_size.offset, G.lpips_lambda.offset) == (384, 388) and G.sim_columns.offset == 392      # 384 + 8: the two fields fill 8 bytes
    z = G()
    assert z.lpips_size == 0 and z.lpips_lambda == 0.0


def _create(**kw):
    """glass_engine_create on the mini geometry (32 px): the rules sit in front of the device lookup, so a refusal needs no GPU; an accepted
    config goes on to look for a device (and fails there on a machine without one)."""
    kw.setdefault("mbstd_group", 2)
    return engine.Engine([16, 16, 32, 32], latent_size=32, mapping_layers=2, batch_size=2, clip=(64, 2, 1, 8, 32, 32), **kw)


@pytest.mark.parametrize("use_d,lam,n_obj,ok", [
    (True, 0.0, 3, True), (True, 0.0, 2, False), (True, 0.5, 2, True), (True, 0.5, 3, False),
    (False, 0.0, 2, True), (False, 0.0, 1, False), (False, 0.5, 1, True), (False, 0.5, 2, False),
])
def test_n_obj_rule_at_create(use_d, lam, n_obj, ok):
    assert engine.lpips_n_obj(use_d, lam) == (n_obj if ok else engine.lpips_n_obj(use_d, lam))
    try:
        e = _create(use_discriminator=use_d, n_obj=n_obj, lpips_size=32, lpips_lambda=lam)
        e.close()
        msg = ""
    except RuntimeError as ex:
        msg = str(ex)
    assert ("n_obj must be 1 + use_discriminator" in msg) == (not ok), msg


def test_create_applies_the_size_rule_and_todays_n_obj_rule():
    with pytest.raises(RuntimeError, match="multiple of 16"):
        _create(n_obj=3, lpips_size=24)
    with pytest.raises(RuntimeError, match="must divide"):
        _create(n_obj=3, lpips_size=64)                       # a 32 px generator
    with pytest.raises(RuntimeError, match="lpips_lambda"):
        _create(n_obj=2, lpips_size=32, lpips_lambda=-1.0)
    with pytest.raises(RuntimeError, match="n_obj must be 1 or 2"):
        _create(n_obj=3)                                      # the objective off: today's rule, verbatim
    with pytest.raises(RuntimeError, match="needs a generator"):
        engine.Engine([], latent_size=4, mapping_layers=0, batch_size=1, use_discriminator=False, n_obj=2, noise_mode=0, lpips_size=32)


# ---- target preparation ------------------------------------------------------------------------------------------------------------
def test_target_preparation_known_answer():
    """An 8 x 12 image of 4 x 4 blocks, centre-cropped to columns 2 .. 9: the left output column averages half of block 0 and half of
    block 1, the right one half of block 1 and half of block 2; then 2 x - 1."""
    vals = np.array([[0.0, 0.25, 0.5], [1.0, 0.75, 0.5]], np.float32)       # block rows x block columns
    img = np.repeat(np.repeat(vals, 4, axis=0), 4, axis=1)
    a = np.stack([img, 1 - img, 0.5 * img])
    t = generator.prepare_lpips_target(a, 2)
    assert t.shape == (3, 2, 2) and t.dtype == np.float32
    want0 = 2 * np.array([[0.125, 0.375], [0.875, 0.625]]) - 1
    np.testing.assert_allclose(t[0], want0, atol=1e-7)
    np.testing.assert_allclose(t[1], 2 * (1 - (want0 + 1) / 2) - 1, atol=1e-7)
    np.testing.assert_allclose(t[2], 2 * (0.5 * (want0 + 1) / 2) - 1, atol=1e-7)
    np.testing.assert_array_equal(generator.prepare_lpips_target(a[:, :, 2:10], 8), 2 * a[:, :, 2:10] - 1)      # box 1: the pixels themselves


def test_target_preparation_from_a_file_and_through_the_antialiased_resize(tmp_path):
    from PIL import Image
    rgb = (synth._rng(3, "png").random((16, 24, 3)) * 255).astype(np.uint8)
    path = os.path.join(str(tmp_path), "t.png")
    Image.fromarray(rgb).save(path)
    t = generator.prepare_lpips_target(path, 8)
    sq = rgb[:, 4:20].astype(np.float64).transpose(2, 0, 1) / 255
    np.testing.assert_allclose(t, 2 * sq.reshape(3, 8, 2, 8, 2).mean(axis=(2, 4)) - 1, atol=1e-6)
    u = generator.prepare_lpips_target(np.full((3, 10, 10), 0.25, np.float32), 4)      # 10 % 4 != 0: PIL's resize; a flat image stays flat
    assert u.shape == (3, 4, 4)
    np.testing.assert_allclose(u, -0.5, atol=1e-5)
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        generator.prepare_lpips_target(np.zeros((8, 8)), 4)


# ---- config keys, flags ------------------------------------------------------------------------------------------------------------
def _ns(name, **kw):
    cfg = types.SimpleNamespace(config=name)
    vars(cfg).update(gconfig.get_config(name))
    vars(cfg).update(kw)
    return cfg


def test_options_defaults_and_refusals():
    assert generator.lpips_options(_ns("StyleGAN2_ffhq_d")) is None
    o = generator.lpips_options(_ns("StyleGAN2_ffhq_d", lpips_target="t.png", lpips_weights="synthetic:1"))
    assert o == dict(target="t.png", size=256, lam=0.0, weights="synthetic:1")
    o = generator.lpips_options(_ns("DeepMindBigGAN256", lpips_target="t.png", lpips_weights="w.pt", lpips_size=128, lpips_lambda=0.5))
    assert (o["size"], o["lam"]) == (128, 0.5)
    with pytest.raises(ValueError, match="without lpips_target"):
        generator.lpips_options(_ns("StyleGAN2_ffhq_d", lpips_size=128))
    with pytest.raises(ValueError, match="multiple of 16"):
        generator.lpips_options(_ns("StyleGAN2_ffhq_d", lpips_target="t.png", lpips_size=100, lpips_weights="synthetic"))
    with pytest.raises(ValueError, match="lpips_lambda"):
        generator.lpips_options(_ns("StyleGAN2_ffhq_d", lpips_target="t.png", lpips_lambda=-0.1, lpips_weights="synthetic"))
    with pytest.raises(RuntimeError, match="lpips_weights is not set"):
        generator.lpips_options(_ns("StyleGAN2_ffhq_d", lpips_target="t.png"))


def test_gpt2_config_refuses_the_keys_before_any_weight_is_looked_for():
    for kw in (dict(lpips_target="t.png"), dict(lpips_lambda=0.5), dict(lpips_size=256), dict(lpips_weights="synthetic")):
        cfg = _ns("GPT2", weights="/nonexistent/gpt2.bin", clip_weights="/nonexistent/clip.pt", **kw)
        cfg.model = lambda c: pytest.fail("the model (its weights) was looked for before the refusal")
        with pytest.raises(ValueError, match="img2txt"):
            generator.Generator(cfg)
    with pytest.raises(ValueError, match="img2txt"):
        run.main(["--config", "GPT2", "--lpips-target", "t.png", "--weights", "/nonexistent", "--clip-weights", "/nonexistent"])


def test_n_obj_and_algorithm_change_on_a_copy():
    for name, n0 in (("StyleGAN2_ffhq_d", 2), ("StyleGAN2_ffhq_nod", 1), ("DeepMindBigGAN512", 1)):
        cfg = _ns(name, lpips_target="t.png", lpips_weights="synthetic:0")
        alg0 = cfg.algorithm
        out = generator.lpips_config(cfg, generator.lpips_options(cfg))
        assert out is not cfg and out.problem_args["n_obj"] == n0 + 1 and out.algorithm == "nsga2"
        assert cfg.problem_args["n_obj"] == n0 and cfg.algorithm == alg0
        assert gconfig.get_config(name)["problem_args"]["n_obj"] == n0 and gconfig.get_config(name)["algorithm"] == alg0
        assert out.problem_args["n_var"] == cfg.problem_args["n_var"] and out.lpips_target == "t.png"
        lam = _ns(name, lpips_target="t.png", lpips_weights="synthetic:0", lpips_lambda=0.3)
        assert generator.lpips_config(lam, generator.lpips_options(lam)) is lam      # lambda > 0: both stay as they are
        assert generator.lpips_config(_ns(name), None).problem_args["n_obj"] == n0


def test_run_flags_reach_the_config(monkeypatch):
    seen = {}

    class Stop(Exception):
        pass

    def fake_problem(config, dist=None):
        seen.update(vars(config))
        raise Stop()
    monkeypatch.setattr(run, "GenerationProblem", fake_problem)
    with pytest.raises(Stop):
        run.main(["--config", "StyleGAN2_church_d", "--lpips-target", "x.png", "--lpips-size", "128", "--lpips-lambda", "0.25",
                  "--lpips-weights", "synthetic:4"])
    assert (seen["lpips_target"], seen["lpips_size"], seen["lpips_lambda"], seen["lpips_weights"]) == ("x.png", 128, 0.25, "synthetic:4")
    seen.clear()
    with pytest.raises(Stop):
        run.main(["--config", "StyleGAN2_church_d"])
    assert not [k for k in generator.LPIPS_KEYS if seen.get(k) is not None]
    with pytest.raises(ValueError, match="without lpips_target"):
        run.main(["--config", "StyleGAN2_church_d", "--lpips-lambda", "0.25"])


def test_load_lpips_state_from_a_torch_file(tmp_path):
    import torch
    sd = synth.lpips_state(2)
    path = os.path.join(str(tmp_path), "vgg.pt")
    torch.save({(k[len("lpips."):] if i % 2 else k): torch.tensor(v).view(1, -1, 1, 1) if ".lin." in k else torch.tensor(v)
                for i, (k, v) in enumerate(sd.items())}, path)
    got = generator.load_lpips_state(path)
    assert set(got) == set(sd)
    for k in sd:
        assert got[k].shape == sd[k].shape and (got[k] == sd[k]).all(), k
    assert (generator.load_lpips_state("synthetic:2")["lpips.lin.4.weight"] == sd["lpips.lin.4.weight"]).all()


# ---- three objectives through the search surface -----------------------------------------------------------------------------------
def test_objective_names_scatters_and_final_pick():
    d3 = generator.lpips_config(_ns("StyleGAN2_ffhq_d", lpips_target="t", lpips_weights="synthetic"),
                                dict(target="t", size=256, lam=0.0, weights="synthetic"))
    assert run.objective_names(d3) == ["similarity", "discriminator", "lpips"]
    nod = generator.lpips_config(_ns("StyleGAN2_ffhq_nod", lpips_target="t", lpips_weights="synthetic"),
                                 dict(target="t", size=256, lam=0.0, weights="synthetic"))
    assert run.objective_names(nod) == ["similarity", "lpips"]
    assert run.objective_names(_ns("StyleGAN2_ffhq_d")) == ["similarity", "discriminator"]
    assert run.objective_names(_ns("StyleGAN2_ffhq_d", lpips_target="t", lpips_lambda=0.5)) == ["similarity", "discriminator"]
    assert run.objective_names(_ns("StyleGAN2_ffhq_nod")) == ["similarity"]
    assert run.scatter_pairs(["similarity", "discriminator"]) == [(0, 1, "F.jpg")]
    assert [p[:2] for p in run.scatter_pairs(["similarity", "discriminator", "lpips"])] == [(0, 1), (0, 2), (1, 2)]
    assert len({p[2] for p in run.scatter_pairs(["similarity", "discriminator", "lpips"])}) == 3
    assert run.final_pick_weights(["similarity", "discriminator"]) == [0.0, 1.0]
    assert run.final_pick_weights(["similarity", "lpips"]) == [0.0, 1.0]
    assert run.final_pick_weights(["similarity", "discriminator", "lpips"]) == [0.0, 0.5, 0.5]
    # a hand-made front: row 0 best similarity, row 1 best realism, row 2 best closeness, row 3 good at the last two
    F = np.array([[-0.9, 1.0, 1.0], [-0.3, 0.0, 0.9], [-0.1, 0.9, 0.0], [-0.2, 0.1, 0.1]])
    assert search.pseudo_weights_choice(F, run.final_pick_weights(["similarity", "discriminator", "lpips"])) == 3
    assert search.pseudo_weights_choice(F[:, [0, 2]], run.final_pick_weights(["similarity", "lpips"])) == 2


def test_nsga2_runs_on_three_objectives():
    class Prob:
        n_var, n_obj, n_constr = 4, 3, 0
        xl, xu = np.full(4, -1.0), np.full(4, 1.0)

        def evaluate(self, x, *a, **k):
            x = np.atleast_2d(x)
            return dict(F=np.stack([(x ** 2).sum(1), ((x - 0.5) ** 2).sum(1), ((x + 0.5) ** 2).sum(1)], 1), G=np.zeros(len(x)))

        _evaluate = None
    p = Prob()
    p._evaluate = lambda x, out, *a, **k: out.update(p.evaluate(x))
    sampling = types.SimpleNamespace(_do=lambda prob, n: np.random.uniform(-1, 1, (n, prob.n_var)))
    res = search.minimize(p, "nsga2", 12, 3, sampling, seed=1, verbose=False)
    assert np.atleast_2d(res.F).shape[1] == 3 and np.atleast_2d(res.X).shape[1] == 4


def _gloo_worker3(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    class FakeEngine:
        cfg = types.SimpleNamespace(n_obj=3)

        def evaluate(self, x, generation=0, first_minibatch=0, noise=None):
            x = np.asarray(x, np.float32)
            return np.stack([x[:, 0], x[:, 1] + first_minibatch, x[:, 2] * generation], 1).astype(np.float32)
    ev = parallel.ShardedEvaluator(FakeEngine(), dist, rank, world, 4)
    q.put((rank, ev.evaluate_global(synth.latents(0, 20, 8).astype(np.float32), generation=2)))      # 5 minibatches: ragged 3 + 2
    dist.destroy_process_group()


def test_three_columns_pass_the_sharded_gather():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gloo_worker3, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    x = synth.latents(0, 20, 8).astype(np.float32)
    mb = np.repeat(np.array([0, 0, 0, 3, 3]), 4)
    want = np.stack([x[:, 0], x[:, 1] + mb, x[:, 2] * 2], 1)
    for _, Fg in res:
        assert Fg.shape == (20, 3)
        np.testing.assert_allclose(Fg, want, rtol=1e-6)
