"""Host side of prompt sets (no GPU): the library's rule and the n_obj rule of create, the config keys and their refusals, the config copy a
pareto set searches (alone and with the LPIPS keys), "TEXT::W" parsing and the flags, and the search surface for K = 2 .. 4 columns."""
import ctypes as C
import types

import numpy as np
import pytest

from clip_glass_amd import config as gconfig
from clip_glass_amd import engine, generator, run


def test_symbols_are_exported():
    lib = engine.load_library()
    for name in ("glass_prompt_set_supported", "glass_engine_set_targets", "glass_engine_last_set_details", "glass_engine_encode_generated",
                 "glass_op_cosine_set", "glass_op_assemble_F_set"):
        assert hasattr(lib, name), name


def test_config_struct_appends_the_field():
    G = engine.GlassConfig
    names = [f[0] for f in G._fields_]
    assert names[33:36] == ["lpips_size", "lpips_lambda", "sim_columns"]
    assert (G.lpips_size.offset, G.lpips_lambda.offset) == (384, 388)             # nothing before it moved
    assert G.sim_columns.offset == 392 and C.sizeof(G) == 408
    assert G().sim_columns == 0


# ---- the library's rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,mode,K", [(1, "sum", 0), (1, "sum", 1), (16, "sum", 0), (7, 0, 1), (2, "pareto", 2), (3, "pareto", 3), (4, 1, 4)])
def test_supported(T, mode, K):
    assert engine.prompt_set_supported(T, mode, K) == (True, "")
    assert engine.Engine.prompt_set_supported(T, mode, K) == (True, "")


@pytest.mark.parametrize("T,mode,K,word", [
    (0, "sum", 0, "1 .. 16"),
    (17, "sum", 0, "1 .. 16"),
    (2, 2, 0, "mode must be"),
    (2, "sum", 2, "mode sum"),              # an engine made for a front takes no blended set
    (2, "sum", 5, "sim_columns"),
    (1, "pareto", 1, "2 .. 4 entries"),
    (5, "pareto", 5, "sim_columns"),
    (5, "pareto", 4, "2 .. 4 entries"),
    (3, "pareto", 2, "sim_columns = the number of entries"),
    (2, "pareto", 0, "sim_columns = the number of entries"),
])
def test_refused_with_the_reason(T, mode, K, word):
    ok, msg = engine.prompt_set_supported(T, mode, K)
    assert not ok and word in msg, msg


def test_mode_names():
    assert engine.prompt_mode_id("sum") == 0 and engine.prompt_mode_id("pareto") == 1 and engine.prompt_mode_id(1) == 1
    with pytest.raises(ValueError, match="expected one of sum, pareto"):
        engine.prompt_mode_id("blend")


def _create(**kw):
    """glass_engine_create on the mini geometry: the rules sit in front of the device lookup, so a refusal needs no GPU; an accepted config
    goes on to look for a device (and fails there, with another message, on a machine without one)."""
    kw.setdefault("mbstd_group", 2)
    return engine.Engine([16, 16, 32, 32], latent_size=32, mapping_layers=2, batch_size=2, clip=(64, 2, 1, 8, 32, 32), **kw)


@pytest.mark.parametrize("K,use_d,lpips,n_obj,ok", [
    (2, False, False, 2, True), (2, False, False, 1, False), (2, True, False, 3, True), (2, True, False, 2, False),
    (4, True, True, 6, True), (4, True, True, 5, False), (3, False, True, 4, True), (3, False, True, 3, False),
])
def test_n_obj_rule_at_create(K, use_d, lpips, n_obj, ok):
    assert engine.prompt_n_obj(K, use_d, lpips) == (n_obj if ok else engine.prompt_n_obj(K, use_d, lpips))
    try:
        e = _create(use_discriminator=use_d, n_obj=n_obj, sim_columns=K, lpips_size=32 if lpips else 0)
        e.close()
        msg = ""
    except RuntimeError as ex:
        msg = str(ex)
    assert ("n_obj must be sim_columns + use_discriminator" in msg) == (not ok), msg


def test_create_refuses_the_fold_and_a_bad_column_count():
    with pytest.raises(RuntimeError, match="no single one"):
        _create(n_obj=3, sim_columns=2, lpips_size=32, lpips_lambda=0.5)
    with pytest.raises(RuntimeError, match="sim_columns must be"):
        _create(n_obj=5, sim_columns=5, use_discriminator=False)
    with pytest.raises(RuntimeError, match="n_obj must be 1 or 2"):
        _create(n_obj=3, sim_columns=1)                    # one column: today's rule, verbatim


# ---- config keys ---------------------------------------------------------------------------------------------------------------------
def _ns(name, **kw):
    cfg = types.SimpleNamespace(config=name)
    vars(cfg).update(gconfig.get_config(name))
    vars(cfg).update(kw)
    return cfg


def test_options_default_and_entries():
    assert generator.prompt_options(_ns("StyleGAN2_ffhq_d")) is None
    assert generator.prompt_config(_ns("StyleGAN2_ffhq_d"), None).algorithm == "nsga2"
    feat = np.arange(4, dtype=np.float64)
    o = generator.prompt_options(_ns("StyleGAN2_ffhq_d", prompts=[("a hat", 0.5), (("image", "p.png"), -2), (feat, 1)]))
    assert o["mode"] == "sum"
    kinds = [(k, w) for k, _, w in o["entries"]]
    assert kinds == [("target", 1.0), ("text", 0.5), ("image", -2.0), ("feature", 1.0)]
    assert o["entries"][1][1] == "a hat" and o["entries"][2][1] == "p.png"
    assert o["entries"][3][1].dtype == np.float32 and o["entries"][3][1].tolist() == [0, 1, 2, 3]
    o = generator.prompt_options(_ns("DeepMindBigGAN256", target_weight=-3))
    assert o == dict(mode="sum", entries=[("target", None, -3.0)])


@pytest.mark.parametrize("kw,word", [
    (dict(prompts=[("x", 1)] * 16), "at most 16"),
    (dict(prompts=[("x", 0.0)]), "finite and non-zero"),
    (dict(prompts=[("x", float("nan"))]), "finite and non-zero"),
    (dict(prompts=[("x", float("inf"))]), "finite and non-zero"),
    (dict(target_weight=0), "target_weight"),
    (dict(prompts=["just a string"]), "pair"),
    (dict(prompt_mode="blend"), "expected one of"),
    (dict(prompt_mode="pareto"), "2 to 4 entries"),
    (dict(prompt_mode="pareto", prompts=[("x", 1)] * 4), "2 to 4 entries"),
    (dict(prompt_mode="pareto", prompts=[("x", 1)], lpips_target="t.png", lpips_lambda=0.5, lpips_weights="synthetic:1"), "lpips_lambda"),
])
def test_options_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        generator.prompt_options(_ns("StyleGAN2_ffhq_d", **kw))


@pytest.mark.parametrize("kw", [dict(prompts=[("x", 1)]), dict(prompt_mode="sum"), dict(target_weight=2.0)])
def test_gpt2_refuses_the_keys_before_any_weight_is_loaded(kw):
    with pytest.raises(ValueError, match="img2txt"):
        generator.prompt_options(_ns("GPT2", **kw))
    with pytest.raises(ValueError, match="img2txt"):
        generator.Generator(_ns("GPT2", **kw))             # no weights, no clip_weights: the refusal comes first


def test_refusal_comes_before_the_weights_on_a_gan_config():
    with pytest.raises(ValueError, match="2 to 4 entries"):
        generator.Generator(_ns("StyleGAN2_ffhq_d", prompt_mode="pareto"))


@pytest.mark.parametrize("name,K,lp,want", [
    ("StyleGAN2_ffhq_d", 2, None, 3), ("StyleGAN2_ffhq_nod", 2, None, 2), ("StyleGAN2_ffhq_d", 4, 0.0, 6), ("StyleGAN2_ffhq_nod", 3, 0.0, 4),
    ("DeepMindBigGAN256", 3, None, 3), ("DeepMindBigGAN256", 2, 0.0, 3),
])
def test_config_copy_of_a_pareto_set(name, K, lp, want):
    kw = dict(prompts=[(np.ones(4), 1.0)] * (K - 1), prompt_mode="pareto")
    if lp is not None:
        kw.update(lpips_target="t.png", lpips_lambda=lp, lpips_weights="synthetic:1")
    cfg = _ns(name, **kw)
    before = dict(cfg.problem_args)
    popts, lopts = generator.prompt_options(cfg), generator.lpips_options(cfg)
    out = generator.prompt_config(generator.lpips_config(cfg, lopts), popts)
    assert out is not cfg and out.problem_args["n_obj"] == want and out.algorithm == "nsga2"
    assert cfg.problem_args == before and gconfig.get_config(name)["problem_args"]["n_obj"] == before["n_obj"]
    names = run.objective_names(out)
    assert len(names) == want and names[:K] == ["similarity-%d" % t for t in range(K)]
    assert names[K:] == (["discriminator"] if name.endswith("_d") else []) + (["lpips"] if lp is not None else [])


def test_sum_mode_searches_the_config_as_it_is():
    cfg = _ns("StyleGAN2_ffhq_d", prompts=[("x", -1.0)])
    assert generator.prompt_config(cfg, generator.prompt_options(cfg)) is cfg
    assert run.objective_names(cfg) == ["similarity", "discriminator"]


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,want", [
    ("a hat", ("a hat", 1.0)), ("a hat::2", ("a hat", 2.0)), ("glasses::-0.5", ("glasses", -0.5)), ("a::b::3", ("a::b", 3.0)),
    ("std::vector", ("std::vector", 1.0)), ("x::1e-2", ("x", 0.01)), ("/p/q.png::-1", ("/p/q.png", -1.0)),
])
def test_weighted_text_parsing(text, want):
    assert generator.parse_weighted(text) == want


def test_flags():
    a = run.build_parser().parse_args([])
    assert a.prompt is None and a.image_prompt is None and a.target_weight is None and a.prompt_mode is None
    a = run.build_parser().parse_args(["--prompt", "a hat::2", "--prompt", "glasses::-1", "--image-prompt", "p.png::0.5", "--target-weight", "3",
                                       "--prompt-mode", "pareto"])
    assert a.prompt == ["a hat::2", "glasses::-1"] and a.image_prompt == ["p.png::0.5"] and a.target_weight == 3.0 and a.prompt_mode == "pareto"
    assert run.cli_prompts(a.prompt, a.image_prompt) == [("a hat", 2.0), ("glasses", -1.0), (("image", "p.png"), 0.5)]
    with pytest.raises(SystemExit):
        run.build_parser().parse_args(["--prompt-mode", "blend"])
    with pytest.raises(ValueError, match="img2txt"):       # refused by main before anything is loaded
        run.main(["--config", "GPT2", "--prompt", "x"])


# ---- the search surface ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("use_d", [False, True])
@pytest.mark.parametrize("lp", [False, True])
def test_names_scatters_and_final_pick(K, use_d, lp):
    kw = dict(prompts=[("x", 1.0)] * (K - 1), prompt_mode="pareto")
    if lp:
        kw.update(lpips_target="t.png", lpips_weights="synthetic:1")
    cfg = _ns("StyleGAN2_ffhq_d" if use_d else "StyleGAN2_ffhq_nod", **kw)
    out = generator.prompt_config(generator.lpips_config(cfg, generator.lpips_options(cfg)), generator.prompt_options(cfg))
    names = run.objective_names(out)
    n = K + use_d + lp
    assert names == ["similarity-%d" % t for t in range(K)] + ["discriminator"] * use_d + ["lpips"] * lp
    pairs = run.scatter_pairs(names)
    assert len(pairs) == n * (n - 1) // 2 and len(set(p[2] for p in pairs)) == len(pairs)
    if n == 2:
        assert pairs == [(0, 1, "F.jpg")]
    else:
        assert (0, 1, "F-similarity-0-similarity-1.jpg") in pairs
    w = run.final_pick_weights(names)
    assert len(w) == n and sum(w) == pytest.approx(1.0)
    if use_d or lp:
        assert w[:K] == [0.0] * K and w[K:] == [1.0 / (use_d + lp)] * (use_d + lp)
    else:
        assert w == [1.0 / K] * K


def test_final_pick_keeps_todays_rule():
    assert run.final_pick_weights(["similarity", "discriminator"]) == [0.0, 1.0]
    assert run.final_pick_weights(["similarity", "lpips"]) == [0.0, 1.0]
    assert run.final_pick_weights(["similarity", "discriminator", "lpips"]) == [0.0, 0.5, 0.5]
