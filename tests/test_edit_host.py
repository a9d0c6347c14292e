"""Host side of image editing (no GPU): glass_edit_supported and its messages, the n_obj bookkeeping for every combination of D / LPIPS
column / pareto K / anchor column (the library's rule, create, and the Generator's config copies), the refusals by name, the direction
entries built from features, the generation-0 sampler and its bounds, the column names and the flags."""
import ctypes as C
import types

import numpy as np
import pytest

from clip_glass_amd import config as gconfig
from clip_glass_amd import engine, generator, operators, problem, run


def test_symbols_are_exported():
    lib = engine.load_library()
    for name in ("glass_edit_supported", "glass_engine_set_anchor", "glass_engine_last_anchor", "glass_engine_set_direction_source",
                 "glass_engine_last_direction_source", "glass_op_cosine_set_dir", "glass_op_latent_anchor"):
        assert hasattr(lib, name), name


def test_config_struct_appends_the_fields_last():
    G = engine.GlassConfig
    names = [f[0] for f in G._fields_]
    assert len(names) == 38 and names[29:31] == ["clip_resize", "clip_normalize"]
    assert names[31:] == ["clip_arch", "clip_rn_layers", "lpips_size", "lpips_lambda", "sim_columns", "anchor", "anchor_lambda"]
    assert G.sim_columns.offset == 392                                            # nothing before them moved
    assert (G.anchor.offset, G.anchor_lambda.offset) == (396, 400)
    assert C.sizeof(G) == 408      # (400 at 8-byte alignment without the two fields: they fill 8, and the struct ends on 4 bytes of padding)
    cfg = G()
    assert cfg.anchor == 0 and cfg.anchor_lambda == 0.0


# ---- the library's rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 2, 4])
@pytest.mark.parametrize("use_d", [False, True])
@pytest.mark.parametrize("lp_col", [False, True])
@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_n_obj_rule_for_every_combination(K, use_d, lp_col, lam):
    want = max(K, 1) + use_d + lp_col + (lam == 0.0)
    assert engine.edit_n_obj(K, use_d, lp_col, True, lam) == want
    assert engine.edit_n_obj(K, use_d, lp_col, False, 0.0) == engine.prompt_n_obj(K, use_d, lp_col)      # no anchor: what it was
    ok, msg = engine.edit_supported("stylegan2", 4, K, use_d, lp_col, True, lam, want)
    if K >= 2 and lam > 0:
        assert not ok and "no single one" in msg
        return
    assert (ok, msg) == (True, "")
    for wrong in (want - 1, want + 1):
        ok, msg = engine.edit_supported("stylegan2", 4, K, use_d, lp_col, True, lam, wrong)
        assert not ok and "n_obj must be max(sim_columns, 1) + use_discriminator + (lpips own column) + (anchor_lambda == 0) = %d, got %d" % (want, wrong) in msg


def test_rule_messages():
    assert engine.edit_supported("stylegan2", 4, 0, True, False, False, 0.0, 2) == (True, "")
    assert engine.edit_supported("biggan", 0, 0, False, False, False, 0.0, 1) == (True, "")          # anchor off: nothing is said about n_obj
    assert engine.edit_supported(None, 0, 0, False, False, False, 0.0, 7) == (True, "")
    for args, word in [
        (("biggan", 0, 0, False, False, True, 0.0, 2), "BigGAN-deep engine has none"),
        ((None, 0, 0, False, False, True, 0.0, 2), "no generator (GPT-2 / img2txt)"),
        (("stylegan2", 4, 0, False, False, False, 0.5, 1), "anchor is 0"),
        (("stylegan2", 4, 0, False, False, True, -1.0, 1), "finite and >= 0"),
        (("stylegan2", 4, 0, False, False, True, float("nan"), 1), "finite and >= 0"),
        (("stylegan2", 4, 0, False, False, 2, 0.0, 2), "anchor must be 0 (off) or 1"),
    ]:
        ok, msg = engine.edit_supported(*args)
        assert not ok and word in msg, (args, msg)


def _create(**kw):
    """glass_engine_create on the mini geometry: the rules sit in front of the device lookup, so a refusal needs no GPU."""
    kw.setdefault("mbstd_group", 2)
    return engine.Engine([16, 16, 32, 32], latent_size=32, mapping_layers=2, batch_size=2, clip=(64, 2, 1, 8, 32, 32), **kw)


def _refusal(**kw):
    try:
        _create(**kw).close()
        return ""
    except RuntimeError as ex:
        return str(ex)


def test_create_applies_the_rule():
    assert "n_obj must be max(sim_columns, 1)" in _refusal(use_discriminator=True, n_obj=2, anchor=True)
    assert "n_obj must be max(sim_columns, 1)" in _refusal(use_discriminator=False, n_obj=1, anchor=True)
    assert "n_obj must be max(sim_columns, 1)" in _refusal(use_discriminator=True, n_obj=3, anchor=True, anchor_lambda=0.5)
    assert "no single one" in _refusal(use_discriminator=False, n_obj=2, sim_columns=2, anchor=True, anchor_lambda=0.5)
    assert "anchor is 0" in _refusal(use_discriminator=True, n_obj=2, anchor=False, anchor_lambda=0.5)
    for kw in (dict(use_discriminator=True, n_obj=3, anchor=True), dict(use_discriminator=False, n_obj=2, anchor=True),
               dict(use_discriminator=True, n_obj=2, anchor=True, anchor_lambda=0.5), dict(use_discriminator=True, n_obj=4, anchor=True, lpips_size=32),
               dict(use_discriminator=True, n_obj=4, sim_columns=2, anchor=True), dict(use_discriminator=True, n_obj=2)):
        msg = _refusal(**kw)
        assert "n_obj" not in msg and "anchor" not in msg, (kw, msg)      # accepted: on to the device lookup (which fails on a machine without one)
    bg = dict(layers=[(0, 16, 16), (1, 16, 1)], attention_pos=1, ch=64, z_dim=16, num_classes=24)
    with pytest.raises(RuntimeError, match="BigGAN-deep engine has none"):
        engine.Engine([], batch_size=2, max_pop=4, clip=(64, 2, 1, 8, 32, 32), biggan=bg, anchor=True)
    with pytest.raises(RuntimeError, match="no generator"):
        engine.Engine([], latent_size=4, mapping_layers=0, batch_size=1, use_discriminator=False, n_obj=2, clip=(64, 2, 1, 8, 32, 32), anchor=True)


# ---- config keys -------------------------------------------------------------------------------------------------------------------
def _ns(name, **kw):
    cfg = types.SimpleNamespace(config=name)
    vars(cfg).update(gconfig.get_config(name))
    vars(cfg).update(kw)
    return cfg


ROW = np.linspace(-1, 1, 512).astype(np.float32)


def test_options_default_and_values():
    assert generator.edit_options(_ns("StyleGAN2_ffhq_d")) is None
    assert generator.edit_config(_ns("StyleGAN2_ffhq_d"), None).problem_args["n_obj"] == 2
    o = generator.edit_options(_ns("StyleGAN2_ffhq_d", edit_latent=ROW, source_text="a face"))
    assert o["anchor"] and o["anchor_column"] and o["lam"] == 0.0 and o["sigma"] == generator.DEFAULT_EDIT_SIGMA and o["image"] is None
    o = generator.edit_options(_ns("StyleGAN2_ffhq_d", edit_latent=ROW, source_text="a face", anchor_lambda=0.25, edit_sigma=0.5))
    assert o["anchor"] and not o["anchor_column"] and o["lam"] == 0.25 and o["sigma"] == 0.5
    o = generator.edit_options(_ns("DeepMindBigGAN256", edit_image="p.png", source_text="a dog"))
    assert not o["anchor"] and not o["anchor_column"] and o["image"] == "p.png" and o["source_text"] == "a dog"


@pytest.mark.parametrize("name,kw,word", [
    ("GPT2", dict(edit_image="p.png"), "edit_image: image editing moves generated images"),
    ("GPT2", dict(edit_latent=ROW), "edit_latent: image editing"),
    ("GPT2", dict(source_text="x"), "source_text: image editing"),
    ("GPT2", dict(anchor_lambda=0.1), "anchor_lambda: image editing"),
    ("GPT2", dict(edit_sigma=0.1), "edit_sigma: image editing"),
    ("DeepMindBigGAN256", dict(edit_latent=ROW, source_text="x"), "edit_latent: the latent anchor is a distance between dlatents"),
    ("DeepMindBigGAN512", dict(edit_image="p.png", source_text="x", anchor_lambda=0.1), "anchor_lambda: the latent anchor"),
    ("StyleGAN2_ffhq_d", dict(edit_image="p.png"), "source_text is required with edit_image"),
    ("StyleGAN2_ffhq_d", dict(edit_latent=ROW), "source_text is required with edit_latent"),
    ("StyleGAN2_ffhq_d", dict(edit_latent=ROW, source_text="  "), "source_text is required"),
    ("StyleGAN2_ffhq_d", dict(source_text="a face"), "set without a source"),
    ("StyleGAN2_ffhq_d", dict(edit_image="p.png", source_text="x", anchor_lambda=0.1), "anchor_lambda set without edit_latent"),
    ("StyleGAN2_ffhq_d", dict(edit_image="p.png", source_text="x", edit_sigma=0.1), "edit_sigma set without edit_latent"),
    ("StyleGAN2_ffhq_d", dict(edit_latent=ROW, source_text="x", anchor_lambda=-1), "anchor_lambda must be finite and >= 0"),
    ("StyleGAN2_ffhq_d", dict(edit_latent=ROW, source_text="x", edit_sigma=0), "edit_sigma must be finite and > 0"),
    ("StyleGAN2_ffhq_d", dict(edit_latent=ROW, source_text="x", anchor_lambda=0.5, prompt_mode="pareto", prompts=[("a hat", 1)]),
     "anchor_lambda > 0 with prompt_mode 'pareto'"),
])
def test_refusals_by_name(name, kw, word):
    with pytest.raises(ValueError, match=word.replace("(", r"\(")):
        generator.edit_options(_ns(name, **kw))


def test_generator_refuses_before_an_engine_is_built(monkeypatch):
    built = []
    monkeypatch.setattr(generator, "Engine", lambda *a, **k: built.append(1))
    for name, kw in (("GPT2", dict(edit_image="p.png")), ("DeepMindBigGAN256", dict(edit_latent=ROW, source_text="x"))):
        cfg = _ns(name, **kw)
        cfg.model = lambda c: built.append("model")
        with pytest.raises(ValueError):
            generator.Generator(cfg)
    assert built == []
    with pytest.raises(ValueError, match="GPT2"):
        run.main(["--config", "GPT2", "--edit-image", "p.png", "--source-text", "a photo"])


@pytest.mark.parametrize("use_d", [False, True])
@pytest.mark.parametrize("lp,lp_lam", [(False, 0.0), (True, 0.0), (True, 0.5)])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("an_lam", [None, 0.0, 0.5])
def test_config_copies_count_the_columns(use_d, lp, lp_lam, K, an_lam):
    """The chain the Generator applies — lpips_config, prompt_config, edit_config — against the library's rule."""
    kw = {}
    if lp:
        kw.update(lpips_target="t.png", lpips_lambda=lp_lam, lpips_weights="synthetic:0")
    if K >= 2:
        kw.update(prompt_mode="pareto", prompts=[("p%d" % i, 1.0) for i in range(K - 1)])
    if an_lam is not None:
        kw.update(edit_latent=ROW, source_text="a face", anchor_lambda=an_lam)
    cfg = _ns("StyleGAN2_ffhq_d" if use_d else "StyleGAN2_ffhq_nod", **kw)
    base = dict(cfg.problem_args)
    try:
        lpo, pro, edo = generator.lpips_options(cfg), generator.prompt_options(cfg), generator.edit_options(cfg)
    except ValueError as ex:
        assert K >= 2 and ((lp and lp_lam > 0) or (an_lam or 0) > 0), ex      # a fold with a front: refused by name
        return
    out = generator.edit_config(generator.prompt_config(generator.lpips_config(cfg, lpo), pro), edo)
    lp_col, an = lp and lp_lam == 0.0, an_lam is not None
    want = engine.edit_n_obj(K if K >= 2 else 0, use_d, lp_col, an, an_lam or 0.0)
    assert out.problem_args["n_obj"] == want
    assert cfg.problem_args == base and gconfig.get_config(cfg.config)["problem_args"]["n_obj"] == (2 if use_d else 1)      # the table is not touched
    if an:
        assert engine.edit_supported("stylegan2", 9, K if K >= 2 else 0, use_d, lp_col, True, an_lam, want) == (True, "")
    if want > base["n_obj"]:
        assert out.algorithm == "nsga2"
    names = run.objective_names(out)
    assert len(names) == want and (names[-1] == "anchor") == (an and an_lam == 0.0) and ("discriminator" in names) == use_d
    weights = run.final_pick_weights(names)
    rest = [w for n, w in zip(names, weights) if not n.startswith("similarity")]
    assert abs(sum(weights) - 1) < 1e-12 and len(set(rest)) <= 1 and (not rest or all(w == 0 for n, w in zip(names, weights) if n.startswith("similarity")))


def test_scatter_files_name_the_anchor():
    assert run.scatter_pairs(["similarity", "anchor"]) == [(0, 1, "F.jpg")]
    files = [f for _, _, f in run.scatter_pairs(["similarity", "discriminator", "anchor"])]
    assert files == ["F-similarity-discriminator.jpg", "F-similarity-anchor.jpg", "F-discriminator-anchor.jpg"]
    assert run.final_pick_weights(["similarity", "discriminator", "lpips", "anchor"]) == [0.0, 1 / 3, 1 / 3, 1 / 3]


# ---- directions --------------------------------------------------------------------------------------------------------------------
def test_direction_entries_from_features():
    rng = np.random.default_rng(0)
    feats = rng.standard_normal((3, 16)) * np.array([[1.0], [7.0], [0.1]])
    src_t, src_i = rng.standard_normal(16) * 3, rng.standard_normal(16) * 0.2
    d = generator.edit_directions(feats, ["target", "image", "text"], src_t, src_i)
    assert d.dtype == np.float32 and d.shape == (3, 16)
    unit = lambda v: v / np.linalg.norm(v)
    for t, base in enumerate((src_t, src_i, src_t)):
        want = unit(unit(feats[t]) - unit(base))
        np.testing.assert_allclose(d[t], want, atol=1e-7)
    np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # scale of either side does not matter: both are taken at unit length
    np.testing.assert_allclose(generator.edit_directions(feats * 5, ["target", "image", "text"], src_t * 0.3, src_i * 11), d, atol=1e-6)
    with pytest.raises(ValueError, match=r"prompt 0 \(target\) is the same as its source \(source_text\)"):
        generator.edit_directions(feats[:1], ["target"], feats[0] * 2, src_i)
    with pytest.raises(ValueError, match=r"prompt 1 \(image\) is the same as its source \(the source image\)"):
        generator.edit_directions(feats[:2], ["target", "image"], src_t, feats[1])


def test_edit_latent_is_one_finite_row(tmp_path):
    np.save(str(tmp_path / "row.npy"), ROW[None])
    assert generator.load_edit_latent(str(tmp_path / "row.npy")).shape == (512,)
    assert generator.load_edit_latent(list(ROW)).dtype == np.float32
    for bad in (np.zeros((2, 8)), np.array([1.0, np.nan]), np.zeros((1, 2, 3))):
        with pytest.raises(ValueError, match="ONE finite row"):
            generator.load_edit_latent(bad)


# ---- generation 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xl,xu", [(-10.0, 10.0), (-0.5, 0.25)])
def test_generation_zero_starts_at_the_source_inside_the_bounds(xl, xu):
    lo, hi = problem.edit_bounds(xl, xu, ROW)
    assert lo <= ROW.min() and hi >= ROW.max() and lo <= xl and hi >= xu
    assert (lo, hi) == ((xl, xu) if xl <= -1 else (-1.0, 1.0))       # widened only as far as the source needs
    P = types.SimpleNamespace(n_var=512, xl=np.full(512, lo), xu=np.full(512, hi))
    s = operators.EditSampling(ROW, 0.4)
    np.random.seed(3)
    X = s._do(P, 16)
    assert X.shape == (16, 512)
    np.testing.assert_array_equal(X[0], ROW.astype(np.float64))      # row 0 IS the source, bit for bit as float32
    assert (X >= lo).all() and (X <= hi).all()
    assert (np.abs(X[1:] - ROW).max(axis=1) > 0.1).all() and len({r.tobytes() for r in X}) == 16
    if xl <= -1:
        assert 0.3 < (X[1:] - ROW).std() < 0.5                       # sigma
    else:
        assert (X[1:] == hi).any() and (X[1:] == lo).any()           # clipped at the widened bounds
    again = s._do(P, 5)                                              # a refill after duplicate elimination: no second copy of the source
    assert again.shape == (5, 512) and not (again == ROW).all(axis=1).any()
    with pytest.raises(ValueError, match="holds 512 floats; the search varies 64"):
        operators.EditSampling(ROW, 0.4)._do(types.SimpleNamespace(n_var=64, xl=lo, xu=hi), 4)


def test_operators_start_at_the_source_in_every_space():
    for space in (None, "w", "w+"):
        ops = operators.get_operators(_ns("StyleGAN2_ffhq_d", latent_space=space, edit_latent=ROW, edit_sigma=0.3))
        assert isinstance(ops["sampling"], operators.EditSampling) and ops["sampling"].sigma == 0.3
    assert operators.get_operators(_ns("StyleGAN2_ffhq_d", edit_latent=ROW))["sampling"].sigma == generator.DEFAULT_EDIT_SIGMA
    assert isinstance(operators.get_operators(_ns("StyleGAN2_ffhq_d"))["sampling"], operators.NormalRandomSampling)


# ---- flags -------------------------------------------------------------------------------------------------------------------------
def test_cli_parsing():
    p = run.build_parser()
    a = p.parse_args([])
    assert all(getattr(a, k) is None for k in generator.EDIT_KEYS)
    a = p.parse_args(["--edit-image", "face.png", "--edit-latent", "w.npy", "--source-text", "a face", "--anchor-lambda", "0.25", "--edit-sigma", "0.05"])
    assert (a.edit_image, a.edit_latent, a.source_text, a.anchor_lambda, a.edit_sigma) == ("face.png", "w.npy", "a face", 0.25, 0.05)
    with pytest.raises(ValueError, match="source_text is required with edit_image"):
        run.main(["--config", "StyleGAN2_ffhq_d", "--edit-image", "face.png"])
    with pytest.raises(ValueError, match="edit_latent: the latent anchor"):
        run.main(["--config", "DeepMindBigGAN256", "--edit-latent", "w.npy", "--source-text", "a dog"])
