"""The opt-in CLIP preprocessing (config.clip_preprocess / --clip-preprocess; glass_config.clip_resize, clip_normalize): host side, no GPU.

* glass_host_resize_taps (include/glass_ops.h): the tap table finalize() builds for the antialiased resize, against torch's own
  F.interpolate(antialias=True) in float64.
* glass_clip_preprocess_supported / glass_engine_create (include/glass.h): what is refused, and why.
* the flag, the names and how Generator hands them to every Engine it builds.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clip_glass_amd import config as gconfig, engine, generator, ops, synth

PAIRS = [(1024, 224), (1024, 336), (512, 224), (256, 224), (128, 224), (64, 32), (32, 32)]
MODES = {1: "bilinear", 2: "bicubic"}


def tap_matrix(R, S, mode):
    start, count, taps = ops.host_resize_taps(R, S, mode)
    W = np.zeros((S, R), np.float64)
    for i in range(S):
        W[i, start[i]:start[i] + count[i]] = taps[i, :count[i]]
    return W, start, count, taps


# ---- the tap tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("R,S", PAIRS)
def test_tap_tables_reproduce_torch(R, S, mode):
    """W x W^T in float64 against torch.  Bar 1e-6 * max|ref|: the taps are fp32 roundings (2^-24 relative each) of the float64 weights, the
    separable resize applies them twice, and a row's sum of |w| is at most 1.26 (bicubic) — about 1e-7 expected."""
    W, _, _, _ = tap_matrix(R, S, mode)
    x = torch.tensor(synth.normal(31, "pp%d_%d" % (R, S), (2, 3, R, R))).double().sigmoid()
    ref = F.interpolate(x, (S, S), mode=MODES[mode], align_corners=False, antialias=True).numpy()
    got = W @ x.numpy() @ W.T
    err = np.abs(got - ref).max()
    print("taps %d -> %d %s: max err %.3e (bar %.3e)" % (R, S, MODES[mode], err, 1e-6 * np.abs(ref).max()))
    assert err <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("R,S", PAIRS)
def test_tap_rows_sum_to_one_and_fit(R, S, mode):
    W, start, count, taps = tap_matrix(R, S, mode)
    assert np.abs(W.sum(1) - 1.0).max() <= 1e-6
    assert count.min() >= 1 and count.max() <= ops.RESIZE_MAX_TAPS
    assert start.min() >= 0 and (start + count).max() <= R
    assert (np.diff(start) >= 0).all()
    for i in range(S):                                   # nothing past a row's count
        assert not taps[i, count[i]:].any()


def test_widest_rows():
    assert tap_matrix(1024, 224, 2)[2].max() == 19
    assert tap_matrix(1024, 336, 2)[2].max() == 13
    assert tap_matrix(1024, 224, 1)[2].max() == 10


@pytest.mark.parametrize("mode", sorted(MODES))
def test_same_size_is_the_identity(mode):
    W, _, _, _ = tap_matrix(32, 32, mode)
    np.testing.assert_array_equal(W, np.eye(32))


def test_caller_buffer_too_narrow_is_refused():
    with pytest.raises(RuntimeError, match="19 taps"):
        ops.host_resize_taps(1024, 224, 2, max_taps=16)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    lib = engine.load_library()
    for name in ("glass_clip_preprocess_supported", "glass_host_resize_taps", "glass_op_preprocess"):
        assert hasattr(lib, name), name


def test_supported_pairs():
    for R, S in PAIRS + [(200, 224)]:
        for rz in (0, 1, 2):
            for nm in (0, 1):
                ok, msg = engine.clip_preprocess_supported(R, S, rz, nm)
                assert ok and msg == "", (R, S, rz, nm, msg)
    assert engine.clip_preprocess_supported(0, 224, 0, 0)[0]           # an engine without a generator


@pytest.mark.parametrize("args,word", [
    ((1024, 224, 3, 0), "clip_resize"),
    ((1024, 224, -1, 0), "clip_resize"),
    ((1024, 224, 0, 2), "clip_normalize"),
    ((1024, 224, 2, -1), "clip_normalize"),
    ((1024, 112, 2, 0), "taps"),          # 9.14 x bicubic: 37 taps
    ((1024, 32, 1, 0), "taps"),           # 32 x bilinear: 65 taps
    ((2048, 224, 1, 0), "at most 1024"),
])
def test_unsupported_say_why(args, word):
    ok, msg = engine.clip_preprocess_supported(*args)
    assert not ok and word in msg, msg


def _create(**kw):
    """glass_engine_create on the mini geometry (64 px would be n_blocks 5; here 4 blocks = 32 px, CLIP at 32 px)."""
    return engine.Engine([16, 16, 32, 32], latent_size=32, mapping_layers=2, clip=(64, 2, 1, 8, 32, 32), **kw)


@pytest.mark.parametrize("kw,word", [
    (dict(clip_resize=3), "clip_resize"),
    (dict(clip_resize=-1), "clip_resize"),
    (dict(clip_normalize=2), "clip_normalize"),
])
def test_engine_create_refuses_out_of_range_fields(kw, word):
    """The check sits in front of the device lookup, so the refusal needs no GPU."""
    with pytest.raises(RuntimeError) as ei:
        _create(**kw)
    assert word in str(ei.value) and "no such HIP device" not in str(ei.value)


def test_engine_create_refuses_an_over_wide_ratio():
    # 1024 px generator (9 blocks) scored by a 32 px tower: a 32 x down-scale, 65 (bilinear) / 129 (bicubic) taps
    ch = [16] * 9
    for rz in (1, 2):
        with pytest.raises(RuntimeError, match="taps"):
            engine.Engine(ch, latent_size=32, mapping_layers=2, clip=(64, 2, 1, 8, 32, 32), clip_resize=rz)


def test_config_struct_ends_with_the_new_fields():
    names = [f[0] for f in engine.GlassConfig._fields_]
    assert names[29:31] == ["clip_resize", "clip_normalize"]                      # the end of the struct when they were appended; later fields follow
    assert (engine.GlassConfig.clip_resize.offset, engine.GlassConfig.clip_normalize.offset) == (356, 360)
    assert engine.GlassConfig().clip_resize == 0 and engine.GlassConfig().clip_normalize == 0


# ---- the flag, the names, the plumbing ---------------------------------------------------------------------------------------
def test_names():
    assert generator.CLIP_PREPROCESS == {"reference": (0, 0), "antialias": (1, 0), "clip": (2, 1)}
    assert generator.clip_preprocess_fields(None) == (0, 0)
    for name, pair in generator.CLIP_PREPROCESS.items():
        assert generator.clip_preprocess_fields(name) == pair
    with pytest.raises(ValueError) as ei:
        generator.clip_preprocess_fields("lanczos")
    for name in generator.CLIP_PREPROCESS:
        assert name in str(ei.value)


def test_cli_flag():
    from clip_glass_amd import run
    p = run.build_parser()
    for name in ("reference", "antialias", "clip"):
        assert p.parse_args(["--clip-preprocess", name]).clip_preprocess == name
    assert p.parse_args([]).clip_preprocess is None
    with pytest.raises(SystemExit):
        p.parse_args(["--clip-preprocess", "lanczos"])


class FakeEngine:
    made = []

    def __init__(self, channels, **kw):
        self.kw = kw
        self.cfg = types.SimpleNamespace(n_obj=kw.get("n_obj", 2))
        FakeEngine.made.append(self)

    def load_state(self, sd): pass
    def finalize(self): pass
    def set_target(self, t): pass


def _txt2img_config(name, **kw):
    cfg = types.SimpleNamespace(config=name, device="cuda:0", target="unused")
    vars(cfg).update(gconfig.get_config(name))
    vars(cfg).update(weights="synthetic:0", clip_weights="synthetic:0", clip_geometry=(64, 2, 1, 8, 32, 32),
                     target_features=np.ones(32, np.float32))
    vars(cfg).update(kw)
    return cfg


@pytest.mark.parametrize("name,pair", [(None, (0, 0)), ("reference", (0, 0)), ("antialias", (1, 0)), ("clip", (2, 1))])
def test_generator_hands_the_fields_to_the_stylegan2_engine(monkeypatch, name, pair):
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    cfg = _txt2img_config("StyleGAN2_ffhq_d", channels=[16, 16, 32, 32], dim_z=32, mapping_layers=2)
    cfg.problem_args = dict(cfg.problem_args, n_var=32, n_constr=32)
    if name is not None:
        cfg.clip_preprocess = name
    g = generator.Generator(cfg)
    assert g.clip_preprocess == (name or "reference")
    assert len(FakeEngine.made) == 1
    kw = FakeEngine.made[0].kw
    assert (kw["clip_resize"], kw["clip_normalize"]) == pair


def test_generator_hands_the_fields_to_the_biggan_engine(monkeypatch):
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    geometry = dict(layers=[(0, 16, 16), (1, 16, 8), (1, 8, 4), (0, 4, 4), (1, 4, 2), (1, 2, 1)], attention_pos=3, ch=64, z_dim=16,
                    num_classes=24)
    cfg = _txt2img_config("DeepMindBigGAN256", clip_preprocess="clip",
                          model=lambda c: types.SimpleNamespace(geometry=geometry, state={}))
    generator.Generator(cfg)
    kw = FakeEngine.made[0].kw
    assert kw["biggan"] is geometry and (kw["clip_resize"], kw["clip_normalize"]) == (2, 1)


def test_generator_refuses_an_unknown_name_before_the_engine(monkeypatch):
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    cfg = _txt2img_config("StyleGAN2_ffhq_d", channels=[16, 16, 32, 32], dim_z=32, mapping_layers=2, clip_preprocess="lanczos")
    with pytest.raises(ValueError, match="reference, antialias, clip"):
        generator.Generator(cfg)
    assert not FakeEngine.made


def test_img2txt_refuses_the_setting(monkeypatch):
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    cfg = types.SimpleNamespace(task="img2txt", model=lambda c: types.SimpleNamespace(state={}), pop_size=4, batch_size=4,
                                clip_weights="synthetic:0", clip_geometry=(64, 2, 1, 8, 32, 32), clip_preprocess="clip")
    with pytest.raises(ValueError, match="img2txt"):
        generator.Generator(cfg)
    assert not FakeEngine.made


def test_run_copies_the_flag_into_the_config(monkeypatch):
    from clip_glass_amd import run
    seen = {}

    class Stop(Exception):
        pass

    def problem(config, dist=None):
        seen["clip_preprocess"] = getattr(config, "clip_preprocess", None)
        seen["clip_model"] = getattr(config, "clip_model", None)
        raise Stop()
    monkeypatch.setattr(run, "GenerationProblem", problem)
    with pytest.raises(Stop):
        run.main(["--config", "StyleGAN2_ffhq_nod", "--clip-preprocess", "clip", "--clip-model", "ViT-B/16"])
    assert seen == dict(clip_preprocess="clip", clip_model="ViT-B/16")
    with pytest.raises(Stop):
        run.main(["--config", "StyleGAN2_ffhq_nod"])
    assert seen["clip_preprocess"] is None
