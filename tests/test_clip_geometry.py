"""Which CLIP image towers the engine accepts, and how a model is chosen (no GPU needed).

* glass_clip_geometry_supported (include/glass.h): the host-only rule glass_engine_create applies.
* generator.CLIP_MODELS / config.clip_model: named geometries, selection for synthetic weights, the mismatch error.
* the oracle's encode_image pinned to the reference's VisualTransformer at patch 16 and patch 14 (it was pinned at patch 8 only:
  tests/test_oracle_vs_reference.py) — live where the reference is present, else against tests/golden/clip_tower_pins.npz
  (tests/golden/make_clip_tower_pins.py).
"""
import os
import types

import numpy as np
import pytest
import torch

import ref_harness as rh
from clip_glass_amd import engine, generator, synth
from oracle import clip_ref

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_tower_pins.npz")
NAMED = {
    "ViT-B/32": ((768, 12, 12, 32, 224, 512), dict(width=512, layers=12)),
    "ViT-B/16": ((768, 12, 12, 16, 224, 512), dict(width=512, layers=12)),
    "ViT-L/14": ((1024, 24, 16, 14, 224, 768), dict(width=768, layers=12)),
    "ViT-L/14@336": ((1024, 24, 16, 14, 336, 768), dict(width=768, layers=12)),
}
ORACLE_CASES = [(16, 64), (14, 56)]


# ---- the library's rule ------------------------------------------------------------------------------------------------------
def test_symbol_is_exported():
    lib = engine.load_library()
    assert hasattr(lib, "glass_clip_geometry_supported")


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_geometries_are_supported(name):
    ok, msg = engine.clip_geometry_supported(NAMED[name][0])
    assert ok and msg == "", (name, msg)


def test_test_geometries_are_supported():
    for geom in ((64, 2, 1, 8, 32, 32), (128, 2, 2, 8, 32, 64)):      # tests/glass_models.py mini / mid
        assert engine.clip_geometry_supported(geom)[0]


@pytest.mark.parametrize("geom,word", [
    ((768, 12, 8, 32, 224, 512), "head dim"),          # head dim 96
    ((512, 12, 16, 32, 224, 512), "head dim"),         # head dim 32
    ((768, 12, 12, 32, 225, 512), "multiple of patch"),
    ((1024, 24, 16, 14, 230, 768), "multiple of patch"),
])
def test_unsupported_geometries_say_why(geom, word):
    ok, msg = engine.clip_geometry_supported(geom)
    assert not ok
    assert msg and word in msg, msg
    lib = engine.load_library()
    assert lib.glass_clip_geometry_supported(*geom) != 0 and lib.glass_last_error().decode() == msg


# ---- the named table and its selection ---------------------------------------------------------------------------------------
def test_named_table():
    assert set(generator.CLIP_MODELS) == set(NAMED)
    for name, (geom, text) in NAMED.items():
        assert tuple(generator.CLIP_MODELS[name]) == geom
        assert generator.clip_model_geometry(name) == geom
        assert generator.clip_model_name(geom) == name
        assert dict(generator.CLIP_TEXT_MODELS[name]) == text
        assert geom[0] // geom[2] == 64
    assert generator.CLIP_MODELS["ViT-B/32"] == generator.CLIP_VIT_B32
    assert generator.clip_model_name((768, 12, 12, 8, 224, 512)) is None
    with pytest.raises(ValueError, match="ViT-B/16"):
        generator.clip_model_geometry("ViT-H/14")


def _one_layer_state(name, with_text=False):
    """A 1-layer cut of a named geometry: every shape of the full model except the depth."""
    w, _, _, patch, res, embed = NAMED[name][0]
    sd = synth.make_state(synth.clip_visual_spec(w, 1, patch, res, embed), 0)
    if with_text:
        sd.update(synth.make_state(synth.clip_text_spec(width=NAMED[name][1]["width"], layers=1, vocab=64, out_dim=embed), 0))
    return sd


@pytest.mark.parametrize("name", sorted(NAMED))
def test_geometry_from_state_one_layer_cut(name):
    geom = NAMED[name][0]
    got = generator.clip_geometry_from_state(_one_layer_state(name, with_text=True))
    assert got == (geom[0], 1, geom[2], geom[3], geom[4], geom[5])
    assert engine.clip_geometry_supported(got)[0]


def _synthetic_config(**kw):
    return types.SimpleNamespace(clip_weights="synthetic:3", **kw)


def test_clip_model_selects_synthetic_geometry(monkeypatch):
    seen = []
    real = synth.make_state

    def one_layer(spec, seed):       # keep the shapes, not the depth: the full ViT-L is 300 M values
        seen.append([s for s in spec if ".resblocks." not in s[0] or ".resblocks.0." in s[0]])
        return real(seen[-1], seed)
    monkeypatch.setattr(synth, "make_state", one_layer)
    state, geom = generator._load_clip_state(_synthetic_config(), False)
    assert geom == NAMED["ViT-B/32"][0]                                  # the default
    for name, (want, text) in NAMED.items():
        state, geom = generator._load_clip_state(_synthetic_config(clip_model=name), True)
        assert geom == want
        assert state["clip.visual.conv1.weight"].shape == (want[0], 3, want[3], want[3])
        assert state["clip.visual.positional_embedding"].shape == ((want[4] // want[3]) ** 2 + 1, want[0])
        assert state["clip.visual.proj"].shape == (want[0], want[5])
        assert state["clip.token_embedding.weight"].shape[1] == text["width"]
        assert state["clip.text_projection"].shape == (text["width"], want[5])
    # an explicit geometry wins over the name, as before the names existed
    mini = (64, 2, 1, 8, 32, 32)
    state, geom = generator._load_clip_state(_synthetic_config(clip_model="ViT-L/14", clip_geometry=mini), False)
    assert geom == mini and state["clip.visual.conv1.weight"].shape == (64, 3, 8, 8)
    with pytest.raises(ValueError, match="unknown CLIP model"):
        generator._load_clip_state(_synthetic_config(clip_model="RN50"), False)


def _write_checkpoint(path, name):
    sd = {k[len("clip."):]: torch.as_tensor(v) for k, v in _one_layer_state(name).items()}
    # the depth is part of the geometry: a 1-layer cut is only "the named model" up to that, so the file carries all layers' keys
    layers = NAMED[name][0][1]
    for k in [k for k in sd if ".resblocks.0." in k]:
        for i in range(1, layers):
            sd[k.replace(".resblocks.0.", ".resblocks.%d." % i)] = sd[k][:1] if k.endswith("in_proj_weight") else sd[k].new_zeros(1)
    torch.save(sd, path)


def test_checkpoint_geometry_wins_and_mismatch_names_both(tmp_path):
    path = str(tmp_path / "vit_b16.pt")
    _write_checkpoint(path, "ViT-B/16")
    cfg = types.SimpleNamespace(clip_weights=path)
    state, geom = generator._load_clip_state(cfg, False)
    assert geom == NAMED["ViT-B/16"][0]                                  # from the state dict, no name given
    cfg.clip_model = "ViT-B/16"
    assert generator._load_clip_state(cfg, False)[1] == NAMED["ViT-B/16"][0]
    cfg.clip_model = "ViT-B/32"
    with pytest.raises(ValueError) as ei:
        generator._load_clip_state(cfg, False)
    assert "ViT-B/32" in str(ei.value) and "ViT-B/16" in str(ei.value)


def test_generator_refuses_unsupported_geometry_before_the_engine():
    with pytest.raises(ValueError, match="head dim must be 64"):
        generator.check_clip_geometry((768, 12, 8, 32, 224, 512))
    generator.check_clip_geometry(NAMED["ViT-L/14@336"][0])


def test_cli_flag():
    from clip_glass_amd import run
    p = run.build_parser()
    assert p.parse_args(["--clip-model", "ViT-L/14@336"]).clip_model == "ViT-L/14@336"
    assert p.parse_args([]).clip_model is None
    with pytest.raises(SystemExit):
        p.parse_args(["--clip-model", "RN50"])


# ---- the oracle at other patch sizes -----------------------------------------------------------------------------------------
def pin_name(patch, res):
    return "image_p%d_r%d" % (patch, res)


def _oracle_inputs(patch, res):
    sd = synth.make_state(synth.clip_visual_spec(width=128, layers=2, patch=patch, res=res, out_dim=64), 8)
    sd.update(synth.make_state(synth.clip_text_spec(width=64, layers=1, ctx=8, vocab=64, out_dim=64), 8))   # build_model wants both towers
    return sd, torch.tensor(synth.normal(9, "img%d" % patch, (3, 3, res, res))).sigmoid()


def ref_encode_image(patch, res):
    sd, img = _oracle_inputs(patch, res)
    model = rh.build_ref_clip(sd)
    assert model.visual.conv1.kernel_size == (patch, patch) and model.visual.input_resolution == res
    with torch.no_grad():
        return model.encode_image(img).numpy()


@pytest.mark.parametrize("patch,res", ORACLE_CASES)
def test_oracle_encode_image_matches_reference(patch, res):
    sd, img = _oracle_inputs(patch, res)
    ref = ref_encode_image(patch, res) if rh.available() else np.load(PINS)[pin_name(patch, res)]
    with torch.no_grad():
        ora = clip_ref.encode_image({k: torch.as_tensor(v) for k, v in sd.items()}, img).numpy()
    assert ora.shape == ref.shape == (3, 64)
    np.testing.assert_allclose(ora, ref, rtol=1e-4, atol=1e-5)
