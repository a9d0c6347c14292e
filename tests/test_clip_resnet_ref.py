"""CLIP's ResNet image towers without a GPU: the float64 restatement (tests/clip_resnet_ref.py) pinned to the reference's own
ModifiedResNet, the conditions the tower tests' inputs must meet, the library's geometry rule, the named table, the selection of a
tower for synthetic weights and from a checkpoint, and the command-line flag.

The restatement is pinned live where the reference is present (clip/model.py build_model -> .visual, float32), else against
tests/golden/clip_resnet_pins.npz (tests/golden/make_clip_resnet_pins.py), at the project's oracle pin tolerance.
"""
import itertools
import os
import types

import numpy as np
import pytest
import torch

import clip_resnet_ref as R
import ref_harness as rh
from clip_glass_amd import engine, generator, synth

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_resnet_pins.npz")
RN50 = ((3, 4, 6, 3), 64, 224, 1024)
RN101 = ((3, 4, 23, 3), 64, 224, 512)


# ---- the restatement against the reference -------------------------------------------------------------------------------------------
def ref_visual_features(case):
    """The reference's ModifiedResNet, built by its own build_model from the synthetic state of a tower case, on the case's images."""
    layers, width, res, embed, _ = R.TOWER_CASES[case]
    sd = dict(R.tower_state(case))
    sd.update(synth.make_state(synth.clip_text_spec(width=64, layers=1, ctx=8, vocab=64, out_dim=embed), 8))   # build_model wants both towers
    st = {k[len("clip."):]: torch.as_tensor(v) for k, v in sd.items()}
    st["input_resolution"] = torch.tensor(res)
    st["context_length"] = torch.tensor(8)
    st["vocab_size"] = torch.tensor(64)
    model = rh.load_reference()["clip_model"].build_model(st).float()
    vis = model.visual
    assert type(vis).__name__ == "ModifiedResNet" and vis.input_resolution == res
    assert tuple(len(getattr(vis, "layer%d" % b)) for b in (1, 2, 3, 4)) == tuple(layers)
    with torch.no_grad():
        return vis(torch.tensor(R.tower_images(case))).numpy()


@pytest.mark.parametrize("case", R.PIN_CASES)
def test_restatement_matches_reference(case):
    ref = ref_visual_features(case) if rh.available() else np.load(PINS)[case]
    got = R.tower_reference(case)
    assert got.shape == ref.shape == (R.TOWER_CASES[case][4], R.TOWER_CASES[case][3])
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("case", sorted(R.TOWER_CASES))
def test_tower_inputs_are_fit_for_the_feature_bar(case):
    """What a GPU comparison at 5e-3 * max|ref| needs of its inputs: fp16 storage of the activations alone stays within 1e-3 * max, and
    every two rows differ by at least 10 x the bar (swapped or repeated rows cannot pass)."""
    ref, stored = R.tower_reference(case), R.tower_reference(case, True)
    scale = np.abs(ref).max()
    assert np.isfinite(ref).all() and scale > 0
    assert np.abs(stored - ref).max() <= 1e-3 * scale, np.abs(stored - ref).max() / scale
    for i, j in itertools.combinations(range(ref.shape[0]), 2):
        assert np.abs(ref[i] - ref[j]).max() >= 10 * R.FEATURE_BAR * scale, (i, j, np.abs(ref[i] - ref[j]).max() / scale)


def test_single_op_references():
    """The op references against torch's own modules on a small map."""
    x = synth.normal(1, "x", (2, 6, 6, 8))
    xt = torch.tensor(x).permute(0, 3, 1, 2).double()
    np.testing.assert_allclose(R.avgpool2(x), torch.nn.AvgPool2d(2)(xt).permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    bn = torch.nn.BatchNorm2d(8).double().eval()
    sd = {"p.weight": synth.normal(2, "g", (8,), 0.1, 0.7), "p.bias": synth.normal(2, "b", (8,), 0.1),
          "p.running_mean": synth.normal(2, "m", (8,), 0.2), "p.running_var": 0.4 + np.abs(synth.normal(2, "v", (8,)))}
    bn.load_state_dict({k[2:]: torch.tensor(v).double() for k, v in sd.items()}, strict=False)
    a, s = R.bn_affine(sd, "p")
    w = synth.normal(3, "w", (8, 8, 3, 3), 0.2)
    res = synth.normal(3, "r", (2, 6, 6, 8))
    with torch.no_grad():
        want = torch.relu(bn(torch.nn.functional.conv2d(xt, torch.tensor(w).double(), padding=1)) + torch.tensor(res).permute(0, 3, 1, 2).double())
    np.testing.assert_allclose(R.conv_bn(x, w, a, s, res=res), want.permute(0, 2, 3, 1).numpy(), rtol=1e-10, atol=1e-12)
    pos = synth.normal(4, "pos", (37, 8))
    tok = R.attnpool_tokens(x.reshape(2, 36, 8), pos)
    np.testing.assert_allclose(tok[:, 0], x.reshape(2, 36, 8).astype(np.float64).mean(1) + pos[0], rtol=1e-12)
    np.testing.assert_allclose(tok[:, 1:], x.reshape(2, 36, 8) + pos[1:].astype(np.float64), rtol=1e-12)


# ---- the library's rule --------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported():
    assert hasattr(engine.load_library(), "glass_clip_resnet_supported")


@pytest.mark.parametrize("geom", [RN50, RN101] + [R.TOWER_CASES[c][:4] for c in sorted(R.TOWER_CASES)])
def test_supported_geometries(geom):
    ok, msg = engine.clip_resnet_supported(geom)
    assert ok and msg == "", (geom, msg)


@pytest.mark.parametrize("geom,word", [
    (((4, 6, 10, 6), 80, 288, 640), "multiple of 64"),       # RN50x4
    (((6, 8, 18, 8), 96, 384, 768), "multiple of 64"),       # RN50x16
    (((3, 4, 6, 3), 64, 225, 1024), "multiple of 32"),
    (((3, 4, 0, 3), 64, 224, 1024), "bottlenecks"),
])
def test_unsupported_geometries_say_why(geom, word):
    ok, msg = engine.clip_resnet_supported(geom)
    assert not ok and word in msg, msg
    with pytest.raises(ValueError, match=word):
        generator.check_clip_geometry(geom)


def test_config_mirror_appends_the_resnet_fields():
    import ctypes
    G = engine.GlassConfig
    names = [f[0] for f in G._fields_]
    assert names[29:33] == ["clip_resize", "clip_normalize", "clip_arch", "clip_rn_layers"]
    assert (G.clip_resize.offset, G.clip_normalize.offset) == (356, 360)         # appended: nothing before them moved
    assert G.clip_arch.offset == 364 == G.clip_normalize.offset + 4 and G.clip_rn_layers.offset == 368 == G.clip_arch.offset + 4
    assert G.clip_rn_layers.size == 16 and G.lpips_size.offset == 384            # the struct with them: 364 + 4 + 16 = 384, 8-byte aligned
    assert ctypes.alignment(G) == 8 and ctypes.sizeof(G) == 408
    cfg = G()
    assert cfg.clip_arch == 0 and list(cfg.clip_rn_layers) == [0, 0, 0, 0]       # zero: the ViT engine


# ---- the named table and the selection -----------------------------------------------------------------------------------------------
def test_named_table():
    assert generator.CLIP_RESNET_MODELS == {"RN50": RN50, "RN101": RN101}
    assert generator.CLIP_RESNET_TEXT_MODELS == {"RN50": dict(width=512, layers=12), "RN101": dict(width=512, layers=12)}
    assert not set(generator.CLIP_RESNET_MODELS) & set(generator.CLIP_MODELS)
    assert generator.clip_resnet_geometry("RN101") == RN101 and generator.clip_resnet_name(RN50) == "RN50"
    assert generator.clip_resnet_name(((1, 1, 1, 1), 64, 64, 64)) is None
    assert generator.resnet_engine_fields(RN50) == (64, 16, 32, 32, 224, 1024)
    with pytest.raises(ValueError, match="RN101"):
        generator.clip_resnet_geometry("RN50x4")


def _cfg(**kw):
    return types.SimpleNamespace(clip_weights="synthetic:3", **kw)


MINI = ((1, 1, 1, 1), 64, 64, 64)


def test_synthetic_selection(monkeypatch):
    real = synth.make_state

    def first_blocks(spec, seed):        # keep every shape, not the depth: RN101 is 56 M values
        return real([s for s in spec if ".layer" not in s[0] or s[0].split(".")[3] == "0"], seed)
    monkeypatch.setattr(synth, "make_state", first_blocks)
    for name, want in (("RN50", RN50), ("RN101", RN101)):
        state, geom = generator._load_clip_state(_cfg(clip_resnet=name), True)
        assert geom == want and generator.is_resnet_geometry(geom)
        assert state["clip.visual.conv1.weight"].shape == (32, 3, 3, 3)
        assert state["clip.visual.layer4.0.downsample.0.weight"].shape == (2048, 1024, 1, 1)
        assert state["clip.visual.attnpool.positional_embedding"].shape == (50, 2048)
        assert state["clip.visual.attnpool.c_proj.weight"].shape == (want[3], 2048)
        assert "clip.visual.proj" not in state
        assert state["clip.token_embedding.weight"].shape[1] == 512 and state["clip.text_projection"].shape == (512, want[3])
    monkeypatch.undo()
    state, geom = generator._load_clip_state(_cfg(clip_resnet="RN101", clip_resnet_geometry=MINI), False)      # the explicit tuple wins
    assert geom == MINI and state["clip.visual.attnpool.positional_embedding"].shape == (5, 2048)
    assert generator.clip_resnet_geometry_from_state(state) == MINI
    with pytest.raises(ValueError, match="unknown CLIP ResNet model"):
        generator._load_clip_state(_cfg(clip_resnet="RN50x4"), False)
    for both in (dict(clip_model="ViT-B/16", clip_resnet="RN50"), dict(clip_geometry=(64, 2, 1, 8, 32, 32), clip_resnet_geometry=MINI)):
        with pytest.raises(ValueError, match="both"):
            generator._load_clip_state(_cfg(**both), False)


def test_synthetic_statistics_are_not_trivial():
    sd = synth.make_state(synth.clip_resnet_spec(*MINI), 0)
    for p in ("clip.visual.bn1", "clip.visual.layer2.0.bn3", "clip.visual.layer3.0.downsample.1"):
        assert (sd[p + ".running_var"] > 0).all() and np.abs(sd[p + ".running_var"] - 1).mean() > 0.1
        assert np.abs(sd[p + ".running_mean"]).mean() > 0.05 and np.abs(sd[p + ".weight"] - 1).mean() > 0.02
        assert sd[p + ".num_batches_tracked"].shape == ()
    a, s = R.bn_affine(sd, "clip.visual.layer2.0.bn3")
    assert np.abs(a - 1).min() > 0.3 and np.abs(s).mean() > 0.01         # far from the identity: a dropped scale or shift cannot pass


def _write_checkpoint(path, geom):
    """Every key of a 1-block-per-stage tower with the named model's widths; the remaining blocks' keys as stubs (the depth is read from
    the key names, clip/model.py:373)."""
    layers, width, res, embed = geom
    sd = synth.make_state(synth.clip_resnet_spec((1, 1, 1, 1), width, res, embed), 0)
    out = {k[len("clip."):]: torch.as_tensor(v) for k, v in sd.items()}
    for st, n in enumerate(layers):
        for i in range(1, n):
            out["visual.layer%d.%d.conv1.weight" % (st + 1, i)] = torch.zeros(1)
    torch.save(out, path)


def test_checkpoint_decides_and_mismatch_names_both(tmp_path):
    path = str(tmp_path / "rn101.pt")
    _write_checkpoint(path, RN101)
    cfg = types.SimpleNamespace(clip_weights=path)
    state, geom = generator._load_clip_state(cfg, False)
    assert geom == RN101 and generator.clip_state_is_resnet(state)          # no clip.visual.proj: a ResNet, no name given
    cfg.clip_resnet = "RN101"
    assert generator._load_clip_state(cfg, False)[1] == RN101
    cfg.clip_resnet = "RN50"
    with pytest.raises(ValueError) as ei:
        generator._load_clip_state(cfg, False)
    assert "RN50" in str(ei.value) and "RN101" in str(ei.value)
    cfg = types.SimpleNamespace(clip_weights=path, clip_model="ViT-B/32")
    with pytest.raises(ValueError) as ei:
        generator._load_clip_state(cfg, False)
    assert "ViT-B/32" in str(ei.value) and "RN101" in str(ei.value)


def test_vit_checkpoint_refuses_a_resnet_name(tmp_path):
    sd = synth.make_state(synth.clip_visual_spec(64, 1, 8, 32, 32), 0)
    path = str(tmp_path / "vit.pt")
    torch.save({k[len("clip."):]: torch.as_tensor(v) for k, v in sd.items()}, path)
    with pytest.raises(ValueError) as ei:
        generator._load_clip_state(types.SimpleNamespace(clip_weights=path, clip_resnet="RN50"), False)
    assert "RN50" in str(ei.value) and "ViT" in str(ei.value)


def test_cli_flag():
    from clip_glass_amd import run
    p = run.build_parser()
    assert p.parse_args(["--clip-resnet", "RN101"]).clip_resnet == "RN101"
    assert p.parse_args([]).clip_resnet is None
    with pytest.raises(SystemExit):
        p.parse_args(["--clip-resnet", "ViT-B/32"])
