"""Crop views, everything that needs no GPU: the boxes (library == numpy mirror == known answers), the definition against an fp32
emulation of the kernel's arithmetic, the host rule and its reasons, the untouched config structs, and the Python plumbing."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import clip_views_ref as VR
from clip_glass_amd import config as gconfig
from clip_glass_amd import engine, generator, synth

KNOWN = {      # seed 7, generation 3, V = 4, 500 per mille, flips on
    32: [(0, 0, 32, 0), (0, 0, 32, 1), (1, 0, 24, 1), (1, 1, 28, 0)],
    64: [(0, 0, 64, 0), (3, 0, 48, 1), (7, 16, 48, 1), (7, 6, 46, 0)],
}


# ---- boxes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [32, 64])
def test_known_answers(R):
    lib = engine.host_clip_view_boxes(7, 3, 4, R, 500, 1, 0)
    mirror = synth.clip_view_boxes(7, 3, 4, R, 500, 1, 0)
    assert lib.dtype == np.int32 and lib.shape == (4, 4)
    assert lib.tolist() == [list(b) for b in KNOWN[R]]
    assert mirror.tolist() == [list(b) for b in KNOWN[R]]


def test_tag():
    assert synth.CLIP_VIEW_TAG == 0x56494557 and synth.CLIP_VIEW_TAG != synth.GPT2_SAMPLE_TAG


@pytest.mark.parametrize("R,permille,seed", [(32, 500, 7), (1024, 250, (5 << 32) | 9), (64, 1, 0), (64, 1000, 3)])
def test_boxes_over_200_generations(R, permille, seed):
    smin = max(2, (R * permille + 999) // 1000)
    flips, sets = set(), set()
    for g in range(200):
        b = engine.host_clip_view_boxes(seed, g, 5, R, permille, 1, 0)
        np.testing.assert_array_equal(b, synth.clip_view_boxes(seed, g, 5, R, permille, 1, 0))
        assert b[0].tolist() == [0, 0, R, 0]
        assert (b[:, 2] >= smin).all() and (b[:, 2] <= R).all()
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all()
        assert (b[:, 0] + b[:, 2] <= R).all() and (b[:, 1] + b[:, 2] <= R).all()
        flips.update(b[1:, 3].tolist())
        sets.add(b.tobytes())
    assert flips == {0, 1}
    if permille == 1000:            # every crop is the whole image: only the four flips vary
        assert smin == R and 1 < len(sets) <= 16
    else:
        assert len(sets) > 100      # different generations differ


def test_fixed_no_flip_and_generations():
    fixed = [engine.host_clip_view_boxes(7, g, 4, 64, 500, 1, 1) for g in (0, 1, 17)]
    for b in fixed[1:]:
        np.testing.assert_array_equal(b, fixed[0])
    np.testing.assert_array_equal(fixed[0], engine.host_clip_view_boxes(7, 0, 4, 64, 500, 1, 0))      # generation word 0
    np.testing.assert_array_equal(fixed[0], synth.clip_view_boxes(7, 5, 4, 64, 500, 1, 1))
    for g in range(50):
        noflip = engine.host_clip_view_boxes(7, g, 6, 64, 500, 0, 0)
        assert (noflip[:, 3] == 0).all()
        np.testing.assert_array_equal(noflip, synth.clip_view_boxes(7, g, 6, 64, 500, 0, 0))
        np.testing.assert_array_equal(noflip[:, :3], engine.host_clip_view_boxes(7, g, 6, 64, 500, 1, 0)[:, :3])
    assert not np.array_equal(engine.host_clip_view_boxes(7, 3, 4, 64, 500, 1, 0), engine.host_clip_view_boxes(7, 4, 4, 64, 500, 1, 0))
    assert not np.array_equal(engine.host_clip_view_boxes(7, 3, 4, 64, 500, 1, 0), engine.host_clip_view_boxes(8, 3, 4, 64, 500, 1, 0))


def test_box_function_refuses_bad_arguments():
    for args in [(7, 0, 0, 64, 500, 1, 0), (7, 0, 17, 64, 500, 1, 0), (7, 0, 4, 1, 500, 1, 0), (7, 0, 4, 64, 0, 1, 0), (7, 0, 4, 64, 1001, 1, 0)]:
        with pytest.raises(RuntimeError):
            engine.host_clip_view_boxes(*args)


# ---- the definition against the kernel's arithmetic ------------------------------------------------------------------------------
def _boxes(R):
    """every edge, s = 2, s = R, a flip; plus an interior box"""
    q = max(2, R // 3)
    return np.concatenate([VR.edge_boxes(R), np.array([(1, R - q - 1, q, 0), (R - q - 1, 1, q, 1)], np.int32)])


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("R,S", [(32, 32), (64, 32), (32, 64), (48, 20)])
def test_emulation_agrees_with_the_definition(R, S, normalize):
    """(32, 32): s < S for every crop; (64, 32): s > S and s < S; (32, 64): up-sampling throughout; (48, 20): an odd ratio.
    Bar 1e-5 * max|ref|: the kernel's source coordinate (s / S) (X + 0.5) - 0.5 is an fp32 number up to s, so it is off by about one ulp(s)
    (three roundings: the ratio, the product, the difference), and a white-noise image turns that into as large a pixel error; ulp(64) =
    7.6e-6 keeps crops up to 64 px under the bar.  The arithmetic is resize_patches_kernel's and has to stay so (the whole-image view is
    bit-equal to the default pass): on a 256 px noise image it measures 5.2e-5 over these boxes (the whole image among them), which is why the sizes here
    stop at 64 and the large sizes are held to the project's resize bar (1e-3) on the device (test_gpu_clip_views.py)."""
    y = synth.normal(23, "y", (2, 3, R, R), 0.8)
    boxes = _boxes(R)
    assert (boxes[:, 2] < S).any() or R > S
    img01 = ((torch.tensor(y).double() + 1) / 2).clip(0, 1)
    ref = VR.torch_views(img01, S, boxes, normalize).numpy()
    got = VR.emulate_views(y, S, boxes, normalize)
    assert got.dtype == np.float32 and got.shape == ref.shape == (2, len(boxes), 3, S, S)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err < 1e-5, err


@pytest.mark.parametrize("R,S", [(32, 32), (64, 32), (32, 64), (1024, 224), (256, 224)])
def test_whole_image_box_is_the_default_resize_exactly(R, S):
    y = synth.normal(23, "y", (1, 3, R, R), 0.8)
    np.testing.assert_array_equal(VR.emulate_views(y, S, [(0, 0, R, 0)])[:, 0], VR.emulate_resize(y, S))


def test_flip_reverses_the_columns():
    y = synth.normal(23, "y", (1, 3, 32, 32), 0.8)
    a = VR.emulate_views(y, 16, [(3, 5, 20, 0), (3, 5, 20, 1)])
    np.testing.assert_array_equal(a[:, 1], a[:, 0][..., ::-1])


def test_patch_rows_order():
    v = torch.arange(2 * 3 * 3 * 4 * 4, dtype=torch.float64).reshape(2, 3, 3, 4, 4)
    rows = VR.as_patch_rows(v, 2)
    assert rows.shape == (2 * 3 * 4, 12)
    b, vw, gy, gx = 1, 2, 1, 0
    np.testing.assert_array_equal(rows[(b * 3 + vw) * 4 + gy * 2 + gx].reshape(3, 2, 2), v[b, vw, :, 2:4, 0:2].numpy())


def test_mean_is_a_fixed_order_fp32_sum():
    vs = synth.normal(3, "s", (5, 4), 0.5).astype(np.float32)
    want = ((((np.float32(0) + vs[:, 0]) + vs[:, 1]) + vs[:, 2]) + vs[:, 3]) / np.float32(4)
    np.testing.assert_array_equal(VR.mean_sims(vs), want.astype(np.float32))
    np.testing.assert_array_equal(VR.mean_sims(vs[:, :1]), vs[:, 0])


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    lib = engine.load_library()
    for name in ("glass_engine_set_clip_views", "glass_clip_views_supported", "glass_host_clip_view_boxes", "glass_engine_last_view_details",
                 "glass_op_view_patches"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("args,words", [
    ((64, 50, 768, 0, 17, 500), ["views", "17"]),
    ((64, 50, 768, 0, -1, 500), ["views"]),
    ((64, 50, 768, 0, 8, 0), ["per mille"]),
    ((64, 50, 768, 0, 8, 1001), ["per mille"]),
    ((64, 50, 768, 1, 8, 500), ["clip_resize", "follow-up"]),
    ((64, 50, 768, 2, 8, 500), ["clip_resize", "tap table"]),
    ((4096, 577, 1024, 0, 16, 500), ["2^31"]),
    ((874, 50, 768, 0, 16, 500), ["2^31"]),          # 874 * 16 * 50 * 3072 = 2^31 + 458752: just above
])
def test_rule_refuses_with_its_reason(args, words):
    ok, msg = engine.clip_views_supported(*args)
    assert not ok
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("args", [(64, 50, 768, 0, 8, 500), (64, 50, 768, 0, 0, 500), (64, 50, 768, 0, 16, 1), (64, 50, 768, 0, 1, 1000),
                                  (873, 50, 768, 0, 16, 500),          # 873 * 16 * 50 * 3072 = 2^31 - 1998848: just below
                                  (64, 50, 768, 2, 0, 500)])           # views off: the preprocessing mode is not this rule's business
def test_rule_accepts(args):
    assert engine.clip_views_supported(*args) == (True, "")


def test_tower_rows():
    assert engine.clip_views_tower_rows(clip=(768, 12, 12, 32, 224, 512)) == (50, 768)
    assert engine.clip_views_tower_rows(clip=(1024, 24, 16, 14, 336, 768)) == (577, 1024)
    assert engine.clip_views_tower_rows(clip_resnet=((3, 4, 6, 3), 64, 224, 1024)) == (56 * 56, 64)
    assert engine.clip_view_permille(0.5) == 500 and engine.clip_view_permille(0.3333) == 333 and engine.clip_view_permille(1) == 1000


def test_config_structs_are_unchanged():
    G = engine.GlassConfig
    every = [f[0] for f in G._fields_]
    names = every[:31]                                              # the struct before the ResNet towers: 364 bytes, 368 at its 8-byte alignment
    assert names[-2:] == ["clip_resize", "clip_normalize"] and (G.clip_resize.offset, G.clip_normalize.offset) == (356, 360)
    assert C.alignment(G) == 8 and G.clip_normalize.size == 4
    assert every[31:33] == ["clip_arch", "clip_rn_layers"] and (G.clip_arch.offset, G.clip_rn_layers.offset) == (364, 368)
    assert G.clip_rn_layers.size == 16 and G.lpips_size.offset == 384        # with them: 384 bytes, and the next field starts there
    assert C.sizeof(G) == 408
    assert not any("view" in n for n in every)


# ---- the plumbing ------------------------------------------------------------------------------------------------------------
def test_cli_flags():
    from clip_glass_amd import run
    p = run.build_parser()
    a = p.parse_args([])
    assert (a.clip_views, a.clip_view_min, a.clip_view_flip, a.clip_view_fixed) == (None, None, None, None)
    a = p.parse_args(["--clip-views", "4", "--clip-view-min", "0.25", "--no-clip-view-flip", "--clip-view-fixed"])
    assert (a.clip_views, a.clip_view_min, a.clip_view_flip, a.clip_view_fixed) == (4, 0.25, False, True)


def test_run_copies_the_flags_into_the_config(monkeypatch):
    from clip_glass_amd import run

    class Stop(Exception):
        pass
    seen = {}
    keys = ("clip_views", "clip_view_min", "clip_view_flip", "clip_view_fixed")

    def problem(config, dist=None):
        seen.update({k: getattr(config, k, None) for k in keys})
        raise Stop()
    monkeypatch.setattr(run, "GenerationProblem", problem)
    with pytest.raises(Stop):
        run.main(["--config", "StyleGAN2_ffhq_nod", "--clip-views", "4", "--clip-view-min", "0.25", "--no-clip-view-flip", "--clip-view-fixed"])
    assert seen == dict(clip_views=4, clip_view_min=0.25, clip_view_flip=False, clip_view_fixed=True)
    with pytest.raises(Stop):
        run.main(["--config", "StyleGAN2_ffhq_nod"])
    assert seen == dict.fromkeys(keys)


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
                     target_features=np.ones(32, np.float32), channels=[16, 16, 32, 32], dim_z=32, mapping_layers=2)
    vars(cfg).update(kw)
    return cfg


def test_generator_hands_the_views_to_the_engine(monkeypatch):
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    g = generator.Generator(_txt2img_config("StyleGAN2_ffhq_d", clip_views=4, clip_view_min=0.25, clip_view_flip=False))
    kw = FakeEngine.made[0].kw
    assert (kw["clip_views"], kw["clip_view_min"], kw["clip_view_flip"], kw["clip_view_fixed"]) == (4, 0.25, False, False)
    assert g.augmentation == dict(kind="crop_views", clip_views=4, clip_view_min=0.25, clip_view_flip=False, clip_view_fixed=False)


def test_unset_flags_take_the_defaults(monkeypatch):
    """run.py's parser leaves an unset flag as None in the config."""
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    generator.Generator(_txt2img_config("StyleGAN2_ffhq_d", clip_views=2, clip_view_min=None, clip_view_flip=None, clip_view_fixed=None))
    kw = FakeEngine.made[0].kw
    assert (kw["clip_views"], kw["clip_view_min"], kw["clip_view_flip"], kw["clip_view_fixed"]) == (2, 0.5, True, False)


def test_generator_default_is_the_reference(monkeypatch):
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    g = generator.Generator(_txt2img_config("StyleGAN2_ffhq_d"))
    assert g.augmentation is None and g.clip_views == 0
    assert not any(k.startswith("clip_view") for k in FakeEngine.made[0].kw)


def test_img2txt_refuses_the_setting(monkeypatch):
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    cfg = types.SimpleNamespace(task="img2txt", model=lambda c: types.SimpleNamespace(state={}), pop_size=4, batch_size=4,
                                clip_weights="synthetic:0", clip_geometry=(64, 2, 1, 8, 32, 32), clip_views=4)
    with pytest.raises(ValueError, match="img2txt"):
        generator.Generator(cfg)
    assert not FakeEngine.made


def test_views_with_the_antialiased_preprocessing_are_refused_with_the_library_message(monkeypatch):
    monkeypatch.setattr(generator, "Engine", FakeEngine)
    FakeEngine.made = []
    _, reason = engine.clip_views_supported(8, 17, 64, 2, 4, 500)
    with pytest.raises(ValueError) as ei:
        generator.Generator(_txt2img_config("StyleGAN2_ffhq_d", clip_views=4, clip_preprocess="clip"))
    assert reason and reason in str(ei.value) and "follow-up" in str(ei.value)
    assert not FakeEngine.made
    with pytest.raises(ValueError, match="views must be in"):
        generator.Generator(_txt2img_config("StyleGAN2_ffhq_d", clip_views=17))
    assert not FakeEngine.made
