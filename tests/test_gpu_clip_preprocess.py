"""The opt-in CLIP preprocessing on the device: preprocess_patches_kernel (antialiased bilinear / bicubic resize, CLIP mean / std) and the
normalising instance of the default resize, against torch's own ops in float64 — op by op, end to end through the C ABI, and the
invariants of the pass (chunking, batching, the untouched default)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clip_glass_amd import ops, synth
from clip_glass_amd.engine import Engine
from clip_glass_amd.generator import CLIP_PREPROCESS
from oracle import clip_ref
import glass_models as M
from util import check, diag

pytestmark = pytest.mark.gpu

MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073], dtype=torch.float64)[None, :, None, None]     # clip/clip.py:73
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711], dtype=torch.float64)[None, :, None, None]


def _t(sd):
    return {k: torch.as_tensor(v) for k, v in sd.items()}


def torch_preprocess(img01, S, resize, normalize):
    """The definition: img01 = biggan_norm(y) [B,3,R,R] in [0, 1] -> float64 [B,3,S,S]."""
    x = torch.as_tensor(img01).double()
    if resize == 0:
        v = F.interpolate(x, (S, S), mode="bilinear", align_corners=False)
    elif resize == 1:
        v = F.interpolate(x, (S, S), mode="bilinear", align_corners=False, antialias=True)
    else:
        v = F.interpolate(x, (S, S), mode="bicubic", align_corners=False, antialias=True).clamp(0, 1)
    return (v - MEAN) / STD if normalize else v


def as_patches(v, ps):
    B, _, S, _ = v.shape
    G = S // ps
    return v.view(B, 3, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, 3 * ps * ps).numpy()


# ---- op level ----------------------------------------------------------------------------------------------------------------
OP_CASES = [(1024, 224, 32), (1024, 224, 16), (1024, 224, 14), (1024, 336, 14), (512, 224, 32), (256, 224, 32), (128, 224, 32),
            (64, 32, 8), (32, 32, 8)]


@pytest.mark.parametrize("resize,normalize", [(1, 0), (2, 1), (0, 1)])
@pytest.mark.parametrize("R,S,ps", OP_CASES)
def test_preprocess_op(R, S, ps, resize, normalize):
    """Bar: the project's resize bar, 1e-3 * max|ref| (fp32 taps, fp32 accumulation, one fp16 rounding of the result)."""
    for B in (2, 3):
        y = synth.normal(23, "y%d" % B, (B, 3, R, R), 0.8)
        ref = as_patches(torch_preprocess(((torch.tensor(y).double() + 1) / 2).clip(0, 1), S, resize, normalize), ps)
        got = ops.preprocess(y, S, ps, resize, normalize)
        assert got.shape == ref.shape == (B * (S // ps) ** 2, 3 * ps * ps)
        check("preprocess %d->%d ps%d mode (%d,%d) B%d" % (R, S, ps, resize, normalize, B), got, ref, 1e-3)


@pytest.mark.parametrize("R,S,ps", [(1024, 224, 32), (256, 224, 14), (64, 32, 8)])
def test_default_through_the_new_op_is_the_old_kernel(R, S, ps):
    y = synth.normal(23, "y", (2, 3, R, R), 0.8)
    np.testing.assert_array_equal(ops.preprocess(y, S, ps, 0, 0), ops.resize(y, S, ps))


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _sg2_engine(name, sd, P, bs, chunk=0, preprocess=None, noise_mode=2, noise_seed=0, **kw):
    c = M.CONFIGS[name]
    if preprocess is not None:
        kw.update(clip_resize=CLIP_PREPROCESS[preprocess][0], clip_normalize=CLIP_PREPROCESS[preprocess][1])
    e = Engine(c["channels"][::-1], latent_size=c["latent"], mapping_layers=c["mapping"], batch_size=bs, use_discriminator=False, n_obj=1,
               max_pop=P, chunk=chunk, clip=c["clip"], noise_mode=noise_mode, noise_seed=noise_seed, **kw)
    e.load_state(sd)
    e.finalize()
    return e


def _bg_engine(sd, P, bs, chunk=0, preprocess=None):
    c = M.BIGGAN_CONFIGS["bg_mini"]
    kw = {}
    if preprocess is not None:
        kw.update(clip_resize=CLIP_PREPROCESS[preprocess][0], clip_normalize=CLIP_PREPROCESS[preprocess][1])
    e = Engine([], batch_size=bs, max_pop=P, chunk=chunk, clip=c["clip"],
               biggan=dict(layers=c["layers"], attention_pos=c["attention_pos"], ch=c["ch"], z_dim=c["z_dim"],
                           num_classes=c["num_classes"], truncation=1.0), **kw)
    e.load_state(sd)
    e.finalize()
    return e


def _against_oracle(tag, e, sd, x, clip, preprocess, **run):
    """The engine's own images -> the torch definition -> the oracle's image tower, against details()."""
    P = x.shape[0]
    img = e.generate(x, **run)
    pre = torch_preprocess(img, clip[4], *CLIP_PREPROCESS[preprocess]).float()
    with torch.no_grad():
        feats = clip_ref.encode_image(_t(sd), pre).numpy()
    target = M.make_target(feats)
    sim_o = torch.cosine_similarity(torch.tensor(feats), torch.tensor(target)[None]).numpy()
    e.set_target(target)
    Fe = e.evaluate(x, **run)
    det = e.details(P)
    check(tag + " clip features", det["features"], feats, 5e-3)
    rel = np.abs(det["sim"] - sim_o) / np.abs(sim_o)
    diag("[e2e] %s sim range [%.3f, %.3f] max rel err %.3e" % (tag, sim_o.min(), sim_o.max(), rel.max()))
    assert rel.max() < 1e-3, "CLIP similarity relative error %.3e > 1e-3" % rel.max()
    np.testing.assert_allclose(Fe[:, 0], -det["sim"], rtol=0, atol=1e-7)
    return target, Fe


@pytest.mark.parametrize("preprocess", ["clip", "antialias"])
def test_end_to_end_mid(preprocess):
    P, bs = 8, 4
    sd = M.make_state("mid", 0, with_d=False)
    x = synth.latents(3, P, M.CONFIGS["mid"]["latent"])
    planes = M.noise_planes("mid", 31, 0, P // bs)
    e = _sg2_engine("mid", sd, P, bs, preprocess=preprocess)
    _against_oracle("mid %s" % preprocess, e, sd, x, M.CONFIGS["mid"]["clip"], preprocess, noise=planes)
    e.close()


@pytest.mark.parametrize("preprocess", ["clip", "antialias"])
def test_end_to_end_biggan_mini(preprocess):
    P, bs = 8, 4
    c = M.BIGGAN_CONFIGS["bg_mini"]
    sd = M.make_biggan_state("bg_mini", 0)
    x = synth.biggan_population(1, P, c["z_dim"], c["num_classes"])
    e = _bg_engine(sd, P, bs, preprocess=preprocess)
    _against_oracle("bg_mini %s" % preprocess, e, sd, x, c["clip"], preprocess)
    e.close()


def test_end_to_end_ffhq_full_size():
    """1024 px -> ViT-B/32 at 224 px through CLIP's own transform: the 4.57 x bicubic down-scale, 19 taps per axis."""
    P, bs = 4, 4
    sd = M.make_state("ffhq", 0, with_d=False)
    x = synth.latents(3, P, M.CONFIGS["ffhq"]["latent"])
    e = _sg2_engine("ffhq", sd, P, bs, preprocess="clip", noise_mode=1, noise_seed=1234)
    _against_oracle("ffhq clip", e, sd, x, M.CONFIGS["ffhq"]["clip"], "clip")
    e.close()


# ---- invariants --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preprocess", ["clip", "antialias"])
def test_whole_population_equals_two_chunks_and_rows_are_independent(preprocess):
    P, bs = 8, 4
    sd = M.make_state("mid", 0, with_d=False)
    x = synth.latents(3, P, M.CONFIGS["mid"]["latent"])
    planes = M.noise_planes("mid", 31, 0, P // bs)
    target = M.make_target(synth.normal(25, "t", (P, M.CONFIGS["mid"]["clip"][5])))
    rows = []
    for chunk in (8, 4):
        e = _sg2_engine("mid", sd, P, bs, chunk=chunk, preprocess=preprocess)
        e.set_target(target)
        rows.append(e.evaluate(x, noise=planes))
        if chunk == 8:
            alone = e.evaluate(x[:4], noise=planes[:1])          # the first minibatch without the second
        e.close()
    np.testing.assert_array_equal(rows[0], rows[1])
    np.testing.assert_array_equal(alone, rows[0][:4])


def test_explicit_zeros_are_the_default_and_the_modes_are_not():
    P, bs = 8, 4
    sd = M.make_state("mid", 0, with_d=False)
    x = synth.latents(3, P, M.CONFIGS["mid"]["latent"])
    planes = M.noise_planes("mid", 31, 0, P // bs)
    target = M.make_target(synth.normal(25, "t", (P, M.CONFIGS["mid"]["clip"][5])))
    out = {}
    for name, kw in [("default", {}), ("zeros", dict(clip_resize=0, clip_normalize=0)), ("reference", dict(preprocess="reference")),
                     ("antialias", dict(preprocess="antialias")), ("clip", dict(preprocess="clip")),
                     ("normalize", dict(clip_resize=0, clip_normalize=1))]:
        e = _sg2_engine("mid", sd, P, bs, **kw)
        e.set_target(target)
        out[name] = e.evaluate(x, noise=planes)
        e.close()
    np.testing.assert_array_equal(out["zeros"], out["default"])
    np.testing.assert_array_equal(out["reference"], out["default"])
    for name in ("antialias", "clip", "normalize"):            # a silently ignored flag would give the default's rows
        diag("[preprocess] mid %s vs default: max |dF| %.3e" % (name, np.abs(out[name] - out["default"]).max()))
        assert not np.array_equal(out[name], out["default"]), name
    assert not np.array_equal(out["clip"], out["antialias"])
