"""Host-only checks of the latent spaces and the truncation trick: the per-layer psi rule of the library, dlatent_avg ingestion, the
synthetic weights left as they were, config / flag plumbing and its refusals, and the operators."""
import hashlib
import os
import types

import numpy as np
import pytest

from clip_glass_amd import config as gconfig
from clip_glass_amd import engine, generator, operators, run, synth
from clip_glass_amd.latent import StyleGAN2LatentSpace, stylegan2_n_lat
from clip_glass_amd.models import StyleGAN2

HERE = os.path.dirname(os.path.abspath(__file__))
needs_lib = pytest.mark.skipif(not os.path.exists(engine.LIB_PATH), reason="libglass.so is not built here")
MINI_CHANNELS = [16, 16, 32, 32]


# ---- glass_host_layer_psi ----------------------------------------------------------------------------------
@needs_lib
@pytest.mark.parametrize("n_lat,psi,cutoff,want", [
    (8, 0.5, 3, [.5, .5, .5, 1, 1, 1, 1, 1]),
    (8, 0.7, None, [.7] * 8),            # cutoff None -> -1: every layer
    (8, 0.7, -1, [.7] * 8),
    (8, 0.7, 8, [.7] * 8),               # cutoff = n_lat
    (8, 0.7, 0, [1.] * 8),               # cutoff 0: off (models.py:276)
    (8, 1.0, 5, [1.] * 8),               # psi 1: off
    (18, 0.0, 1, [0.] + [1.] * 17),
])
def test_layer_psi_table(n_lat, psi, cutoff, want):
    np.testing.assert_array_equal(engine.host_layer_psi(n_lat, psi, cutoff), np.array(want, np.float32))


@needs_lib
@pytest.mark.parametrize("psi,cutoff,msg", [(-0.1, None, "psi < 0"), (1.01, None, "psi > 1"), (float("nan"), None, "finite"),
                                            (float("inf"), None, "finite"), (0.5, 9, "cutoff"), (0.5, -2, "cutoff")])
def test_layer_psi_refusals(psi, cutoff, msg):
    with pytest.raises(RuntimeError, match=msg):
        engine.host_layer_psi(8, psi, cutoff)


# ---- weights -------------------------------------------------------------------------------------------------
def test_dlatent_avg_read_from_the_container_and_kept_out_of_state():
    import torch
    w = os.path.join(HERE, "golden", "containers", "mini")
    m = StyleGAN2(types.SimpleNamespace(weights=w, dim_z=32))
    g = torch.load(os.path.join(w, "G.pth"), map_location="cpu", weights_only=False)
    want = g["state_dict"]["dlatent_avg"].float().numpy()
    assert m.dlatent_avg.dtype == np.float32 and m.dlatent_avg.shape == (32,)
    np.testing.assert_array_equal(m.dlatent_avg, want)
    assert not [k for k in m.state if k.endswith("dlatent_avg")]


def test_synthetic_weights_have_a_dlatent_avg_of_their_own():
    m = StyleGAN2(types.SimpleNamespace(weights="synthetic:5", dim_z=32, channels=MINI_CHANNELS, mapping_layers=2))
    np.testing.assert_array_equal(m.dlatent_avg, synth.dlatent_avg(32, 5))
    assert m.dlatent_avg.shape == (32,) and m.dlatent_avg.dtype == np.float32 and np.abs(m.dlatent_avg).min() > 0
    assert not np.array_equal(synth.dlatent_avg(32, 5), synth.dlatent_avg(32, 6))
    assert "dlatent_avg" not in m.state


def _state_hash(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(str(v.shape).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


MINI_STATE_SHA256 = "49f81b24143aff58e3f75ef3bc63462b642c60d6d42330c28a3f3f6c5c63150d"      # computed on the commit before synth.dlatent_avg existed


def test_make_state_is_what_it_was():
    sd = synth.make_state(synth.stylegan2_g_spec(MINI_CHANNELS, 32, 2), 0)
    sd.update(synth.make_state(synth.stylegan2_d_spec(MINI_CHANNELS), 0))
    assert "dlatent_avg" not in sd
    assert _state_hash(sd) == MINI_STATE_SHA256


# ---- config / flags ------------------------------------------------------------------------------------------
def _cfg(name, **kw):
    c = types.SimpleNamespace(config=name)
    vars(c).update(gconfig.get_config(name))
    vars(c).update(kw)
    return c


def test_latent_options_defaults_and_values():
    assert generator.latent_options(_cfg("StyleGAN2_ffhq_d")) == ("z", 1.0, None)
    assert generator.latent_options(_cfg("StyleGAN2_ffhq_d", latent_space=None, truncation_psi=None)) == ("z", 1.0, None)
    assert generator.latent_options(_cfg("StyleGAN2_car_nod", latent_space="w+", truncation_psi=0.7, truncation_cutoff=8)) == ("w+", 0.7, 8)
    assert generator.latent_options(_cfg("DeepMindBigGAN256")) == ("z", 1.0, None)
    with pytest.raises(ValueError, match="unknown latent_space"):
        generator.latent_options(_cfg("StyleGAN2_ffhq_d", latent_space="s"))


@pytest.mark.parametrize("name", ["DeepMindBigGAN256", "DeepMindBigGAN512", "GPT2"])
@pytest.mark.parametrize("kw", [dict(latent_space="w"), dict(truncation_psi=0.7), dict(truncation_cutoff=4)])
def test_latent_options_refused_for_other_generators(name, kw):
    with pytest.raises(ValueError, match="StyleGAN2 configs"):
        generator.latent_options(_cfg(name, **kw))


def test_run_flags_reach_the_config_and_are_refused_for_biggan(tmp_path):
    a = run.build_parser().parse_args(["--latent-space", "w+", "--truncation-psi", "0.7", "--truncation-cutoff", "8"])
    assert (a.latent_space, a.truncation_psi, a.truncation_cutoff) == ("w+", 0.7, 8)
    d = run.build_parser().parse_args([])
    assert (d.latent_space, d.truncation_psi, d.truncation_cutoff) == (None, None, None)
    with pytest.raises(SystemExit):
        run.build_parser().parse_args(["--latent-space", "s"])
    for cfg in ("DeepMindBigGAN256", "GPT2"):      # refused before any weight is looked for
        with pytest.raises(ValueError, match="StyleGAN2 configs"):
            run.main(["--config", cfg, "--latent-space", "w", "--tmp-folder", str(tmp_path)])
        with pytest.raises(ValueError, match="StyleGAN2 configs"):
            run.main(["--config", cfg, "--truncation-psi", "0.5", "--tmp-folder", str(tmp_path)])


def test_latent_space_rows_and_saved_keys():
    for space, key, width in (("z", "z", 32), ("w", "w", 32), ("w+", "w_plus", 8 * 32)):
        c = types.SimpleNamespace(batch_size=4, dim_z=32, channels=MINI_CHANNELS, latent_space=space)
        ls = StyleGAN2LatentSpace(c)
        assert ls.population().shape == (4, width) and ls.population().dtype == np.float32
        assert list(ls.state_dict()) == [key]
        ls.set_from_population(np.ones((3, width)))
        assert ls.state_dict()[key].shape == (3, width)
    assert list(StyleGAN2LatentSpace(types.SimpleNamespace(batch_size=4, dim_z=32)).state_dict()) == ["z"]       # no key: z, as before
    assert stylegan2_n_lat(types.SimpleNamespace()) == 18 and stylegan2_n_lat(types.SimpleNamespace(n_lat=14)) == 14


# ---- operators -----------------------------------------------------------------------------------------------
def test_operators_for_z_are_what_they_were():
    for c in (_cfg("StyleGAN2_ffhq_d"), _cfg("StyleGAN2_ffhq_d", latent_space="z"), _cfg("StyleGAN2_ffhq_d", latent_space=None)):
        ops = operators.get_operators(c)
        assert set(ops) == {"sampling", "crossover", "mutation"}
        assert type(ops["sampling"]) is operators.NormalRandomSampling and (ops["sampling"].mu, ops["sampling"].std) == (0, 1)
        if not operators.HAVE_PYMOO:
            assert ops["crossover"] == dict(kind="crossover", name="real_sbx", prob=1.0, eta=3.0)
            assert ops["mutation"] == dict(kind="mutation", name="real_pm", prob=0.5, eta=3.0)
    np.random.seed(4)
    a = operators.get_operators(_cfg("StyleGAN2_ffhq_d"))["sampling"]._do(types.SimpleNamespace(n_var=512), 3)
    np.random.seed(4)
    np.testing.assert_array_equal(a, np.random.normal(0, 1, size=(3, 512)))


class _StubGenerator:
    def __init__(self):
        self.seen = []

    def map_latents(self, z):
        self.seen.append(np.array(z))
        return (2 * np.asarray(z, np.float32) + 1).astype(np.float32)


@pytest.mark.parametrize("space,tile", [("w", 1), ("w+", 8)])
def test_mapped_normal_sampling(space, tile):
    c = _cfg("StyleGAN2_ffhq_d", latent_space=space, dim_z=32, channels=MINI_CHANNELS)
    ops = operators.get_operators(c)
    z_ops = operators.get_operators(_cfg("StyleGAN2_ffhq_d"))
    assert type(ops["sampling"]) is operators.MappedNormalSampling
    assert ops["crossover"] == z_ops["crossover"] or type(ops["crossover"]) is type(z_ops["crossover"])
    assert ops["mutation"] == z_ops["mutation"] or type(ops["mutation"]) is type(z_ops["mutation"])
    prob = types.SimpleNamespace(generator=_StubGenerator(), n_var=32 * tile)
    np.random.seed(7)
    X = ops["sampling"]._do(prob, 5)
    assert X.shape == (5, 32 * tile) and X.dtype == np.float64
    z = prob.generator.seen[0]
    assert z.shape == (5, 32) and z.dtype == np.float32
    np.random.seed(7)
    np.testing.assert_array_equal(z, np.random.normal(0, 1, size=(5, 32)).astype(np.float32))     # drawn as the z search draws
    for l in range(tile):                                                                       # layer-major: the dlatent, n_lat times
        np.testing.assert_array_equal(X[:, l * 32:(l + 1) * 32], 2 * z + 1)
    np.random.seed(7)
    np.testing.assert_array_equal(ops["sampling"].do(prob, 5) if not operators.HAVE_PYMOO else ops["sampling"]._do(prob, 5), X)   # deterministic under a seed


def test_engine_refuses_an_unknown_space_by_name():
    with pytest.raises(ValueError, match="unknown latent_space"):
        engine.latent_space_id("w++")
    assert [engine.latent_space_id(s) for s in ("z", "w", "w+")] == [0, 1, 2]
    assert engine.truncation_cutoff_arg(None) == -1 and engine.truncation_cutoff_arg(3) == 3
