"""Host-only checks of latent space "sub": the layer-group spec, the library's one rule (glass_subspace_supported, through ctypes — no GPU),
the config / flag plumbing and its refusals, the npz round trip and the row width.  Needs the built library, not a GPU."""
import types

import numpy as np
import pytest

from clip_glass_amd import config as gconfig
from clip_glass_amd import engine, generator, operators, run, subspace
from clip_glass_amd.latent import StyleGAN2LatentSpace

MINI_CHANNELS = [16, 16, 32, 32]


# ---- parse_layer_groups -------------------------------------------------------------------------------------------
def test_parse_layer_groups():
    np.testing.assert_array_equal(subspace.parse_layer_groups(None, 18), np.zeros(18, np.int32))
    np.testing.assert_array_equal(subspace.parse_layer_groups("", 8), np.zeros(8, np.int32))
    np.testing.assert_array_equal(subspace.parse_layer_groups("0-3,4-7,8-17", 18), [0] * 4 + [1] * 4 + [2] * 10)
    np.testing.assert_array_equal(subspace.parse_layer_groups("5", 8), [-1] * 5 + [0] + [-1] * 2)
    np.testing.assert_array_equal(subspace.parse_layer_groups("4-7, 0-1", 10), [1, 1, -1, -1, 0, 0, 0, 0, -1, -1])      # frozen remainder
    lg = subspace.parse_layer_groups("0-3,4-7", 8)
    assert lg.dtype == np.int32 and subspace.n_groups(lg) == 2


@pytest.mark.parametrize("spec,msg", [
    ("0-3,2-5", r"range '2-5' overlaps an earlier range at layer 2"),
    ("3-1", r"range '3-1' is empty"),
    ("0-3,,4-7", r"range '' of '0-3,,4-7' is not LAYER or FIRST-LAST"),
    ("0-8", r"range '0-8' leaves the generator's style layers 0 .. 7"),
    ("8", r"range '8' leaves the generator's style layers 0 .. 7"),
    ("a-3", r"range 'a-3' of 'a-3' is not LAYER or FIRST-LAST"),
    ("1-2-3", r"range '1-2-3'"),
    ("-1", r"range '-1'"),
])
def test_parse_layer_groups_refusals(spec, msg):
    with pytest.raises(ValueError, match=msg):
        subspace.parse_layer_groups(spec, 8)


# ---- glass_subspace_supported ---------------------------------------------------------------------------------------
def test_library_declares_and_exports_the_subspace_abi():
    lib = engine.load_library()
    for name in ("glass_subspace_supported", "glass_engine_set_subspace_shape", "glass_engine_set_subspace", "glass_engine_expand_latents",
                 "glass_op_dlatent_subspace"):
        assert hasattr(lib, name), name
    assert engine.LATENT_SPACES["sub"] == 3 and engine.latent_space_id("sub") == 3


@pytest.mark.parametrize("n_lat,L,G,K,lg", [
    (18, 512, 1, 1, [0] * 18),                         # K = 1
    (18, 512, 1, 512, [0] * 18),                       # K = L (and the LDS limit)
    (8, 32, 1, 32, [0] * 8),                           # K = L
    (8, 32, 8, 4, list(range(8))),                     # G = n_lat
    (8, 32, 1, 4, [-1] * 7 + [0]),                     # all but one layer frozen
    (10, 64, 2, 7, [1, -1, 0, 0, 1, -1, 0, 1, 1, 1]),  # non-contiguous groups
    (18, 512, 3, 64, None),                            # the shape alone
])
def test_subspace_supported_accepts(n_lat, L, G, K, lg):
    assert engine.subspace_supported(n_lat, L, G, K, lg) == (True, "")
    assert engine.Engine.subspace_supported(n_lat, L, G, K, lg) == (True, "")


@pytest.mark.parametrize("n_lat,L,G,K,lg,msg", [
    (8, 32, 1, 0, [0] * 8, "components must be at least 1"),
    (8, 32, 1, 33, [0] * 8, "components must not exceed latent_size 32"),
    (18, 1024, 1, 513, [0] * 18, "components must not exceed 512"),
    (8, 30, 1, 4, [0] * 8, "latent_size 30 must be a multiple of 4"),
    (8, 32, 2, 4, [0] * 8, "group 1 is empty"),
    (8, 32, 2, 4, [0, 1, 2, 0, 0, 0, 0, 0], r"layer_group\[2\] = 2 must be -1 \(frozen\) or a group index in \[0, 2\)"),
    (8, 32, 9, 4, None, "groups must not exceed n_lat 8"),
    (8, 32, 0, 4, None, "groups must be at least 1"),
    (8, 32, 1, 4, [0, -2, 0, 0, 0, 0, 0, 0], r"layer_group\[1\] = -2"),
    (8, 32, 1, 4, [0] * 7, "layer_group must hold n_lat = 8 values, got 7"),
])
def test_subspace_supported_refuses(n_lat, L, G, K, lg, msg):
    ok, why = engine.subspace_supported(n_lat, L, G, K, lg)
    assert not ok
    assert __import__("re").search(msg, why), why


# ---- config / flags ---------------------------------------------------------------------------------------------------
def _cfg(name, **kw):
    c = types.SimpleNamespace(config=name)
    vars(c).update(gconfig.get_config(name))
    vars(c).update(kw)
    return c


SG2 = ["StyleGAN2_ffhq_d", "StyleGAN2_car_nod", "StyleGAN2_church_d"]


@pytest.mark.parametrize("name", SG2)
def test_options_accept_sub_on_the_stylegan2_configs(name):
    c = _cfg(name, latent_space="sub")
    assert generator.latent_options(c) == ("sub", 1.0, None)
    assert generator.subspace_options(c) == dict(components=64, layers=None, samples=None, basis=None)
    c = _cfg(name, latent_space="sub", subspace_components=1000, subspace_layers="0-3,4-7", subspace_samples=2048, truncation_psi=0.7)
    assert generator.latent_options(c) == ("sub", 0.7, None)
    assert generator.subspace_options(c) == dict(components=512, layers="0-3,4-7", samples=2048, basis=None)      # capped at dim_z
    assert generator.subspace_options(_cfg(name)) is None and generator.subspace_options(_cfg(name, latent_space="w+")) is None


def test_search_options_accept_sub_on_the_nod_configs():
    assert generator.search_options(_cfg("StyleGAN2_ffhq_nod", latent_space="sub", algorithm="cmaes")) == dict(sigma=1.0)
    with pytest.raises(ValueError, match="one objective"):
        generator.search_options(_cfg("StyleGAN2_ffhq_d", latent_space="sub", algorithm="cmaes"))


@pytest.mark.parametrize("name", ["DeepMindBigGAN256", "DeepMindBigGAN512", "GPT2"])
def test_options_refuse_sub_on_the_other_generators(name):
    with pytest.raises(ValueError, match="StyleGAN2 configs"):
        generator.latent_options(_cfg(name, latent_space="sub"))
    with pytest.raises(ValueError, match=r"subspace_components: latent space sub is a subspace of a StyleGAN2 generator's W; config '%s'" % name):
        generator.latent_options(_cfg(name, subspace_components=8))
    with pytest.raises(ValueError, match=r"latent space sub is a subspace of a StyleGAN2 generator's W; config '%s'" % name):
        generator.subspace_options(_cfg(name, latent_space="sub"))


@pytest.mark.parametrize("kw", [dict(subspace_components=8), dict(subspace_layers="0-3"), dict(subspace_samples=100), dict(subspace_basis="x.npz")])
@pytest.mark.parametrize("space", [None, "z", "w", "w+"])
def test_subspace_keys_need_the_space(kw, space):
    with pytest.raises(ValueError, match="%s set without latent_space 'sub'" % list(kw)[0]):
        generator.latent_options(_cfg("StyleGAN2_ffhq_d", latent_space=space, **kw))


def test_options_refuse_bad_values(tmp_path):
    with pytest.raises(ValueError, match="subspace_components must be at least 1"):
        generator.subspace_options(_cfg("StyleGAN2_ffhq_d", latent_space="sub", subspace_components=0))
    with pytest.raises(ValueError, match="subspace_samples=10 rows cannot carry 64 principal directions"):
        generator.subspace_options(_cfg("StyleGAN2_ffhq_d", latent_space="sub", subspace_samples=10))
    # a basis of another network's L
    path = str(tmp_path / "b32.npz")
    subspace.save(path, np.zeros(32), np.eye(32)[:4], np.ones(4), np.zeros(8, np.int32))
    with pytest.raises(ValueError, match="its directions have L = 32 entries and the network's dlatents 512"):
        generator.latent_options(_cfg("StyleGAN2_ffhq_d", latent_space="sub", subspace_basis=path))
    assert generator.subspace_options(_cfg("StyleGAN2_ffhq_d", latent_space="sub", subspace_basis=path, dim_z=32))["basis"] == path
    with pytest.raises(ValueError, match="holds 4 directions and subspace_components asks for 8"):
        generator.subspace_options(_cfg("StyleGAN2_ffhq_d", latent_space="sub", subspace_basis=path, dim_z=32, subspace_components=8))


def test_run_flags_reach_the_config_and_are_refused(tmp_path):
    a = run.build_parser().parse_args(["--latent-space", "sub", "--subspace-components", "8", "--subspace-layers", "0-3,4-7", "--subspace-samples",
                                       "512", "--subspace-basis", "b.npz"])
    assert (a.latent_space, a.subspace_components, a.subspace_layers, a.subspace_samples, a.subspace_basis) == ("sub", 8, "0-3,4-7", 512, "b.npz")
    d = run.build_parser().parse_args([])
    assert (d.subspace_components, d.subspace_layers, d.subspace_samples, d.subspace_basis) == (None, None, None, None)
    for cfg in ("DeepMindBigGAN256", "GPT2"):      # refused before any weight is looked for
        with pytest.raises(ValueError, match="StyleGAN2"):
            run.main(["--config", cfg, "--latent-space", "sub", "--tmp-folder", str(tmp_path)])
        with pytest.raises(ValueError, match="StyleGAN2"):
            run.main(["--config", cfg, "--subspace-components", "8", "--tmp-folder", str(tmp_path)])
    with pytest.raises(ValueError, match="subspace_layers set without latent_space 'sub'"):
        run.main(["--config", "StyleGAN2_ffhq_nod", "--subspace-layers", "0-3", "--tmp-folder", str(tmp_path)])


# ---- npz ----------------------------------------------------------------------------------------------------------------
def test_npz_round_trip(tmp_path):
    rng = np.random.RandomState(0)
    mean, comp, std = subspace.pca_basis(rng.normal(size=(64, 32)), 6)
    lg = subspace.parse_layer_groups("0-3,6-7", 8)
    path = str(tmp_path / "subspace.npz")
    subspace.save(path, mean, comp, std, lg)
    got = subspace.load(path, latent_size=32)
    assert sorted(got) == ["components", "layer_group", "mean", "stdev"]
    for k, v in (("mean", mean), ("components", comp), ("stdev", std), ("layer_group", lg)):
        assert got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), k
    with np.load(path) as f:
        assert sorted(f.files) == ["components", "layer_group", "mean", "stdev"]
    np.savez(str(tmp_path / "ganspace.npz"), mean=mean, components=comp, stdev=std)            # a plain GANSpace export: no groups
    assert subspace.load(str(tmp_path / "ganspace.npz"))["layer_group"] is None
    np.savez(str(tmp_path / "short.npz"), mean=mean, components=comp)
    with pytest.raises(ValueError, match=r"missing array\(s\) stdev"):
        subspace.load(str(tmp_path / "short.npz"))
    np.savez(str(tmp_path / "bent.npz"), mean=mean[:-1], components=comp, stdev=std)
    with pytest.raises(ValueError, match="do not fit"):
        subspace.load(str(tmp_path / "bent.npz"))
    basis, base = subspace.operands(mean, comp, std, 8)
    assert basis.shape == (6, 32) and base.shape == (8, 32) and basis.dtype == base.dtype == np.float32
    np.testing.assert_array_equal(basis, (std[:, None] * comp).astype(np.float32))
    np.testing.assert_array_equal(base, np.tile(mean.astype(np.float32), (8, 1)))
    np.testing.assert_array_equal(subspace.operands(mean, comp, std, 8, base=np.arange(256.0))[1], np.arange(256, dtype=np.float32).reshape(8, 32))
    with pytest.raises(ValueError, match=r"a w row\) or n_lat \* L = 256"):
        subspace.operands(mean, comp, std, 8, base=np.zeros(33))


# ---- width, state key, operators ---------------------------------------------------------------------------------------------
def test_latent_space_width_and_state_key():
    c = types.SimpleNamespace(batch_size=4, dim_z=32, channels=MINI_CHANNELS, latent_space="sub", subspace_components=8, subspace_layers="0-3,4-7")
    ls = StyleGAN2LatentSpace(c)
    assert ls.width == 16 and ls.population().shape == (4, 16) and ls.population().dtype == np.float32
    assert list(ls.state_dict()) == ["sub"]
    c.subspace_shape = (3, 5)                        # what the Generator settled on wins over the keys
    assert StyleGAN2LatentSpace(c).width == 15
    d = types.SimpleNamespace(batch_size=4, dim_z=32, channels=MINI_CHANNELS, latent_space="sub")
    assert StyleGAN2LatentSpace(d).width == 32       # one group of every layer, 64 directions capped at dim_z
    for space, key, width in (("z", "z", 32), ("w", "w", 32), ("w+", "w_plus", 8 * 32)):      # the others as they were
        ls = StyleGAN2LatentSpace(types.SimpleNamespace(batch_size=4, dim_z=32, channels=MINI_CHANNELS, latent_space=space))
        assert ls.width == width and list(ls.state_dict()) == [key]


def test_operators_sample_coefficients_as_z():
    c = _cfg("StyleGAN2_ffhq_nod", latent_space="sub", subspace_components=8)
    ops_ = operators.get_operators(c)
    assert isinstance(ops_["sampling"], operators.NormalRandomSampling)
    assert type(ops_["crossover"]) is type(operators.get_operators(_cfg("StyleGAN2_ffhq_nod"))["crossover"])
    e = operators.get_operators(_cfg("StyleGAN2_ffhq_nod", latent_space="sub", subspace_components=8, subspace_layers="0-3,4-7", edit_latent="w.npy",
                                     edit_sigma=0.2))
    assert isinstance(e["sampling"], operators.EditSampling) and e["sampling"].source_row.shape == (16,) and not e["sampling"].source_row.any()
    assert e["sampling"].sigma == 0.2
