"""The device search on mixed rows at engine level (include/glass.h "Device search", paragraph "Mixed rows"), on the mini BigGAN of
tests/glass_models.py: z 16, 24 classes, pop 8, batch 4, GA.

As tests/test_gpu_search.py, every generation is checked from the DEVICE's own state: the offspring against the mirror
(tests/search_mixed_ref.py) applied to the population the device held — bit columns exactly, real columns at test_gpu_search_ops.py's bars —
F against the engine's own evaluate of those rows, the survivors against search_device_ref.survive of the device's own F."""
import os
import pickle

import numpy as np
import pytest

import glass_models as M
import search_device_ref as SR
import search_mixed_ref as MR
from clip_glass_amd import synth

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
POP, BS, XL, XU = 8, 4, -2.0, 2.0
PROB_X, PROB_FLIP = 0.2, 10 / 1000
C = M.BIGGAN_CONFIGS["bg_mini"]
ZD, NC = C["z_dim"], C["num_classes"]
ALL = ("X", "F", "rank", "cd", "off_X", "off_F", "flags", "counts")


def make(seed=1, finalize=True, search=True, prob_x=PROB_X, prob_flip=PROB_FLIP):
    from clip_glass_amd.engine import Engine
    e = Engine([], batch_size=BS, max_pop=POP, clip=C["clip"],
               biggan=dict(layers=C["layers"], attention_pos=C["attention_pos"], ch=C["ch"], z_dim=ZD, num_classes=NC))
    if search:
        e.set_search_mixed("ga", POP, ZD, XL, XU, prob_x=prob_x, prob_flip=prob_flip, seed=seed)
    e.load_state(M.make_biggan_state("bg_mini", 0))
    if finalize:
        e.finalize()
        e.set_target(np.random.default_rng(4).standard_normal(C["clip"][5]).astype(np.float32))
    return e


def x0():
    """Truncated-normal z and a few class bits per row, as the BigGAN configs' sampler draws them."""
    x = synth.biggan_population(6, POP, ZD, NC).astype(np.float32)
    x[:, :ZD] = np.clip(x[:, :ZD], XL, XU)
    bits = np.random.default_rng(8).random((POP, NC)) < 0.15
    x[:, ZD:] = bits
    return x


@pytest.mark.parametrize("prob_x,prob_flip", [(PROB_X, PROB_FLIP), (1.0, 0.05)])
def test_three_generations_against_mirror(prob_x, prob_flip):
    seed = 1
    e = make(seed, prob_x=prob_x, prob_flip=prob_flip)
    assert (e.search_pop, e.search_n_real) == (POP, ZD)
    e.search_init(x0())
    exchanged = 0
    for gen in (1, 2, 3):
        b = e.search_read("X", "F", "rank", "cd")
        e.search_step(gen)
        a = e.search_read(*ALL)
        name = "engine mixed prob_x %g gen %d" % (prob_x, gen)
        m = MR.vary_mixed(b["X"], ZD, b["rank"], b["cd"], XL, XU, 3.0, 3.0, 0.5, prob_x, prob_flip, seed, gen)
        MR.check_bits(name, a["off_X"][:, ZD:], m)
        SR.check_offspring(name, a["off_X"][:, :ZD], b["X"][:, :ZD], m["real"], XL, XU)
        exchanged += sum(s.size for s in m["selected"])
        assert np.array_equal(a["flags"], SR.duplicates(b["X"], a["off_X"]))
        assert np.array_equal(SR.bits(a["off_F"]), SR.bits(e.evaluate(a["off_X"], generation=gen)))
        Fm, Xm = np.concatenate([b["F"], a["off_F"]]), np.concatenate([b["X"], a["off_X"]])
        ref = SR.survive(Fm, POP, POP, False, a["flags"])
        got = dict(chosen=ref["chosen"], rank=a["rank"], cd=a["cd"], counts=a["counts"], F=a["F"], X=a["X"])      # (the engine keeps the rows)
        SR.check_survival(name, got, Fm, POP, POP, False, a["flags"], Xm)
        assert np.isfinite(a["off_F"]).all() and (a["off_F"][:, 0] != a["off_F"][0, 0]).any()
    assert exchanged > 0 or prob_x < 1.0
    p = e.search_read("X")["X"]
    assert (p[:, :ZD] >= XL).all() and (p[:, :ZD] <= XU).all() and np.isin(p[:, ZD:], (0.0, 1.0)).all()
    e.close()


def test_evaluate_in_halves_equals_whole():
    e = make()
    X0 = x0()
    e.search_init(X0)
    F0 = e.evaluate(X0, generation=0)
    p = e.search_read("X", "F")
    ref = SR.survive(F0, POP, POP, False)
    assert np.array_equal(SR.bits(p["X"]), SR.bits(X0[ref["chosen"]])) and np.array_equal(SR.bits(p["F"]), SR.bits(F0[ref["chosen"]]))
    e.search_vary(1)
    e.search_evaluate(1)
    one = e.search_read("off_X", "off_F")
    e.search_survive(1)
    s1 = e.search_read("X", "F", "rank", "cd")
    e.search_init(X0)
    e.search_vary(1)
    e.search_evaluate(1, 0, 4)
    e.search_evaluate(1, 4, 4)
    two = e.search_read("off_X", "off_F")
    assert np.array_equal(SR.bits(two["off_X"]), SR.bits(one["off_X"])) and np.array_equal(SR.bits(two["off_F"]), SR.bits(one["off_F"]))
    e.search_survive(1)
    s2 = e.search_read("X", "F", "rank", "cd")
    for k in s1:
        assert np.array_equal(s1[k].view(np.uint8), s2[k].view(np.uint8)), k
    e.close()


def test_seed_decides_the_search_and_nothing_is_uploaded():
    finals = []
    for seed in (1, 1, 2):
        e = make(seed)
        e.search_init(x0())
        up0 = e.latent_uploads()
        for gen in (1, 2, 3):
            e.search_step(gen)
            assert e.latent_uploads() == up0      # no host-to-device latent copy after generation 0
        finals.append(e.search_read("X")["X"])
        e.close()
    assert np.array_equal(SR.bits(finals[0]), SR.bits(finals[1]))
    assert not np.array_equal(SR.bits(finals[0]), SR.bits(finals[2]))
    for p in finals:
        assert (p[:, :ZD] >= XL).all() and (p[:, :ZD] <= XU).all() and np.isin(p[:, ZD:], (0.0, 1.0)).all()


def test_search_init_refuses_a_value_that_is_no_bit():
    e = make()
    X = x0()
    X[5, ZD + 3] = 0.5
    with pytest.raises(RuntimeError, match="row 5 column %d" % (ZD + 3)):
        e.search_init(X)
    with pytest.raises(RuntimeError, match=r"search_init\(\) first"):
        e.search_step(1)
    X[5, ZD + 3] = 1.0
    e.search_init(X)
    e.search_step(1)
    e.close()


def test_set_search_mixed_refusals():
    from clip_glass_amd.engine import Engine
    e = make()
    with pytest.raises(RuntimeError, match="set_search_mixed: the engine is finalized"):
        e.set_search_mixed("ga", POP, ZD, XL, XU)
    with pytest.raises(RuntimeError, match=r"prob_x and prob_flip must be in \[0, 1\]"):
        e.set_search_operators_mixed(XL, XU, prob_x=1.5)
    e.close()
    e = make(finalize=False, search=False)
    with pytest.raises(RuntimeError, match="n_real must be z_dim = %d" % ZD):
        e.set_search_mixed("ga", POP, ZD - 4, XL, XU)
    with pytest.raises(RuntimeError, match="multiple of batch_size"):
        e.set_search_mixed("ga", 6, ZD, XL, XU)
    with pytest.raises(RuntimeError, match=r"prob_x and prob_flip must be in \[0, 1\]"):
        e.set_search_mixed("ga", POP, ZD, XL, XU, prob_flip=-0.1)
    with pytest.raises(RuntimeError, match="BigGAN.*set_search_mixed"):
        e.set_search("ga", POP, XL, XU)
    with pytest.raises(RuntimeError, match="no mixed device search is on"):
        e.set_search_operators_mixed(XL, XU)
    assert not hasattr(e, "search_n_real")
    e.close()
    s = M.CONFIGS["mini"]
    es = Engine(s["channels"][::-1], latent_size=s["latent"], mapping_layers=s["mapping"], batch_size=BS, use_discriminator=False, n_obj=1,
                max_pop=POP, clip=s["clip"], noise_mode=1, noise_seed=3)
    with pytest.raises(RuntimeError, match="StyleGAN2 row has no bit columns"):
        es.set_search_mixed("ga", POP, s["latent"], XL, XU)
    es.close()


def _run(tmp, device):
    from clip_glass_amd import run
    target = np.random.default_rng(4).standard_normal(C["clip"][5]).astype(np.float32)
    extra = dict(weights="synthetic:0", clip_weights="synthetic:0", dim_z=ZD, num_classes=NC,
                 biggan_geometry=dict(layers=C["layers"], attention_pos=C["attention_pos"], ch=C["ch"]),
                 clip_geometry=C["clip"], target_features=target, batch_size=BS,
                 problem_args=dict(n_var=ZD + NC, n_obj=1, n_constr=ZD, xl=-2, xu=2))
    os.makedirs(tmp, exist_ok=True)
    argv = ["--config", "DeepMindBigGAN512", "--generations", "3", "--save-each", "100", "--tmp-folder", tmp, "--pop-size", "8"]
    return run.main(argv + (["--device-search"] if device else []), extra_config=extra)


def test_minimize_device_through_run(tmp_path):
    res = _run(str(tmp_path / "dev"), True)
    host = _run(str(tmp_path / "host"), False)
    for r in (res, host):
        assert np.asarray(r.X).shape == (ZD + NC,) and np.asarray(r.F).shape == (1,) and len(r.pop) == POP and r.pop[0].X.shape == (ZD + NC,)
        assert r.G.shape == r.CV.shape == (1,)
    X = np.stack([p.X for p in res.pop])
    assert (X[:, :ZD] >= XL).all() and (X[:, :ZD] <= XU).all() and np.isin(X[:, ZD:], (0.0, 1.0)).all()
    assert sorted(os.listdir(str(tmp_path / "dev"))) == sorted(os.listdir(str(tmp_path / "host")))
    d = pickle.load(open(str(tmp_path / "dev" / "genetic_result"), "rb"))
    assert set(d) == {"X", "F", "G", "CV"} and np.atleast_2d(d["X"]).shape[1] == ZD + NC
