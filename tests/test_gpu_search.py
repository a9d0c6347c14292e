"""The device search at engine level (include/glass.h "Device search"), on the mini StyleGAN2 of tests/glass_models.py: pop 8, batch 4, with a
discriminator (NSGA-II, two objectives) and without (GA).

Every generation is checked from the DEVICE's own state — the offspring against the float64 mirror (tests/search_device_ref.py) applied to the
population the device held, the survivors against the mirror applied to the device's own F — so that fp32 rounding in X never compounds into
a different search.  Bars: those of tests/test_gpu_search_ops.py (discrete outcomes exact, values within 2 fp32 ulps at the bound; survival
exact, distances bitwise)."""
import os
import pickle

import numpy as np
import pytest

import glass_models as M
import search_device_ref as SR

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
POP, BS, XL, XU = 8, 4, -10.0, 10.0
C = M.CONFIGS["mini"]


def make(with_d, seed=1, finalize=True, search=True):
    from clip_glass_amd.engine import Engine
    e = Engine(C["channels"][::-1], latent_size=C["latent"], mapping_layers=C["mapping"], batch_size=BS, use_discriminator=with_d,
               n_obj=2 if with_d else 1, max_pop=POP, clip=C["clip"], noise_mode=1, noise_seed=3)
    if search:
        e.set_search("nsga2" if with_d else "ga", POP, XL, XU, seed=seed)
    e.load_state(M.make_state("mini", 0, with_d=with_d))
    if finalize:
        e.finalize()
        e.set_target(np.random.default_rng(4).standard_normal(C["clip"][5]).astype(np.float32))
    return e


def x0():
    return np.random.default_rng(6).standard_normal((POP, C["latent"])).astype(np.float32)


ALL = ("X", "F", "rank", "cd", "off_X", "off_F", "flags", "counts")


@pytest.mark.parametrize("with_d", [True, False])
def test_evaluate_rows_and_halves(with_d):
    e = make(with_d)
    X0 = x0()
    e.search_init(X0)
    # generation 0: the population is X0 ranked by the mirror's survival of the pass's own F
    F0 = e.evaluate(X0, generation=0)
    p = e.search_read("X", "F", "rank", "cd")
    ref = SR.survive(F0, POP, POP, with_d)
    assert np.array_equal(SR.bits(p["X"]), SR.bits(X0[ref["chosen"]])) and np.array_equal(SR.bits(p["F"]), SR.bits(F0[ref["chosen"]]))
    assert np.array_equal(p["rank"], ref["rank"]) and np.array_equal(p["cd"].view(np.uint64), ref["cd"].view(np.uint64))
    # search_evaluate's F is glass_engine_evaluate's on the read-back offspring of the same generation
    e.search_vary(1)
    e.search_evaluate(1)
    one = e.search_read("off_X", "off_F")
    assert np.array_equal(SR.bits(one["off_F"]), SR.bits(e.evaluate(one["off_X"], generation=1)))
    e.search_survive(1)
    s1 = e.search_read("X", "F", "rank", "cd")
    # the offspring scored as two halves: the same F bits and the same survivors
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


@pytest.mark.parametrize("with_d", [True, False])
def test_three_generations_against_mirror(with_d):
    seed = 1
    e = make(with_d, seed)
    e.search_init(x0())
    for gen in (1, 2, 3):
        b = e.search_read("X", "F", "rank", "cd")
        e.search_step(gen)
        a = e.search_read(*ALL)
        m = SR.vary(b["X"], b["rank"], b["cd"], XL, XU, 3.0, 3.0, 0.5, seed, gen)
        SR.check_offspring("engine d=%d gen %d" % (with_d, gen), a["off_X"], b["X"], m, XL, XU)
        assert np.array_equal(a["flags"], SR.duplicates(b["X"], a["off_X"]))
        Fm, Xm = np.concatenate([b["F"], a["off_F"]]), np.concatenate([b["X"], a["off_X"]])
        got = dict(chosen=None, rank=a["rank"], cd=a["cd"], counts=a["counts"], F=a["F"], X=a["X"])
        ref = SR.survive(Fm, POP, POP, with_d, a["flags"])
        got["chosen"] = ref["chosen"]      # (the engine keeps the rows, not the indices: X and F below pin them)
        SR.check_survival("engine d=%d gen %d" % (with_d, gen), got, Fm, POP, POP, with_d, a["flags"], Xm)
        assert np.isfinite(a["off_F"]).all() and (a["off_F"][:, 0] != a["off_F"][0, 0]).any()
    e.close()


def test_seed_decides_the_search():
    finals = []
    for seed in (1, 1, 2):
        e = make(True, seed)
        e.search_init(x0())
        for gen in (1, 2, 3):
            e.search_step(gen)
        finals.append(e.search_read("X")["X"])
        e.close()
    assert np.array_equal(SR.bits(finals[0]), SR.bits(finals[1]))
    assert not np.array_equal(SR.bits(finals[0]), SR.bits(finals[2]))


def test_call_order_refusals():
    e = make(True)
    with pytest.raises(RuntimeError, match="set_search: the engine is finalized"):
        e.set_search("nsga2", POP, XL, XU)
    with pytest.raises(RuntimeError, match=r"search_step: search_init\(\) first"):
        e.search_step(1)
    e.search_init(x0())
    with pytest.raises(RuntimeError, match="search_vary of this generation first"):
        e.search_evaluate(1)
    e.close()
    e = make(True, search=False)
    with pytest.raises(RuntimeError, match="the device search is off"):
        e.search_init(x0())
    e.close()
    from clip_glass_amd.engine import Engine
    b = M.BIGGAN_CONFIGS["bg_mini"]
    eb = Engine([], batch_size=4, max_pop=8, clip=b["clip"],
                biggan=dict(layers=b["layers"], attention_pos=b["attention_pos"], ch=b["ch"], z_dim=b["z_dim"], num_classes=b["num_classes"]))
    with pytest.raises(RuntimeError, match="BigGAN"):
        eb.set_search("ga", 8, -2, 2)
    eb.close()
    e = make(True, finalize=False, search=False)
    with pytest.raises(RuntimeError, match="multiple of batch_size"):
        e.set_search("nsga2", 6, XL, XU)
    with pytest.raises(RuntimeError, match="n_obj = 1"):
        e.set_search("ga", POP, XL, XU)
    e.close()


def _run(tmp, monkeypatch, space, device):
    from clip_glass_amd import run
    from clip_glass_amd.engine import Engine
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_problem.npz")))
    extra = dict(channels=C["channels"], dim_z=C["latent"], mapping_layers=C["mapping"], clip_geometry=C["clip"],
                 clip_text_geometry=dict(width=64, layers=2), target_features=g["text_features"],
                 problem_args=dict(n_var=C["latent"], n_obj=2, n_constr=C["latent"], xl=-10, xu=10))
    steps = []
    inner = Engine.search_step

    def recording(self, generation):
        if not steps:
            steps.append((0, self.search_read("F")["F"], self.latent_uploads()))
        inner(self, generation)
        steps.append((generation, self.search_read("F")["F"], self.latent_uploads()))
    monkeypatch.setattr(Engine, "search_step", recording)
    os.makedirs(tmp, exist_ok=True)
    argv = ["--config", "StyleGAN2_ffhq_d", "--generations", "3", "--save-each", "100", "--tmp-folder", tmp, "--weights", "synthetic:0",
            "--clip-weights", "synthetic:0", "--pop-size", "8", "--latent-space", space] + (["--device-search"] if device else [])
    return run.main(argv, extra_config=extra), steps


@pytest.mark.parametrize("space", ["z", "w+"])
def test_minimize_device_through_run(tmp_path, monkeypatch, space):
    res, steps = _run(str(tmp_path / "dev"), monkeypatch, space, True)
    host, none = _run(str(tmp_path / "host"), monkeypatch, space, False)
    assert not none and [s[0] for s in steps] == [0, 1, 2, 3]
    width = C["latent"] * (8 if space == "w+" else 1)
    # today's shapes: the first front, and the population
    for r in (res, host):
        assert np.atleast_2d(r.X).shape[1] == width and np.atleast_2d(r.F).shape[1] == 2 and np.atleast_2d(r.X).shape[0] == np.atleast_2d(r.F).shape[0]
        assert len(r.pop) == 8 and r.pop[0].X.shape == (width,) and r.pop[0].F.shape == (2,) and r.G.shape == r.CV.shape == (np.atleast_2d(r.X).shape[0],)
    # elitism: the best similarity objective never gets worse
    best = [float(F[:, 0].min()) for _, F, _ in steps]
    assert all(b1 <= b0 for b0, b1 in zip(best, best[1:])), best
    # no host-to-device latent copy by the pass after generation 0
    assert all(up == steps[0][2] for _, _, up in steps), [s[2] for s in steps]
    # the same set of result files as the run without the flag
    assert sorted(os.listdir(str(tmp_path / "dev"))) == sorted(os.listdir(str(tmp_path / "host")))
    assert set(pickle.load(open(str(tmp_path / "dev" / "genetic_result"), "rb"))) == {"X", "F", "G", "CV"}
