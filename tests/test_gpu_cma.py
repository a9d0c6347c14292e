"""The sep-CMA-ES device search at engine level (include/glass.h "Device search: sep-CMA-ES"), on the mini StyleGAN2 of
tests/glass_models.py: pop 8, batch 4, no discriminator (one objective).

Every generation is checked from the DEVICE's own state, as tests/test_gpu_search.py does it: the samples against the float64 mirror
(tests/cma_ref.py) applied to the state the device held, the update against the mirror applied to the device's own rows and F — so that
fp32 rounding never compounds into a different search.  Bars: those of tests/test_gpu_cma_ops.py."""
import os
import pickle

import numpy as np
import pytest

import cma_ref as CR
import glass_models as M

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
POP, BS, XL, XU = 8, 4, -10.0, 10.0
C = M.CONFIGS["mini"]
N = C["latent"]


def make(seed=1, with_d=False, finalize=True, search="cmaes"):
    from clip_glass_amd.engine import Engine
    e = Engine(C["channels"][::-1], latent_size=C["latent"], mapping_layers=C["mapping"], batch_size=BS, use_discriminator=with_d,
               n_obj=2 if with_d else 1, max_pop=POP, clip=C["clip"], noise_mode=1, noise_seed=3)
    if search:
        e.set_search(search, POP, XL, XU, seed=seed)
    e.load_state(M.make_state("mini", 0, with_d=with_d))
    if finalize:
        e.finalize()
        e.set_target(np.random.default_rng(4).standard_normal(C["clip"][5]).astype(np.float32))
    return e


def start():
    rng = np.random.default_rng(6)
    return 0.3 * rng.standard_normal(N), rng.uniform(0.5, 2.0, N), 0.8


def mirror_state(c):
    return dict(m=c["mean"], d=c["diag"], ps=c["p_sigma"], pc=c["p_c"], sigma=c["sigma"], ps_norm=c["ps_norm"], h=c["h"], finite=c["finite"],
                updated=c["updated"], skipped=c["skipped"], updates=c["updates"], best_X=c["best_X"], best_F=c["best_F"])


def test_three_generations_against_mirror():
    seed = 5
    e = make(seed)
    e.search_init_cma(*start())
    uploads = e.latent_uploads()
    first = e.search_read_cma()
    assert np.array_equal(first["mean"], start()[0]) and np.array_equal(first["diag"], start()[1]) and first["sigma"] == 0.8
    assert not first["p_sigma"].any() and not first["p_c"].any() and np.isinf(first["best_F"]) and first["updates"] == first["skipped"] == 0
    seen = []
    for g in (0, 1, 2):
        st = mirror_state(e.search_read_cma())
        e.search_step(g)
        a, c = e.search_read("off_X", "off_F", "counts"), e.search_read_cma()
        CR.check_sample("engine gen %d" % g, a["off_X"], st, POP, XL, XU, seed, g)
        assert np.isfinite(a["off_F"]).all() and (a["off_F"][:, 0] != a["off_F"][0, 0]).any() and list(a["counts"]) == [0, 0]
        ref, mag = CR.update(st, a["off_X"], a["off_F"][:, 0], POP, XL, XU, g)
        got = mirror_state(c)
        got["order"] = ref["order"]      # (the engine keeps the state, not the order: the state below pins it)
        CR.check_update("engine gen %d" % g, got, ref, mag)
        assert c["updates"] == g + 1 and c["skipped"] == 0
        seen.append(a["off_F"][:, 0])
    assert e.latent_uploads() == uploads      # no host-to-device latent copy after init
    assert c["best_F"] == float(np.concatenate(seen).min())
    e.close()


def test_rows_scored_whole_and_as_halves():
    e = make()
    e.search_init_cma(*start())
    e.search_vary(0)
    e.search_evaluate(0)
    one = e.search_read("off_X", "off_F")
    e.search_survive(0)
    s1 = e.search_read_cma()
    assert np.array_equal(CR.bits(one["off_F"]), CR.bits(e.evaluate(one["off_X"], generation=0)))
    e.search_init_cma(*start())
    e.search_vary(0)
    e.search_evaluate(0, 0, 4)
    e.search_evaluate(0, 4, 4)
    two = e.search_read("off_X", "off_F")
    assert np.array_equal(CR.bits(two["off_X"]), CR.bits(one["off_X"])) and np.array_equal(CR.bits(two["off_F"]), CR.bits(one["off_F"]))
    e.search_survive(0)
    s2 = e.search_read_cma()
    for k in s1:
        assert np.array_equal(np.asarray(s1[k]), np.asarray(s2[k])), k
    assert s1["updates"] == 1 and s1["best_F"] == float(one["off_F"].min())
    e.close()


def test_seed_decides_the_search():
    finals = []
    for seed in (1, 1, 2):
        e = make(seed)
        e.search_init_cma(*start())
        for g in (0, 1, 2):
            e.search_step(g)
        finals.append(e.search_read_cma()["mean"])
        e.close()
    assert np.array_equal(CR.bits(finals[0]), CR.bits(finals[1])) and not np.array_equal(CR.bits(finals[0]), CR.bits(finals[2]))


def test_refusals_by_name():
    from clip_glass_amd.engine import Engine
    x0 = np.zeros((POP, N), np.float32)
    e = make()
    with pytest.raises(RuntimeError, match="set_search: the engine is finalized"):
        e.set_search("cmaes", POP, XL, XU)
    with pytest.raises(RuntimeError, match=r"search_step: search_init_cma\(\) first"):
        e.search_step(0)
    with pytest.raises(RuntimeError, match=r"search_init: a cmaes search keeps a distribution"):
        e.search_init(x0)
    with pytest.raises(RuntimeError, match="sigma0 must be finite and positive"):
        e.search_init_cma(np.zeros(N), None, 0.0)
    e.search_init_cma(np.zeros(N))
    with pytest.raises(RuntimeError, match="search_vary of this generation first"):
        e.search_evaluate(0)
    with pytest.raises(RuntimeError, match="search_survive: search_vary and search_evaluate of this generation first"):
        e.search_survive(0)
    with pytest.raises(RuntimeError, match="a cmaes search has no population"):
        e.search_read("X")
    e.close()
    e = make(search="ga")
    with pytest.raises(RuntimeError, match="search_init_cma: this engine's search is ga / nsga2"):
        e.search_init_cma(np.zeros(N))
    e.close()
    e = make(with_d=True, finalize=False, search=None)
    with pytest.raises(RuntimeError, match="cmaes minimises one objective and this engine has 2"):
        e.set_search("cmaes", POP, XL, XU)
    e.close()
    e = make(finalize=False, search=None)
    with pytest.raises(RuntimeError, match="multiple of batch_size"):
        e.set_search("cmaes", 6, XL, XU)
    e.close()
    b = M.BIGGAN_CONFIGS["bg_mini"]
    eb = Engine([], batch_size=4, max_pop=8, clip=b["clip"],
                biggan=dict(layers=b["layers"], attention_pos=b["attention_pos"], ch=b["ch"], z_dim=b["z_dim"], num_classes=b["num_classes"]))
    with pytest.raises(RuntimeError, match="cmaes samples real-valued rows; a BigGAN row holds boolean class bits"):
        eb.set_search("cmaes", 8, -2, 2)
    eb.close()


def _run(tmp, monkeypatch, space, algorithm):
    from clip_glass_amd import run
    from clip_glass_amd.engine import Engine
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_problem.npz")))
    extra = dict(channels=C["channels"], dim_z=C["latent"], mapping_layers=C["mapping"], clip_geometry=C["clip"],
                 clip_text_geometry=dict(width=64, layers=2), target_features=g["text_features"],
                 problem_args=dict(n_var=C["latent"], n_obj=1, n_constr=C["latent"], xl=-10, xu=10))
    steps = []
    inner = getattr(Engine.search_step, "inner", Engine.search_step)      # (a second run in one test wraps the method itself, not the first wrapper)

    def recording(self, generation):
        inner(self, generation)
        if algorithm == "cmaes":
            r = self.search_read("off_X", "off_F")
            steps.append((generation, r["off_X"], r["off_F"], self.search_read_cma(), self.evaluate(r["off_X"], generation=generation)))
    recording.inner = inner
    monkeypatch.setattr(Engine, "search_step", recording)
    os.makedirs(tmp, exist_ok=True)
    argv = ["--config", "StyleGAN2_ffhq_nod", "--generations", "3", "--save-each", "100", "--tmp-folder", tmp, "--weights", "synthetic:0",
            "--clip-weights", "synthetic:0", "--pop-size", "8", "--latent-space", space, "--device-search"]
    return run.main(argv + (["--algorithm", "cmaes", "--cma-sigma", "0.5"] if algorithm == "cmaes" else []), extra_config=extra), steps


@pytest.mark.parametrize("space", ["z", "w+"])
def test_minimize_device_through_run(tmp_path, monkeypatch, space):
    res, steps = _run(str(tmp_path / "cma"), monkeypatch, space, "cmaes")
    _run(str(tmp_path / "ga"), monkeypatch, space, "ga")
    assert [s[0] for s in steps] == [0, 1, 2, 3]
    width = C["latent"] * (8 if space == "w+" else 1)
    assert res.X.shape == (width,) and res.F.shape == (1,) and len(res.pop) == 8 and res.pop[0].X.shape == (width,) and res.mean.shape == (width,)
    assert res.sigma > 0 and np.isfinite(res.mean).all()
    # the pass's own F for the rows read back, the best-so-far never worse, and the result row scores to its reported F
    best = [s[3]["best_F"] for s in steps]
    assert all(b1 <= b0 for b0, b1 in zip(best, best[1:])), best
    for _, X, F, _, again in steps:
        assert np.array_equal(CR.bits(F), CR.bits(again))
    allX, allF = np.concatenate([s[1] for s in steps]), np.concatenate([s[2] for s in steps])[:, 0]
    assert float(res.F[0]) == float(allF.min()) == best[-1]
    hit = np.nonzero((allX == res.X.astype(np.float32)).all(axis=1))[0]
    assert hit.size and (allF[hit] == np.float32(res.F[0])).any()
    # the same set of result files as the GA's device run
    assert sorted(os.listdir(str(tmp_path / "cma"))) == sorted(os.listdir(str(tmp_path / "ga")))
    assert set(pickle.load(open(str(tmp_path / "cma" / "genetic_result"), "rb"))) == {"X", "F", "G", "CV"}
