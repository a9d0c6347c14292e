"""Island populations at engine level (include/glass.h "Device search: islands"), on the mini StyleGAN2 and the mini BigGAN of
tests/glass_models.py: pop 8 per island, batch 4.

Every bar is exact.  Without migration island i of one engine equals, bit for bit and buffer by buffer, a single-search engine under seed + i
started from the island's own rows — the offspring, their F under the island's noise planes, the flags, the survivors, their ranks and
distances.  A migration is checked from the DEVICE's own state: the populations read back behind search_survive go through the mirror
(tests/search_islands_ref.py) and must equal what search_migrate leaves.  Each test also asserts that the offspring F are finite and not all
equal, so that no equality holds vacuously."""
import os

import numpy as np
import pytest

import glass_models as M
import search_device_ref as SR
import search_islands_ref as IR
from clip_glass_amd import synth

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GLASS_EMULATE")), reason="launches the library's own kernels: no emulated form")]
POP, BS, XL, XU = 8, 4, -10.0, 10.0
C = M.CONFIGS["mini"]
B = M.BIGGAN_CONFIGS["bg_mini"]
ALL = ("X", "F", "rank", "cd", "off_X", "off_F", "flags")


def make(with_d, seed=1, islands=None, migrate_every=0, migrants=1, pop=POP, finalize=True):
    """islands None: a single search (the setter is never called)."""
    from clip_glass_amd.engine import Engine
    e = Engine(C["channels"][::-1], latent_size=C["latent"], mapping_layers=C["mapping"], batch_size=BS, use_discriminator=with_d,
               n_obj=2 if with_d else 1, max_pop=pop * (islands or 1), clip=C["clip"], noise_mode=1, noise_seed=3)
    e.set_search("nsga2" if with_d else "ga", pop, XL, XU, seed=seed)
    if islands is not None:
        e.set_search_islands(islands, migrate_every, migrants)
    e.load_state(M.make_state("mini", 0, with_d=with_d))
    if finalize:
        e.finalize()
        e.set_target(np.random.default_rng(4).standard_normal(C["clip"][5]).astype(np.float32))
    return e


def make_bg(seed=1, islands=None):
    from clip_glass_amd.engine import Engine
    e = Engine([], batch_size=BS, max_pop=POP * (islands or 1), clip=B["clip"],
               biggan=dict(layers=B["layers"], attention_pos=B["attention_pos"], ch=B["ch"], z_dim=B["z_dim"], num_classes=B["num_classes"]))
    e.set_search_mixed("ga", POP, B["z_dim"], -2.0, 2.0, prob_x=0.5, prob_flip=0.02, seed=seed)
    if islands is not None:
        e.set_search_islands(islands)
    e.load_state(M.make_biggan_state("bg_mini", 0))
    e.finalize()
    e.set_target(np.random.default_rng(4).standard_normal(B["clip"][5]).astype(np.float32))
    return e


def x0(K, pop=POP):
    return np.random.default_rng(6).standard_normal((K, pop, C["latent"])).astype(np.float32)


def x0_bg(K):
    zd, nc = B["z_dim"], B["num_classes"]
    x = synth.biggan_population(6, K * POP, zd, nc).astype(np.float32)
    x[:, :zd] = np.clip(x[:, :zd], -2.0, 2.0)
    x[:, zd:] = np.random.default_rng(8).random((K * POP, nc)) < 0.15
    return x.reshape(K, POP, zd + nc)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def lively(off_F):
    assert np.isfinite(off_F).all() and (off_F[..., 0] != off_F.reshape(-1, off_F.shape[-1])[0, 0]).any()


def islands_equal_single_searches(isl, singles, X0, generations=(1, 2, 3)):
    K = len(singles)
    isl.search_init(X0.reshape(K * X0.shape[1], -1))
    for i, e in enumerate(singles):
        e.search_init(X0[i])
    uploads = isl.latent_uploads()
    for gen in (0,) + tuple(generations):
        if gen:
            isl.search_step(gen)
        a = isl.search_read(*(ALL if gen else ALL[:4]), islands=True)
        for i, e in enumerate(singles):
            if gen:
                e.search_step(gen)
            s = e.search_read(*(ALL if gen else ALL[:4]))
            for k in s:
                assert same(a[k][i], s[k]), "generation %d island %d: %s" % (gen, i, k)
        if gen:
            lively(a["off_F"])
            assert not same(a["off_X"][0], a["off_X"][1])
            assert np.array_equal(isl.search_read_islands()[:, :2].sum(axis=0), isl.search_read("counts")["counts"])
    assert isl.latent_uploads() == uploads      # no host-to-device latent copy over the island generations


@pytest.mark.parametrize("with_d", [True, False])
def test_islands_equal_separate_searches(with_d):
    K, seed = 3, 5
    isl = make(with_d, seed, islands=K)
    singles = [make(with_d, seed + i) for i in range(K)]
    islands_equal_single_searches(isl, singles, x0(K))
    for e in [isl] + singles:
        e.close()


def test_islands_equal_separate_searches_mixed_rows():
    K, seed = 2, 2 ** 64 - 1      # (island 1's seed wraps to 0)
    isl = make_bg(seed, islands=K)
    singles = [make_bg((seed + i) % 2 ** 64) for i in range(K)]
    islands_equal_single_searches(isl, singles, x0_bg(K))
    for e in [isl] + singles:
        e.close()


@pytest.mark.parametrize("with_d", [True, False])
def test_migration_against_mirror_from_the_device_state(with_d):
    K, n = 3, 2
    e = make(with_d, 3, islands=K, migrate_every=1, migrants=n)
    twin = make(with_d, 3, islands=K, migrate_every=1, migrants=n)      # the same generations through search_step
    X0 = x0(K).reshape(K * POP, -1)
    e.search_init(X0)
    twin.search_init(X0)
    moved = 0
    for gen in (1, 2):
        e.search_vary(gen)
        e.search_evaluate(gen)
        e.search_survive(gen)
        pre = e.search_read("X", "F", "rank", "cd", "off_F", islands=True)
        lively(pre["off_F"])
        e.search_migrate(gen)
        post = e.search_read("X", "F", "rank", "cd", islands=True)
        post["accepted"] = e.search_read_islands()[:, 2]
        ref = IR.check_migration("engine d=%d generation %d" % (with_d, gen), post, pre["X"], pre["F"], pre["rank"], pre["cd"], n, with_d)
        moved += int(ref["accepted"].sum())
        twin.search_step(gen)
        t = twin.search_read("X", "F", "rank", "cd", islands=True)
        for k in t:
            assert same(t[k], post[k]), "search_step against the phases, generation %d: %s" % (gen, k)
        assert same(twin.search_read_islands(), e.search_read_islands())
    assert moved > 0
    with pytest.raises(RuntimeError, match="search_migrate: search_survive of this generation first"):
        e.search_migrate(2)
    e.close()
    twin.close()


def test_migration_not_due_changes_nothing():
    e = make(False, 3, islands=2, migrate_every=2, migrants=1)
    e.search_init(x0(2).reshape(2 * POP, -1))
    e.search_vary(1)
    e.search_evaluate(1)
    e.search_survive(1)
    pre = e.search_read("X", "F", "rank", "cd")
    e.search_migrate(1)      # generation 1 with M = 2: none due
    post = e.search_read("X", "F", "rank", "cd")
    assert all(same(pre[k], post[k]) for k in pre) and (e.search_read_islands()[:, 2] == 0).all()
    e.close()


@pytest.mark.parametrize("K,pop", [(3, 384), (2, 1024)])
def test_more_rows_than_one_workgroup_ranks(K, pop):
    """3 x 384 = 1152 rows, above the 1024 a single search can hold, and 2 x 1024 (each island's survival then ranks 2048 merged rows in more
    than 64 KB of LDS): the last island against one single-search engine of pop rows."""
    seed = 9
    isl = make(True, seed, islands=K, pop=pop)
    one = make(True, seed + K - 1, pop=pop)
    X0 = x0(K, pop)
    isl.search_init(X0.reshape(K * pop, -1))
    one.search_init(X0[K - 1])
    isl.search_step(1)
    one.search_step(1)
    a, s = isl.search_read(*ALL, islands=True), one.search_read(*ALL)
    for k in s:
        assert same(a[k][K - 1], s[k]), k
    lively(a["off_F"])
    isl.close()
    one.close()


@pytest.mark.parametrize("with_d", [True, False])
def test_own_prompts(with_d):
    """K = 2 over a two-entry prompt set, island i with weight 1 on entry i alone: every buffer of island i equals a single-search engine's
    under seed + i with entry i as its one target."""
    K, seed = 2, 11
    feats = np.random.default_rng(12).standard_normal((2, C["clip"][5])).astype(np.float32)
    isl = make(with_d, seed, islands=K)
    isl.set_targets(feats, [1.0, 1.0], "sum")
    isl.set_island_weights(np.eye(2, dtype=np.float32))
    singles = [make(with_d, seed + i) for i in range(K)]
    for i, e in enumerate(singles):
        e.set_target(feats[i])
    islands_equal_single_searches(isl, singles, x0(K), generations=(1, 2))
    F = isl.search_read("F", islands=True)["F"]
    assert not same(F[0], F[1])
    for e in [isl] + singles:
        e.close()


def test_own_prompts_refusals():
    feats = np.random.default_rng(12).standard_normal((2, C["clip"][5])).astype(np.float32)
    e = make(False, islands=2, migrate_every=1)
    with pytest.raises(RuntimeError, match=r"set_island_weights: set_targets\(\) first"):
        e.set_island_weights(np.eye(2))
    e.set_targets(feats, [1.0, 1.0], "sum")
    with pytest.raises(RuntimeError, match="own prompts are not combined with migration"):
        e.set_island_weights(np.eye(2))
    e.close()
    e = make(False, islands=2)
    e.set_targets(feats, [1.0, 1.0], "sum")
    with pytest.raises(RuntimeError, match="the table has 3 rows and the search 2 islands"):
        e.set_island_weights(np.ones((3, 2)))
    with pytest.raises(RuntimeError, match="the table has 3 columns and the prompt set 2 entries"):
        e.set_island_weights(np.ones((2, 3)))
    with pytest.raises(RuntimeError, match="island 1 has no non-zero weight"):
        e.set_island_weights(np.array([[1, 0], [0, 0]]))
    e.set_island_weights(np.eye(2))
    e.set_targets(np.concatenate([feats, feats[:1]]), [1.0, 1.0, 1.0], "sum")      # the set changes under the table
    with pytest.raises(RuntimeError, match="the engine's targets have changed: set_island_weights again"):
        e.search_init(x0(2).reshape(2 * POP, -1))
    e.close()
    e = make(False)
    e.set_targets(feats, [1.0, 1.0], "sum")
    with pytest.raises(RuntimeError, match="set_island_weights: this search has no islands"):
        e.set_island_weights(np.eye(2))
    e.close()


def test_off_means_off():
    """An engine that never calls the setter and one under set_search_islands(1, 0, 1) launch the same three kernels — there is one instance per
    phase, and a single search is its island 0 — and are the same search, bit for bit; only the island entry points tell them apart."""
    off, k1 = make(True, 4), make(True, 4, islands=1)
    rows = {}
    for name, e in (("off", off), ("k1", k1)):
        e.set_profiling(True)
        e.search_init(x0(1)[0])
        for gen in (1, 2):
            e.search_step(gen)
        rows[name] = sorted(r["name"] for r in e.profile() if r["name"].startswith("search."))
    assert rows["off"] == ["search.duplicates@ga_duplicates_kernel<4>", "search.survive@ga_survive_kernel", "search.vary@ga_vary_kernel<4>"]
    assert rows["k1"] == ["search.duplicates@ga_duplicates_kernel<4>", "search.survive@ga_survive_kernel", "search.vary@ga_vary_kernel<4>"]
    a, b = off.search_read(*ALL, "counts"), k1.search_read(*ALL, "counts")
    for k in a:
        assert same(a[k], b[k]), k
    lively(a["off_F"])
    with pytest.raises(RuntimeError, match="search_migrate: this search has no islands"):
        off.search_migrate(2)
    with pytest.raises(RuntimeError, match="search_read_islands: this search has no islands"):
        off.search_read_islands()
    off.close()
    k1.close()


def test_call_order_and_shape_refusals():
    from clip_glass_amd.engine import Engine
    e = make(True, islands=2)
    with pytest.raises(RuntimeError, match="set_search_islands: the engine is finalized"):
        e.set_search_islands(2)
    with pytest.raises(RuntimeError, match=r"search_migrate: search_init\(\) first"):
        e.search_migrate(1)
    with pytest.raises(ValueError, match="exactly pop = 16 rows"):
        e.search_init(x0(1)[0])
    e.search_init(x0(2).reshape(2 * POP, -1))
    with pytest.raises(RuntimeError, match="search_migrate: search_survive of this generation first"):
        e.search_migrate(1)
    e.search_vary(1)
    with pytest.raises(RuntimeError, match="whole minibatches inside the offspring rows"):
        e.search_evaluate(1, 12, 8)
    e.search_evaluate(1, 12, 4)      # a minibatch of island 1
    e.close()
    e = Engine(C["channels"][::-1], latent_size=C["latent"], mapping_layers=C["mapping"], batch_size=BS, use_discriminator=False, n_obj=1,
               max_pop=16, clip=C["clip"], noise_mode=1, noise_seed=3)
    with pytest.raises(RuntimeError, match="set_search_islands: the device search is off"):
        e.set_search_islands(2)
    e.set_search("ga", POP, XL, XU)
    with pytest.raises(RuntimeError, match="islands \\* pop = 24 rows are scored in one pass and max_pop is 16"):
        e.set_search_islands(3)
    with pytest.raises(RuntimeError, match=r"migrants must be in \[1, pop / 2 = 4\]"):
        e.set_search_islands(2, 1, 5)
    with pytest.raises(RuntimeError, match=r"islands must be in \[1, 64\]"):
        e.set_search_islands(0)
    e.set_search("cmaes", POP, XL, XU)
    with pytest.raises(RuntimeError, match="cmaes search, which keeps one distribution"):
        e.set_search_islands(2)
    e.close()


def _run(tmp, extra_argv, **extra):
    from clip_glass_amd import run
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_problem.npz")))
    cfg = dict(channels=C["channels"], dim_z=C["latent"], mapping_layers=C["mapping"], clip_geometry=C["clip"],
               clip_text_geometry=dict(width=64, layers=2), target_features=g["text_features"],
               problem_args=dict(n_var=C["latent"], n_obj=2, n_constr=C["latent"], xl=-10, xu=10))
    cfg.update(extra)
    os.makedirs(tmp, exist_ok=True)
    argv = ["--config", "StyleGAN2_ffhq_d", "--generations", "2", "--save-each", "100", "--tmp-folder", tmp, "--weights", "synthetic:0",
            "--clip-weights", "synthetic:0", "--pop-size", "8", "--device-search"] + extra_argv
    return run.main(argv, extra_config=cfg)


def test_islands_through_run(tmp_path):
    import pickle
    tmp = str(tmp_path / "shared")
    res = _run(tmp, ["--islands", "2", "--migrate-every", "1", "--migrants", "2"])
    assert len(res.islands) == 2 and len(res.pop) == 16 and all(len(r.pop) == 8 for r in res.islands)
    assert np.atleast_2d(res.X).shape[1] == C["latent"] and np.atleast_2d(res.F).shape[1] == 2
    # the overall front is the non-dominated front of the union: no row of any island dominates a row of it
    allF = np.array([p.F for p in res.pop])
    for f in np.atleast_2d(res.F):
        assert not ((allF <= f).all(axis=1) & (allF < f).any(axis=1)).any()
    files = set(os.listdir(tmp))
    assert {"output.jpg", "output-island-0.jpg", "output-island-1.jpg", "genetic_result", "genetic-it-final.jpg"} <= files
    saved = pickle.load(open(os.path.join(tmp, "genetic_result"), "rb"))
    assert set(saved) == {"X", "F", "G", "CV", "islands"} and len(saved["islands"]) == 2 and set(saved["islands"][0]) == {"X", "F", "G", "CV"}
    # own prompts: a second island on a feature of its own; the overall result is island 0's
    other = np.random.default_rng(13).standard_normal(C["clip"][5]).astype(np.float32)
    own = _run(str(tmp_path / "own"), [], island_prompts=[other])
    assert len(own.islands) == 2 and len(own.pop) == 8
    assert np.array_equal(np.atleast_2d(own.X), np.atleast_2d(own.islands[0].X)) and np.array_equal(np.atleast_2d(own.F), np.atleast_2d(own.islands[0].F))
    assert "output-island-1.jpg" in os.listdir(str(tmp_path / "own"))
