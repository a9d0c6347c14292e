"""Island populations, the parts that need no GPU: glass_search_islands_supported at each of its limits (the rule is host only), the refusals of
run.py / the Generator's island_options and of search.minimize by their messages, the counting of --island-prompt, the islands' weight table
and the shape of an island Result."""
import types

import numpy as np
import pytest

from clip_glass_amd import run, search
from clip_glass_amd.engine import SEARCH_MAX_ISLANDS, search_islands_supported
from clip_glass_amd.generator import island_config, island_options, island_weight_table


def ok(*a, **k):
    good, msg = search_islands_supported(*a, **k)
    return good, msg


def test_supported_at_each_limit():
    assert ok(1, 2, 1, 1, "ga")[0] and ok(SEARCH_MAX_ISLANDS, 1024, 512, 2, "nsga2", 3, 512)[0]
    good, msg = ok(0, 8, 4, 1, "ga")
    assert not good and "islands must be in [1, 64], got 0" in msg
    good, msg = ok(SEARCH_MAX_ISLANDS + 1, 8, 4, 1, "ga")
    assert not good and "islands must be in [1, 64], got 65" in msg
    # pop keeps its limits per island
    assert not ok(2, 1, 4, 1, "ga")[0] and "pop must be in [2, 1024]" in ok(2, 1025, 4, 1, "ga")[1]
    # islands * pop * n_var below 2^31: 64 * 1024 * 32767 fits, 64 * 1024 * 32768 = 2^31 does not (each island alone would)
    assert ok(64, 1024, 32767, 1, "ga")[0]
    good, msg = ok(64, 1024, 32768, 1, "ga")
    assert not good and "islands * pop * n_var must be below 2^31" in msg and search.DEVICE_MAX_POP == 1024
    # migrants in [1, pop / 2], migrate_every >= 0
    assert ok(3, 8, 4, 1, "ga", 1, 4)[0]
    for n in (0, 5):
        good, msg = ok(3, 8, 4, 1, "ga", 1, n)
        assert not good and "migrants must be in [1, pop / 2 = 4]" in msg
    good, msg = ok(3, 8, 4, 1, "ga", -1, 1)
    assert not good and "migrate_every must be >= 0" in msg
    # GA and NSGA-II only; the single search's own rules still hold
    good, msg = ok(2, 8, 4, 1, "cmaes")
    assert not good and "cmaes keeps one distribution" in msg
    good, msg = ok(2, 8, 4, 2, "ga")
    assert not good and "n_obj = 1" in msg
    assert not ok(2, 8, 4, 1, "annealing")[0]


def cfg(**kw):
    base = dict(config="StyleGAN2_ffhq_d", task="txt2img", algorithm="nsga2", pop_size=16, batch_size=4, device_search=True)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_island_options_default_and_counting():
    assert island_options(cfg()) is None and island_options(cfg(device_search=False)) is None
    assert island_options(cfg(islands=3)) == dict(islands=3, migrate_every=0, migrants=1, prompts=[])
    assert island_options(cfg(islands=3, migrate_every=5, migrants=8))["migrants"] == 8
    # --target is island 0's prompt and each island prompt adds an island; --islands, if given, must agree
    assert island_options(cfg(island_prompts=["a cat", "a dog"]))["islands"] == 3
    assert island_options(cfg(island_prompts=["a cat"], islands=2))["islands"] == 2
    with pytest.raises(ValueError, match="islands=2 does not agree with island_prompts.*which makes 3"):
        island_options(cfg(island_prompts=["a cat", "a dog"], islands=2))
    c = cfg(island_prompts=["a cat"], prompts=[("glasses", -0.5)])
    out = island_config(c, island_options(c))
    assert out.prompts == [("glasses", -0.5), ("a cat", 1.0)] and c.prompts == [("glasses", -0.5)]
    assert island_config(c, None) is c


@pytest.mark.parametrize("kw,msg", [
    (dict(islands=2, task="img2txt", config="GPT2", pop_size=100), "the GPT2 config searches integer token rows"),
    (dict(islands=2, dist=True), "islands run on one rank"),
    (dict(islands=2, algorithm="cmaes"), "algorithm cmaes keeps one distribution"),
    (dict(islands=2, device_search=False), "the host search has no islands"),
    (dict(migrate_every=2, device_search=False), "the host search has no islands"),
    (dict(islands=65), r"islands must be in \[1, 64\], got 65"),
    (dict(islands=2, migrants=9), r"migrants must be in \[1, pop_size / 2 = 8\]"),
    (dict(islands=2, migrate_every=-1), "migrate_every must be >= 0"),
    (dict(island_prompts=["a cat"], migrate_every=3), "a migrant's F would be stale under another island's prompt"),
    (dict(island_prompts=["a cat"], prompt_mode="pareto"), "island_prompts with prompt_mode 'pareto'"),
    (dict(island_prompts=["a cat"], edit_image="x.jpg", source_text="a face"), "island_prompts with an edit source"),
])
def test_island_options_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        island_options(cfg(**kw))


@pytest.mark.parametrize("argv,msg", [
    (["--config", "GPT2", "--islands", "2", "--device-search"], "the GPT2 config searches integer token rows"),
    (["--islands", "2", "--device-search", "--dist"], "islands run on one rank"),
    (["--config", "StyleGAN2_ffhq_nod", "--algorithm", "cmaes", "--islands", "2", "--device-search"], "algorithm cmaes keeps one distribution"),
    (["--islands", "2"], "the host search has no islands"),
    (["--island-prompt", "a cat", "--device-search", "--migrate-every", "2"], "a migrant's F would be stale"),
    (["--island-prompt", "a cat", "--device-search", "--prompt-mode", "pareto"], "island_prompts with prompt_mode 'pareto'"),
    (["--island-prompt", "a cat", "--device-search", "--edit-image", "x.jpg", "--source-text", "a face"], "island_prompts with an edit source"),
    (["--island-prompt", "a cat", "--island-prompt", "a dog", "--islands", "2", "--device-search"], "does not agree with island_prompts"),
])
def test_run_refuses_before_anything_is_loaded(argv, msg, tmp_path):
    # (no weights are given: a run that got as far as loading them would fail on the missing files, not with these messages)
    with pytest.raises(ValueError, match=msg):
        run.main(argv + ["--tmp-folder", str(tmp_path), "--weights", str(tmp_path / "none")])


def test_minimize_refusals():
    problem = types.SimpleNamespace(n_var=4, n_obj=1, xl=-1.0, xu=1.0)
    with pytest.raises(ValueError, match="islands=3 without device=True: the host search has no islands"):
        search.minimize(problem, "ga", 8, 1, None, islands=3)
    with pytest.raises(ValueError, match="islands=2 with algorithm cmaes"):
        search.minimize(problem, "cmaes", 8, 1, None, islands=2, device=True)
    with pytest.raises(ValueError, match="islands must be >= 1"):
        search.minimize(problem, "ga", 8, 1, None, islands=0)
    # an engine that was set up without islands (or for another count) is refused by name, before anything is sampled
    engine = types.SimpleNamespace(search_pop=8)
    problem = types.SimpleNamespace(n_var=4, n_obj=1, xl=-1.0, xu=1.0, engine=engine, config=types.SimpleNamespace(batch_size=4))
    with pytest.raises(ValueError, match="islands=2, and the engine's search was set up without islands"):
        search.minimize(problem, "ga", 8, 1, None, islands=2, device=True)
    engine.search_islands = 3
    with pytest.raises(ValueError, match="islands=2, and the engine's search was set up for 3"):
        search.minimize(problem, "ga", 8, 1, None, islands=2, device=True)
    with pytest.raises(ValueError, match="islands=1, and the engine's search was set up for 3"):
        search.minimize(problem, "ga", 8, 1, None, device=True)


def test_island_weight_table():
    # the caller's set (target 1, a negative prompt) in front, two island prompts behind it
    t = island_weight_table([1.0, -0.5, 1.0, 1.0], 3)
    assert np.array_equal(t, np.array([[1, -0.5, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)) and t.dtype == np.float32
    assert np.array_equal(island_weight_table([2.0, 1.0], 2), np.array([[2, 0], [0, 1]], np.float32))


def test_island_result_shapes():
    rng = np.random.default_rng(0)
    K, pop, nv = 3, 4, 5
    X, F = rng.standard_normal((K * pop, nv)), rng.standard_normal((K * pop, 1))
    F[7, 0] = -9.0      # the best row overall lives on island 1
    res = search._island_result(X, F, False, K, pop, False)
    assert len(res.islands) == K and len(res.pop) == K * pop and np.array_equal(res.X, X[7]) and np.array_equal(res.islands[1].X, X[7])
    assert all(len(r.pop) == pop and r.X.shape == (nv,) for r in res.islands)
    own = search._island_result(X, F, False, K, pop, True)      # own prompts: the overall result is island 0's
    assert len(own.pop) == pop and np.array_equal(own.X, own.islands[0].X) and np.array_equal(own.X, X[int(np.argmin(F[:pop, 0]))])
    F2 = rng.standard_normal((K * pop, 2))
    res = search._island_result(X, F2, True, K, pop, False)     # NSGA-II: the non-dominated front of the union
    front = search.fast_non_dominated_sort(F2)[0][0]
    assert np.array_equal(res.F, F2[front]) and all(np.atleast_2d(r.X).shape[1] == nv for r in res.islands)
