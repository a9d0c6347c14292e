"""sep-CMA-ES on the host (include/glass.h "Device search: sep-CMA-ES"): the float64 mirror of tests/cma_ref.py against search.minimize's
host "cmaes" bit for bit, the update bar against planted faults, convergence where the GA stalls, the box as a repair, the host-only
rules and the moments of the draws.  No GPU."""
import numpy as np
import pytest

import cma_ref as CR
from clip_glass_amd import search, synth
from clip_glass_amd.operators import NormalRandomSampling

XL, XU = -10.0, 10.0


class Quadratic:
    """f(x) = sum scale_j (x_j - centre_j)^2 over [xl, xu]^n; keeps every row it was asked to score."""
    n_obj = 1

    def __init__(self, centre, scale=None, n_obj=1):
        self.centre = np.asarray(centre, float)
        self.scale = np.ones_like(self.centre) if scale is None else np.asarray(scale, float)
        self.n_var, self.xl, self.xu, self.n_obj, self.rows = self.centre.size, XL, XU, n_obj, []

    def f(self, X):
        return ((np.asarray(X, float) - self.centre) ** 2 * self.scale).sum(axis=-1)

    def _evaluate(self, X, out):
        self.rows.append(np.array(X))
        out["F"] = np.repeat(self.f(X)[:, None], self.n_obj, axis=1)


def alternating(n):
    return np.where(np.arange(n) % 2 == 0, 3.0, -2.0)


def ellipsoid_scale(n, ratio=1e2):
    return ratio ** (np.arange(n) / max(n - 1, 1))


@pytest.mark.parametrize("n,lam", [(1, 4), (3, 5), (65, 16)])
def test_mirror_equals_host_bitwise(n, lam):
    seed, gens = 7, 5
    prob = Quadratic(alternating(n) * 0.5, ellipsoid_scale(n, 10.0))
    m0, d0, s0 = np.linspace(-0.5, 0.5, n), np.linspace(0.5, 2.0, n), 0.8
    seen = []
    res = search.minimize(prob, "cmaes", lam, gens - 1, None, seed=seed, cma_mean=m0, cma_diag=d0, cma_sigma=s0,
                          callback=lambda a: seen.append((a.n_gen, a.state.m.copy(), a.state.d.copy(), a.state.ps.copy(), a.state.pc.copy(), a.state.sigma)))
    st = CR.new_state(m0, d0, s0)
    for g in range(gens):
        X = CR.sample(st, lam, XL, XU, seed, g)
        assert np.array_equal(CR.bits(X), CR.bits(prob.rows[g].astype(np.float32))), "generation %d: the rows" % g
        st, _ = CR.update(st, X, prob.f(X), lam, XL, XU, g)
        for rec in [r for r in seen if r[0] == g]:
            for k, v in zip(("m", "d", "ps", "pc"), rec[1:5]):
                assert np.array_equal(CR.bits(st[k]), CR.bits(v)), "generation %d: %s" % (g, k)
            assert st["sigma"] == rec[5], "generation %d: sigma" % g
    host = res.state
    for k, v in (("m", host.m), ("d", host.d), ("ps", host.ps), ("pc", host.pc), ("best_X", host.best_X)):
        assert np.array_equal(CR.bits(st[k]), CR.bits(v)), k
    assert (st["sigma"], st["best_F"], st["ps_norm"], st["h"], st["skipped"]) == (host.sigma, host.best_F, host.ps_norm, host.h, host.skipped)
    assert [r[0] for r in seen] == list(range(1, gens)) and len(prob.rows) == gens
    assert np.array_equal(res.X, host.best_X.astype(float)) and res.F.shape == (1,) and res.sigma == host.sigma and len(res.pop) == lam


def planted_case():
    """A generation on which every planted fault moves the state: sigma large enough to clip, two tied rows among the mu best, and a
    p_sigma long enough that h = 0."""
    n, lam, seed, g = 8, 8, 3, 2
    st = CR.new_state(np.linspace(-8.0, 8.0, n), np.linspace(0.5, 2.0, n), 6.0)
    st["ps"], st["pc"], st["ps_norm"] = np.full(n, 4.0), np.linspace(-1.0, 1.0, n), 0.5
    X = CR.sample(st, lam, XL, XU, seed, g)
    raw = CR.sample_double(st, lam, XL, XU, seed, g, clip=False)
    F = np.arange(lam, dtype=float)[::-1].copy()
    F[[1, 5]] = -1.0      # the two best rows tie: (F, index) puts row 1 first
    return st, X, raw, F, lam, g


def test_update_bar_passes_the_host_rule_and_fails_every_planted_fault():
    st, X, raw, F, lam, g = planted_case()
    assert (np.abs(raw) > XU).mean() >= 0.1
    ref, mag = CR.update(st, X, F, lam, XL, XU, g, Xraw=raw)
    assert ref["h"] == 0 and ref["updated"] == 1 and list(ref["order"][:2]) == [1, 5]
    # the host rule, on the same state, passes the bar
    hs = search.CMAState(st["m"], st["d"], st["sigma"])
    hs.ps, hs.pc, hs.ps_norm = st["ps"].copy(), st["pc"].copy(), st["ps_norm"]
    search.cma_update(hs, search.cma_constants(lam, X.shape[1]), X, F, XL, XU, g)
    got = dict(m=hs.m, d=hs.d, ps=hs.ps, pc=hs.pc, sigma=hs.sigma, ps_norm=hs.ps_norm, h=hs.h, finite=lam, updated=1, skipped=hs.skipped,
               updates=hs.updates, order=search.cma_rank(F)[0], best_X=hs.best_X, best_F=hs.best_F)
    CR.check_update("host", got, ref, mag)
    for fault in CR.FAULTS:
        bad, _ = CR.update(st, X, F, lam, XL, XU, g, fault=fault, Xraw=raw)
        with pytest.raises(AssertionError):
            CR.check_update(fault, bad, ref, mag)


def run_cma(prob, gens=150, pop=16, seed=1):
    return search.minimize(prob, "cmaes", pop, gens, None, seed=seed, cma_mean=0.0, cma_diag=1.0, cma_sigma=1.0)


def test_converges_on_a_sphere_where_the_ga_does_not():
    n = 64
    prob = Quadratic(alternating(n))
    f0 = float(prob.f(np.zeros(n)))
    res = run_cma(prob)
    ratio = float(res.F[0]) / f0
    print("sphere n=64: cmaes best f / f(0) = %.3e after %d evaluations" % (ratio, sum(len(r) for r in prob.rows)))
    assert sum(len(r) for r in prob.rows) == 151 * 16
    assert float(prob.f(res.X)) == pytest.approx(float(res.F[0]), rel=1e-12)
    assert ratio <= 1e-2
    ga_prob = Quadratic(alternating(n))
    ga = search.minimize(ga_prob, "ga", 16, 150, NormalRandomSampling(), seed=1)
    ga_ratio = float(np.atleast_1d(ga.F)[0]) / f0
    print("sphere n=64: ga best f / f(0) = %.3e" % ga_ratio)
    assert ga_ratio >= 0.5


def test_converges_on_an_ellipsoid():
    n = 64
    prob = Quadratic(alternating(n), ellipsoid_scale(n))
    ratio = float(run_cma(prob).F[0]) / float(prob.f(np.zeros(n)))
    print("ellipsoid n=64: cmaes best f / f(0) = %.3e" % ratio)
    assert ratio <= 5e-2


def test_optimum_outside_the_box():
    n = 64
    prob = Quadratic(np.full(n, 12.0))
    sigmas = []
    res = search.minimize(prob, "cmaes", 16, 150, None, seed=1, cma_mean=0.0, cma_diag=1.0, cma_sigma=1.0,
                          callback=lambda a: sigmas.append(a.state.sigma))
    rows = np.concatenate(prob.rows)
    assert rows.min() >= XL and rows.max() <= XU
    assert np.isfinite(sigmas).all() and min(sigmas) > 0 and np.isfinite(res.sigma) and res.sigma > 0
    print("optimum outside the box: best %.1f (floor 256)" % float(res.F[0]))
    assert float(res.F[0]) <= 1.25 * 256


def test_host_only_rules():
    from clip_glass_amd.engine import search_supported
    for pop, n_obj, ok in ((3, 1, False), (1025, 1, False), (4, 2, False), (4, 1, True), (1024, 1, True)):
        got, msg = search_supported(pop, 512, n_obj, "cmaes")
        assert got == ok and (ok or "cmaes" in msg), (pop, n_obj, msg)
    assert not search_supported(1024, 1 << 21, 1, "cmaes")[0]
    with pytest.raises(ValueError, match="cmaes: minimises one objective"):
        search.minimize(Quadratic(np.zeros(4), n_obj=2), "cmaes", 8, 1, None, cma_mean=0.0, cma_diag=1.0)
    for kind in ("bool", "int"):
        with pytest.raises(ValueError, match="cmaes: samples real-valued rows and this mask has %s columns" % kind):
            search.minimize(Quadratic(np.zeros(4)), "cmaes", 8, 1, None, mask=["real"] * 3 + [kind], cma_mean=0.0, cma_diag=1.0)
    with pytest.raises(ValueError, match="cmaes: pop_size 3 is under 4"):
        search.minimize(Quadratic(np.zeros(4)), "cmaes", 3, 1, None, cma_mean=0.0, cma_diag=1.0)


def test_initial_distribution_is_the_samplings_own():
    prob = Quadratic(np.zeros(32))
    m0, d0, s0 = search.cma_initial(prob, NormalRandomSampling(), 5)
    np.random.seed(5)
    S = np.random.normal(0, 1, size=(search.CMA_INIT_ROWS, 32))
    assert np.array_equal(m0, S.mean(axis=0)) and np.array_equal(d0, S.var(axis=0)) and s0 == 1.0
    assert np.abs(m0).max() < 5 / np.sqrt(search.CMA_INIT_ROWS) and np.abs(d0 - 1).max() < 5 * np.sqrt(2.0 / search.CMA_INIT_ROWS)


def test_moments_of_the_draws():
    N = 1 << 20
    z = synth.search_normals(11, 3, np.arange(1024)[:, None], np.arange(1024)[None, :])
    assert z.shape == (1024, 1024) and z.dtype == np.float64 and np.isfinite(z).all()
    assert abs(z.mean()) <= 5 / np.sqrt(N)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / N)
    assert abs((z[:, :-1] * z[:, 1:]).mean()) <= 5 / np.sqrt(N - 1024)
    # a draw is a pure function of its counter
    assert np.array_equal(z[5:7, 100:200], synth.search_normals(11, 3, np.arange(5, 7)[:, None], np.arange(100, 200)[None, :]))
    assert not np.array_equal(z[:2], synth.search_normals(11, 4, np.arange(2)[:, None], np.arange(1024)[None, :]))


def test_configs_cmaes_cannot_search_are_refused_by_name():
    """generator.search_options: before any weight is looked for, each refusal names what to use instead."""
    import types
    from clip_glass_amd.config import get_config
    from clip_glass_amd.generator import Generator, search_options

    def cfg(name, **kw):
        return types.SimpleNamespace(config=name, **dict(get_config(name), algorithm="cmaes", **kw))
    assert search_options(cfg("StyleGAN2_ffhq_nod")) == dict(sigma=1.0)
    assert search_options(cfg("StyleGAN2_ffhq_nod", cma_sigma=0.25, lpips_target="t.png", lpips_lambda=0.5)) == dict(sigma=0.25)
    assert search_options(types.SimpleNamespace(config="StyleGAN2_ffhq_d", **get_config("StyleGAN2_ffhq_d"))) is None      # nsga2: nothing to say
    for bad, match in ((cfg("StyleGAN2_ffhq_d"), "has 2 .*use a _nod config, or nsga2"),
                       (cfg("StyleGAN2_ffhq_nod", lpips_target="t.png"), "lpips_lambda = 0 .*lpips_lambda > 0, or use nsga2"),
                       (cfg("StyleGAN2_ffhq_nod", edit_latent="r.npy", anchor_lambda=0.0), "anchor_lambda = 0 .*anchor_lambda > 0, or use nsga2"),
                       (cfg("StyleGAN2_ffhq_nod", prompt_mode="pareto", prompts=[("a", 1.0)]), "pareto prompt set .*prompt_mode sum, or nsga2"),
                       (cfg("DeepMindBigGAN256"), "BigGAN row is .*use ga"),
                       (cfg("GPT2"), "GPT2 config searches integer tokens: use ga"),
                       (cfg("StyleGAN2_ffhq_nod", dist=True), "--dist.* run one rank, or ga / nsga2"),
                       (cfg("StyleGAN2_ffhq_nod", cma_sigma=0.0), "cma_sigma must be finite and positive")):
        with pytest.raises(ValueError, match=match):
            search_options(bad)
    with pytest.raises(ValueError, match="use a _nod config, or nsga2"):      # the Generator refuses before it looks for ./stylegan2/weights
        Generator(cfg("StyleGAN2_ffhq_d"))
