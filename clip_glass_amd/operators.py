"""Operators — mirror of /root/reference/operators.py (the API surface `run.py` uses:
`get_operators(config) -> dict(sampling, crossover, mutation)`).

The three custom Sampling classes are restated with builtin dtypes (np.float / np.bool are
gone from numpy >= 1.24, which breaks the reference as written: operators.py:10,18,34).
Crossover / mutation come from pymoo's factory exactly as in the reference when pymoo is
importable; without pymoo the factory names are returned as specs and the native driver
(search.py) applies the same operators per variable type from the `mask` entry.
"""
import numpy as np

try:
    from pymoo.model.sampling import Sampling
    from pymoo.factory import get_crossover, get_mutation, get_sampling
    HAVE_PYMOO = True
except ImportError:
    HAVE_PYMOO = False

    class Sampling:
        def __init__(self):
            pass

        def do(self, problem, n_samples, **kwargs):
            return self._do(problem, n_samples, **kwargs)

    def _spec(kind):
        def make(name, **kw):
            return dict(kind=kind, name=name, **kw)
        return make
    get_crossover, get_mutation, get_sampling = _spec("crossover"), _spec("mutation"), _spec("sampling")


class TruncatedNormalRandomSampling(Sampling):
    """operators.py:9-15"""

    def __init__(self, var_type=float):
        super().__init__()
        self.var_type = var_type

    def _do(self, problem, n_samples, **kwargs):
        from scipy.stats import truncnorm
        return truncnorm.rvs(-2, 2, size=(n_samples, problem.n_var)).astype(np.float32)


class NormalRandomSampling(Sampling):
    """operators.py:17-25"""

    def __init__(self, mu=0, std=1, var_type=float):
        super().__init__()
        self.mu, self.std, self.var_type = mu, std, var_type

    def _do(self, problem, n_samples, **kwargs):
        return np.random.normal(self.mu, self.std, size=(n_samples, problem.n_var))


class MappedNormalSampling(Sampling):
    """Sampling for a search in w / w+: z ~ N(0, 1) drawn as NormalRandomSampling draws it, sent through the generator's mapping network
    (problem.generator.map_latents) — the population starts where a z search starts, expressed as dlatents.  tile = n_lat repeats the
    dlatent for every style layer of a w+ row (layer-major)."""

    def __init__(self, dim_z, tile=1):
        super().__init__()
        self.dim_z, self.tile = int(dim_z), int(tile)

    def _do(self, problem, n_samples, **kwargs):
        z = np.random.normal(0, 1, size=(n_samples, self.dim_z))
        w = np.asarray(problem.generator.map_latents(z.astype(np.float32)), dtype=float)
        return np.tile(w, (1, self.tile))


class EditSampling(Sampling):
    """Sampling for a search that starts at a source row (config.edit_latent; generator.edit_start_population): the first call returns the
    source itself as row 0 and source + sigma * N(0, 1) below it, clipped to the problem's bounds; later calls (the refill after duplicate
    elimination) return perturbed rows only.  Draws come from numpy's global RNG, as the other samplings' do."""

    def __init__(self, source_row, sigma):
        super().__init__()
        self.source_row, self.sigma, self.started = np.asarray(source_row, dtype=np.float32), float(sigma), False

    def _do(self, problem, n_samples, **kwargs):
        from .generator import edit_start_population
        if problem.n_var != self.source_row.size:
            raise ValueError("edit_latent holds %d floats; the search varies %d" % (self.source_row.size, problem.n_var))
        X = edit_start_population(self.source_row, n_samples + int(self.started), self.sigma, problem.xl, problem.xu,
                                  lambda size: np.random.normal(0, 1, size=size))
        first, self.started = (1 if self.started else 0), True
        return X[first:]


class BinaryRandomSampling(Sampling):
    """operators.py:27-34"""

    def __init__(self, prob=0.5):
        super().__init__()
        self.prob = prob

    def _do(self, problem, n_samples, **kwargs):
        val = np.random.random((n_samples, problem.n_var))
        return (val < self.prob).astype(bool)


class MixedVariableSampling(Sampling):
    """pymoo.operators.mixed_variable_operator.MixedVariableSampling restated (used when pymoo is absent):
    each variable type is drawn by its own Sampling over the columns the mask assigns to it."""

    def __init__(self, mask, process):
        super().__init__()
        self.mask, self.process = np.asarray(mask), process

    def _do(self, problem, n_samples, **kwargs):
        X = np.empty((n_samples, len(self.mask)), dtype=float)
        for kind, sampling in self.process.items():
            cols = np.nonzero(self.mask == kind)[0]

            class _Sub:                      # the sub-problem pymoo hands to each per-type operator
                n_var = len(cols)
                xl = np.asarray(problem.xl)[cols] if np.ndim(problem.xl) else problem.xl
                xu = np.asarray(problem.xu)[cols] if np.ndim(problem.xu) else problem.xu
            X[:, cols] = np.asarray(sampling._do(_Sub, n_samples), dtype=float)
        return X


class IntegerRandomSampling(Sampling):
    """pymoo "int_random": uniform integers in [xl, xu]."""

    def _do(self, problem, n_samples, **kwargs):
        xl = np.broadcast_to(np.asarray(problem.xl, float), (problem.n_var,))
        xu = np.broadcast_to(np.asarray(problem.xu, float), (problem.n_var,))
        return np.floor(xl + np.random.random((n_samples, problem.n_var)) * (xu - xl + 1)).astype(float)


def get_operators(config):
    """operators.py:37-81.  The extra "mask" entry (variable types) is what the native driver (search.py)
    needs to apply the same per-type operators when pymoo is absent."""
    if config.config.split("_")[0] == "StyleGAN2":
        space = getattr(config, "latent_space", None) or "z"
        if getattr(config, "edit_latent", None) is not None:      # image editing: the search starts at the source row, in any space
            from .generator import DEFAULT_EDIT_SIGMA, load_edit_latent
            sigma = getattr(config, "edit_sigma", None)
            if space == "sub":        # the file's row is the subspace's base: the search starts at the zero row of coefficients
                from .subspace import row_width
                source = np.zeros(row_width(config), np.float32)
            else:
                source = load_edit_latent(config.edit_latent)
            return dict(sampling=EditSampling(source, DEFAULT_EDIT_SIGMA if sigma is None else sigma),
                        crossover=get_crossover("real_sbx", prob=1.0, eta=3.0),
                        mutation=get_mutation("real_pm", prob=0.5, eta=3.0))
        if space not in ("z", "sub"):      # same crossover and mutation; the initial population comes through the mapping network
            # (sub: unit-variance coefficients, drawn as z's variables are — NormalRandomSampling below)
            from .latent import stylegan2_n_lat
            return dict(sampling=MappedNormalSampling(config.dim_z, stylegan2_n_lat(config) if space == "w+" else 1),
                        crossover=get_crossover("real_sbx", prob=1.0, eta=3.0),
                        mutation=get_mutation("real_pm", prob=0.5, eta=3.0))
        return dict(sampling=NormalRandomSampling(),
                    crossover=get_crossover("real_sbx", prob=1.0, eta=3.0),
                    mutation=get_mutation("real_pm", prob=0.5, eta=3.0))
    if config.config in ("DeepMindBigGAN256", "DeepMindBigGAN512"):
        mask = ["real"] * config.dim_z + ["bool"] * config.num_classes
        process = {"real": TruncatedNormalRandomSampling(), "bool": BinaryRandomSampling(prob=5 / 1000)}
        if not HAVE_PYMOO:
            return dict(sampling=MixedVariableSampling(mask, process), mask=mask,
                        crossover=dict(kind="crossover", name="mixed",
                                       real=get_crossover("real_sbx", prob=1.0, eta=3.0), bool=get_crossover("bin_hux", prob=0.2)),
                        mutation=dict(kind="mutation", name="mixed",
                                      real=get_mutation("real_pm", prob=0.5, eta=3.0), bool=get_mutation("bin_bitflip", prob=10 / 1000)))
        from pymoo.operators.mixed_variable_operator import MixedVariableCrossover, MixedVariableMutation
        from pymoo.operators.mixed_variable_operator import MixedVariableSampling as PymooMixedSampling
        return dict(
            sampling=PymooMixedSampling(mask, process), mask=mask,
            crossover=MixedVariableCrossover(mask, {"real": get_crossover("real_sbx", prob=1.0, eta=3.0),
                                                    "bool": get_crossover("bin_hux", prob=0.2)}),
            mutation=MixedVariableMutation(mask, {"real": get_mutation("real_pm", prob=0.5, eta=3.0),
                                                  "bool": get_mutation("bin_bitflip", prob=10 / 1000)}))
    if config.config == "GPT2":
        return dict(sampling=get_sampling("int_random") if HAVE_PYMOO else IntegerRandomSampling(),
                    mask=["int"] * config.dim_z,
                    crossover=get_crossover("int_sbx", prob=1.0, eta=3.0),
                    mutation=get_mutation("int_pm", prob=0.5, eta=3.0))
    raise Exception("Unknown config")
