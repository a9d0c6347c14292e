"""Float64 mirror of the sep-CMA-ES rule, written from include/glass.h "Device search: sep-CMA-ES" (not from clip_glass_amd/search.py), and the
bars the kernels of csrc/cmaes.hip are held to.

A state is a dict: m, d, ps, pc float64 [n]; sigma, ps_norm; h, finite, updated, skipped, updates; best_X float32 [n], best_F.  update()
returns the next state and, for every float element, the sum of the magnitudes of the terms it is built from: the update bar is 1e-12 of
that (contraction is off on the device, so only exp / pow and the summation order of ||p_sigma|| can differ at all).

`fault` plants one mistake, by name, so that tests/test_cma_ref.py can show the bar fails on it."""
import numpy as np

from clip_glass_amd import synth

BLOCK = 256
FAULTS = ("weights", "c_sigma", "no_h", "unclipped", "tie", "sigma_first", "yw2")
UPDATE_RTOL = 1e-12


def constants(lam, n, fault=None):
    mu = lam // 2
    w = np.log(mu + 0.5) - np.log(np.arange(1, mu + 1, dtype=float))
    raw = w
    w = w / w.sum()
    mu_eff = 1.0 / (w * w).sum()
    c_sigma = (mu_eff + 2.0) / (n + mu_eff + 5.0)
    if fault == "c_sigma":
        c_sigma = 2.0 / (n + 5.0)
    d_sigma = 1.0 + 2.0 * max(0.0, np.sqrt((mu_eff - 1.0) / (n + 1.0)) - 1.0) + c_sigma
    c_c = (4.0 + mu_eff / n) / (n + 4.0 + 2.0 * mu_eff / n)
    c_1 = 2.0 / ((n + 1.3) ** 2 + mu_eff)
    c_mu = min(1.0 - c_1, 2.0 * (mu_eff - 2.0 + 1.0 / mu_eff) / ((n + 2.0) ** 2 + mu_eff))
    c_1 = min(1.0, c_1 * (n + 2.0) / 3.0)
    c_mu = min(1.0 - c_1, c_mu * (n + 2.0) / 3.0)
    chi = np.sqrt(float(n)) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n))
    return dict(mu=mu, w=raw if fault == "weights" else w, mu_eff=mu_eff, c_sigma=c_sigma, d_sigma=d_sigma, c_c=c_c, c_1=c_1, c_mu=c_mu, chi=chi)


def new_state(m, d, sigma, n=None):
    n = np.size(m) if n is None else n
    return dict(m=np.broadcast_to(np.asarray(m, float), (n,)).copy(), d=np.broadcast_to(np.asarray(d, float), (n,)).copy(), ps=np.zeros(n),
                pc=np.zeros(n), sigma=float(sigma), ps_norm=0.0, h=0, finite=0, updated=0, skipped=0, updates=0,
                best_X=np.zeros(n, np.float32), best_F=np.inf)


def sample_double(state, lam, xl, xu, seed, g, rows=None, clip=True):
    """x of the header's step 1 BEFORE the rounding to fp32, float64 [rows, n]; clip=False: m + (sigma sqrt(d)) z alone."""
    rows = np.arange(lam) if rows is None else np.asarray(rows)
    z = synth.search_normals(seed, g, rows[:, None], np.arange(state["m"].size)[None, :])
    x = state["m"] + (state["sigma"] * np.sqrt(state["d"])) * z
    return np.minimum(np.maximum(x, xl), xu) if clip else x


def sample(state, lam, xl, xu, seed, g, rows=None):
    return sample_double(state, lam, xl, xu, seed, g, rows).astype(np.float32)


def rank(F, fault=None):
    """(order, finite): by (F, index), -0.0 tying 0.0; non-finite rows last, by index."""
    F = np.asarray(F, float).reshape(-1)
    keyed = sorted(((float(f) + 0.0, -i if fault == "tie" else i) for i, f in enumerate(F) if np.isfinite(f)))
    order = [abs(i) for _, i in keyed] + [i for i, f in enumerate(F) if not np.isfinite(f)]
    return np.array(order, np.int64), len(keyed)


def sum_squares(v):
    """sum v^2 as the header partitions it: parts of 256 variables in index order, the parts in order."""
    total = 0.0
    for b in range(0, v.size, BLOCK):
        part = 0.0
        for x in v[b:b + BLOCK]:
            part = part + x * x
        total = total + part
    return total


def update(state, X, F, lam, xl, xu, g, fault=None, Xraw=None):
    """(next state, magnitudes) of steps 3 and 4 on the rows X float32 [lam, n] as they were evaluated and their F [lam].  Xraw: the unclipped
    samples, used only by the planted fault "unclipped"."""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    n = s["m"].size
    c = constants(lam, n, fault)
    order, finite = rank(F, fault)
    s["order"], s["finite"] = order, finite
    mag = {}
    if finite < c["mu"]:
        s["updated"], s["skipped"], s["best_src"] = 0, s["skipped"] + 1, -1
        return s, mag
    s["updated"], s["updates"], s["best_src"] = 1, s["updates"] + 1, -1
    Fb = np.asarray(F).reshape(-1)[order[0]]
    if Fb < s["best_F"]:
        s["best_X"], s["best_F"], s["best_src"] = np.asarray(X[order[0]], np.float32).copy(), float(Fb), int(order[0])
    m, d, sigma, w = state["m"], state["d"], state["sigma"], c["w"]
    rows = np.asarray(Xraw if fault == "unclipped" else X)
    yw, s2, ya = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(c["mu"]):
        y = (rows[order[i]].astype(float) - m) / sigma
        yw = yw + w[i] * y
        s2 = s2 + w[i] * (y * y)
        ya = ya + w[i] * np.abs(y)
    s["m"] = m + sigma * yw
    mag["m"] = np.abs(m) + sigma * ya
    a_s = np.sqrt(c["c_sigma"] * (2.0 - c["c_sigma"]) * c["mu_eff"])
    ps = (1.0 - c["c_sigma"]) * state["ps"] + a_s * yw / np.sqrt(d)
    mag["ps"] = np.abs((1.0 - c["c_sigma"]) * state["ps"]) + a_s * ya / np.sqrt(d)
    s["ps"] = ps
    norm = np.sqrt(sum_squares(ps))
    s["ps_norm"] = float(norm)
    mag["ps_norm"] = float(np.sqrt(sum_squares(mag["ps"])))
    s["threshold_ratio"] = float(norm / np.sqrt(1.0 - np.power(1.0 - c["c_sigma"], 2.0 * (g + 1.0))) / ((1.4 + 2.0 / (n + 1.0)) * c["chi"]))
    h = 1.0 if norm / np.sqrt(1.0 - np.power(1.0 - c["c_sigma"], 2.0 * (g + 1.0))) < (1.4 + 2.0 / (n + 1.0)) * c["chi"] else 0.0
    s["h"] = int(h)
    a_c = np.sqrt(c["c_c"] * (2.0 - c["c_c"]) * c["mu_eff"])
    pc = (1.0 - c["c_c"]) * state["pc"] + (h * a_c) * yw
    mag["pc"] = np.abs((1.0 - c["c_c"]) * state["pc"]) + (h * a_c) * ya
    s["pc"] = pc
    keep = 0.0 if fault == "no_h" else ((1.0 - h) * c["c_c"]) * (2.0 - c["c_c"])
    rank_mu = yw * yw if fault == "yw2" else s2
    s["d"] = ((1.0 - c["c_1"]) - c["c_mu"]) * d + c["c_1"] * (pc * pc + keep * d) + c["c_mu"] * rank_mu
    mag["d"] = np.abs(((1.0 - c["c_1"]) - c["c_mu"]) * d) + c["c_1"] * (mag["pc"] * mag["pc"] + keep * d) + c["c_mu"] * s2
    step_norm = state["ps_norm"] if fault == "sigma_first" else norm
    arg = min(1.0, (c["c_sigma"] / c["d_sigma"]) * (step_norm / c["chi"] - 1.0))
    free = sigma * np.exp(arg)
    s["sigma"] = float(min(max(free, 1e-10), xu - xl))
    s["sigma_free"] = float(free)      # before the clamp: which clamp, if any, a test hit
    mag["sigma"] = float(free) * (1.0 + (c["c_sigma"] / c["d_sigma"]) * (mag["ps_norm"] / c["chi"] + 1.0))
    return s, mag


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_update(name, got, ref, mag, rtol=UPDATE_RTOL):
    """The update bar: every float element of the state within rtol of the magnitudes it is built from; the discrete outcomes exact."""
    for k in ("h", "finite", "updated", "skipped", "updates"):
        assert int(got[k]) == int(ref[k]), "%s: %s is %r, the mirror says %r" % (name, k, got[k], ref[k])
    assert np.array_equal(np.asarray(got["order"]), np.asarray(ref["order"])), "%s: order" % name
    assert np.array_equal(bits(np.asarray(got["best_X"], np.float32)), bits(np.asarray(ref["best_X"], np.float32))), "%s: best_X" % name
    assert np.float32(got["best_F"]) == np.float32(ref["best_F"]) or (np.isinf(got["best_F"]) and np.isinf(ref["best_F"])), "%s: best_F" % name
    if not ref["updated"]:
        return
    for k in ("m", "ps", "pc", "d", "sigma", "ps_norm"):
        g, r = np.asarray(got[k], float), np.asarray(ref[k], float)
        err = np.abs(g - r) / np.maximum(np.asarray(mag[k], float), 1e-300)
        assert np.isfinite(g).all() and err.max() <= rtol, "%s: %s is off by %.3e of its terms' magnitudes (bar %.0e)" % (name, k, err.max(), rtol)


def check_sample(name, got, state, lam, xl, xu, seed, g, rows=None):
    """The sample bar: every element within 1 fp32 ulp of the mirror's double rounded to fp32 (device log / cos), inside the bounds, and an
    element the mirror clips exactly at the bound."""
    ref64 = sample_double(state, lam, xl, xu, seed, g, rows)
    raw = sample_double(state, lam, xl, xu, seed, g, rows, clip=False)
    ref = ref64.astype(np.float32)
    got = np.asarray(got, np.float32)
    assert got.shape == ref.shape and np.isfinite(got).all(), name
    ulp = np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))
    bad = np.abs(got.astype(float) - ref.astype(float)) > ulp
    assert not bad.any(), "%s: %d elements beyond 1 fp32 ulp, worst %.3e ulps" % (
        name, bad.sum(), (np.abs(got.astype(float) - ref.astype(float)) / ulp).max())
    assert (got >= np.float32(xl)).all() and (got <= np.float32(xu)).all(), "%s: outside the bounds" % name
    margin = 1e-9 * (xu - xl)      # (clipped by a margin no rounding of log / cos can cross)
    lo, hi = raw < xl - margin, raw > xu + margin
    assert (got[lo] == np.float32(xl)).all() and (got[hi] == np.float32(xu)).all(), "%s: a clipped element is not exactly the bound" % name
    return float((lo | hi).mean())
