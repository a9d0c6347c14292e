"""Numpy mirror of the device search's rule for mixed rows (include/glass.h "Device search", paragraph "Mixed rows"; csrc/search.hip
ga_vary_bits_kernel): search_device_ref.vary on the real columns, half-uniform crossover and bit-flip on the bit columns, driven by
synth.search_uniforms at purposes 3 (gate), 4 (key) and 5 (flip).

Not a test module: tests/test_search_mixed_ref.py pins it by hand and by invariants, the GPU tests compare the kernels with it."""
import numpy as np

from clip_glass_amd import synth
import search_device_ref as SR


def hux_gate(seed, generation, n_matings, prob_x):
    """open bool [n_matings]: the mating exchanges bits."""
    m = np.arange(n_matings, dtype=np.uint32)
    return synth.search_uniforms(seed, generation, m, 0, synth.SEARCH_DRAW_BIT_GATE)[0] < float(prob_x)


def hux_keys(seed, generation, n_matings, n_real, n_bits):
    """keys uint32 [n_matings, n_bits]: the raw first Philox word at (mating, column n_real + j) — u0 = (w0 + 0.5) 2^-32 is exact in double, so
    w0 comes back from it exactly."""
    m = np.arange(n_matings, dtype=np.uint32)[:, None]
    j = (n_real + np.arange(n_bits, dtype=np.uint32))[None, :]
    u0 = synth.search_uniforms(seed, generation, m, j, synth.SEARCH_DRAW_BIT_KEY)[0]
    return (u0 * 2.0 ** 32 - 0.5).astype(np.uint32)


def hux_select(a, b, keys, gate=True):
    """One mating.  a, b: the parents' bit sections [n_bits]; keys uint32 [n_bits].  (D, selected): the columns (0-based in the bit section)
    where the parents differ, ascending, and those of them that are exchanged — the (|D| + 1) >> 1 smallest by (key, column); none where the
    gate is closed."""
    a, b = np.asarray(a), np.asarray(b)
    D = np.nonzero(a != b)[0]
    if not gate or D.size == 0:
        return D, D[:0]
    k = np.asarray(keys, dtype=np.uint32)[D]
    order = np.lexsort((D, k))      # by key, equal keys by column
    return D, np.sort(D[order[: (D.size + 1) >> 1]])


def bitflip(seed, generation, rows, n_real, n_bits, prob_flip):
    """flips bool [len(rows), n_bits] for the offspring rows `rows`."""
    r = np.asarray(rows, dtype=np.uint32)[:, None]
    j = (n_real + np.arange(n_bits, dtype=np.uint32))[None, :]
    return synth.search_uniforms(seed, generation, r, j, synth.SEARCH_DRAW_BIT_FLIP)[0] < float(prob_flip)


def hux_children(a, b, selected):
    """(child 0, child 1) of one mating's bit sections: child 0 takes b's bit at the selected columns, child 1 takes a's."""
    c0, c1 = np.array(a, copy=True), np.array(b, copy=True)
    c0[selected], c1[selected] = np.asarray(b)[selected], np.asarray(a)[selected]
    return c0, c1


def vary_mixed(X, n_real, rank, cd, xl, xu, eta_c, eta_m, prob_m, prob_x, prob_flip, seed, generation, keys=None):
    """The offspring of the fp32 mixed population X [pop, n_real + n_bits].  dict(real: search_device_ref.vary's dict for X[:, :n_real],
    off32 float32 [pop, n_var] the whole rows, bits float32 [pop, n_bits], gate bool [n_matings], D / selected: per-mating column arrays
    (0-based in the bit section), flips bool [pop, n_bits], parents).  keys: injected uint32 [n_matings, n_bits] instead of the drawn ones."""
    X = np.asarray(X, np.float32)
    pop, nv = X.shape
    n_bits = nv - n_real
    real = SR.vary(X[:, :n_real], rank, cd, xl, xu, eta_c, eta_m, prob_m, seed, generation)
    parents = real["parents"]
    nm = parents.shape[1]
    gate = hux_gate(seed, generation, nm, prob_x)
    if keys is None:
        keys = hux_keys(seed, generation, nm, n_real, n_bits)
    bits = np.empty((2 * nm, n_bits), np.float32)
    Ds, sels = [], []
    for m in range(nm):
        a, b = X[parents[0, m], n_real:], X[parents[1, m], n_real:]
        D, sel = hux_select(a, b, keys[m], bool(gate[m]))
        bits[2 * m], bits[2 * m + 1] = hux_children(a, b, sel)
        Ds.append(D)
        sels.append(sel)
    bits = bits[:pop]
    flips = bitflip(seed, generation, np.arange(pop), n_real, n_bits, prob_flip)
    bits = np.where(flips, np.float32(1.0) - bits, bits).astype(np.float32)
    off32 = np.concatenate([real["off32"], bits], axis=1)
    return dict(real=real, off32=off32, bits=bits, gate=gate, D=Ds, selected=sels, flips=flips, parents=parents)


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------------
BIT_PATTERNS = ("bernoulli", "all_differ", "all_but_one_differ", "identical", "one_differs")


def population_case(pop, n_real, n_bits, pattern, xl=-2.0, xu=2.0, seed=3):
    """X float32 [pop, n_real + n_bits], rank, cd: search_device_ref.population_case's real columns and one of the bit patterns — Bernoulli(0.005)
    rows; rows that alternate between a random section and its complement, so that parents from rows of different parity differ in every
    bit (|D| = n_bits), or in every bit but one (|D| = n_bits - 1: the other parity of |D|); identical sections; identical sections but for
    one column, which the odd rows have flipped (|D| = 1 between rows of different parity).  Which matings pair such rows is the
    tournament's business: a test that needs one asserts that the mirror's D shows it."""
    Xr, rank, cd = SR.population_case(pop, n_real, xl, xu, seed)
    rng = np.random.default_rng(seed + 17)
    if pattern == "bernoulli":
        B = rng.random((pop, n_bits)) < 0.005
    elif pattern in ("all_differ", "all_but_one_differ"):
        base = rng.random(n_bits) < 0.5
        B = np.where((np.arange(pop) % 2 == 0)[:, None], base[None, :], ~base[None, :])
        if pattern == "all_but_one_differ":
            B[:, n_bits // 3] = base[n_bits // 3]
    elif pattern == "identical":
        B = np.repeat((rng.random(n_bits) < 0.3)[None, :], pop, axis=0)
    elif pattern == "one_differs":
        B = np.repeat((rng.random(n_bits) < 0.3)[None, :], pop, axis=0)
        B[1::2, 7 % n_bits] ^= True
    else:
        raise ValueError(pattern)
    return np.concatenate([Xr, B.astype(np.float32)], axis=1), rank, cd


def check_bits(name, got_bits, m):
    """got_bits float32 [rows, n_bits] against the mirror's dict m: exactly equal, and nothing but 0.0 / 1.0."""
    ref = m["bits"]
    assert got_bits.shape == ref.shape, name
    assert np.isin(got_bits, (0.0, 1.0)).all(), "%s: a bit column holds something else than 0.0 / 1.0" % name
    wrong = np.argwhere(SR.bits(got_bits) != SR.bits(ref))
    assert wrong.size == 0, "%s: %d bits differ from the mirror, first at row %d bit %d" % (name, len(wrong), wrong[0][0], wrong[0][1])
