"""Float64 restatements of the prompt-set kernels (csrc/score.hip; include/glass.h "Prompt sets"), each with its float32 twin
(test infrastructure).  Built on small_ops_ref.cosine / seq_sum: a column of a set is that file's cosine against the entry, the mean over
the views its cosine_views, so tests/test_small_ops_ref.py's pins (torch.cosine_similarity, the oracle's fitness) carry over.
tests/test_prompt_set_ref.py pins what is new here — the weighted combination and the sign rule."""
import numpy as np

import small_ops_ref as R


def weight_sum(weights, dt=np.float64):
    """W = sum_t |w_t|, added in the order t = 0 .. T - 1."""
    return R.seq_sum(np.abs(np.asarray(weights, dtype=dt)), dt)


def combine(set_sim, weights, dt=np.float64):
    """Mode sum: acc = 0; acc = acc + w_t * cbar[:, t] for t = 0 .. T - 1 (product and sum rounded separately in the twin); acc / W."""
    c, w = np.asarray(set_sim, dtype=dt), np.asarray(weights, dtype=dt)
    acc = np.zeros(c.shape[0], dt)
    for t in range(c.shape[1]):
        acc = acc + w[t] * c[:, t]
    return acc / weight_sum(w, dt)


def cosine_set(feat, targets, weights, dt=np.float64):
    """feat [P, V, D] (V = 1: no views), targets [T, D], weights [T] -> (view_sim [P, V]: entry 0's cosines per view, set_sim [P, T]: per
    entry the mean over the views summed in the order v = 0 .. V - 1 — the cosine itself for V = 1 —, sim [P]: combine())."""
    f = np.asarray(feat, dtype=dt)
    P, V, D = f.shape
    targets = np.asarray(targets, dtype=dt)
    cols, view0 = [], None
    for t in range(targets.shape[0]):
        vs, mean = R.cosine_views(f, targets[t], dt)
        if t == 0:
            view0 = vs
        cols.append(vs[:, 0] if V == 1 else mean)
    set_sim = np.stack(cols, axis=1)
    return view0, set_sim, combine(set_sim, weights, dt)


def assemble_F_set(set_sim, weights, dis=None, lp=None, dt=np.float64):
    """Mode pareto: F[:, t] = set_sim[:, t] where w_t < 0, else -set_sim[:, t]; then relu(1 - dis); then lp (each where given)."""
    c, w = np.asarray(set_sim, dtype=dt), np.asarray(weights, dtype=dt)
    cols = [np.where(w[None, :] < 0, c, -c)]
    if dis is not None:
        cols.append(np.maximum(dt(1) - np.asarray(dis, dtype=dt), dt(0))[:, None])
    if lp is not None:
        cols.append(np.asarray(lp, dtype=dt)[:, None])
    return np.concatenate(cols, axis=1)
